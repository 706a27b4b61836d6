"""Inputs shared by tests/test_harrisgrid_cpu.py and tests/test_gpu_harrisgrid.py."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def crops():
    """The 256x192 lenna and 320x200 hut crops of the reference's test images (tests/golden/fast_rosten.npz)."""
    z = np.load(os.path.join(GOLD, "fast_rosten.npz"))
    out = {}
    for name, key in (("lenna", "lenna_256x192_img"), ("hut", "hut_320x200_img")):
        img = z[key]
        h, w = img.shape
        out[name] = np.ascontiguousarray(img[:h & ~3, :w & ~3])
    return out


def squares(pts, size=96):
    """Background 50 with 5x5 squares of 200 whose top-left pixels are pts: translated copies of one pattern have
    bit-equal responses, so which of them a cell reports is the tie order's decision."""
    img = np.full((size, size), 50, np.uint8)
    for x, y in pts:
        img[y:y + 5, x:x + 5] = 200
    return img


# pairs in one row, in one column, and apart in both; then a comb of squares through the centre cell whose Harris
# maxima (a square's bottom-right pixel) sit on rows 7, 16 and 12 of the cell: raster order reports the first, the CUDA
# launch order (rows 0, 4, 8, .. share the first warp) the second
TIE_CASES = [[(36, 37), (50, 37)], [(36, 37), (36, 50)], [(35, 36), (52, 47)], [(34, 35), (44, 44), (54, 40)]]
