#!/usr/bin/env python3
"""Generate tests/golden/harrisgrid.npz: feature grids and keep masks of the grid Harris / Shi-Tomasi detector
(vilib::HarrisGPU) from tests/harris_ref.py on the two crops of fast_rosten.npz.  These pin the restatement against
regressions; they are not reference outputs (the reference's detector is CUDA).

    python tests/golden/make_harrisgrid_golden.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import harris_ref as hr  # noqa: E402

# (min_level, max_level, hborder, vborder, filter_border, use_harris, k * 1000, quality * 100, tie_rule, cell_w, cell_h)
CONFIGS = [
    (0, 1, 0, 0, hr.BORDER_SKIP, 1, 40, 10, 0, 32, 32),   # test_harris.cpp:143-154
    (0, 1, 0, 0, hr.BORDER_SKIP, 0, 40, 10, 0, 32, 32),
    (0, 3, 0, 0, hr.BORDER_SKIP, 1, 40, 10, 0, 32, 32),
    (0, 3, 0, 0, hr.BORDER_SKIP, 0, 40, 10, 1, 32, 32),
    (1, 3, 8, 5, hr.BORDER_ZERO, 1, 40, 0, 0, 32, 32),
    (0, 2, 0, 0, hr.BORDER_REPLICATE, 0, 40, 90, 0, 32, 32),
    (0, 2, 0, 0, hr.BORDER_REFLECT, 1, 150, 10, 1, 32, 32),
    (0, 2, 0, 0, hr.BORDER_WRAP, 1, 40, 10, 0, 32, 32),
    (0, 3, 0, 0, hr.BORDER_REFLECT_101, 0, 40, 10, 0, 32, 32),
    (0, 2, 16, 16, hr.BORDER_REFLECT_101, 1, 40, 10, 0, 32, 32),
    (0, 3, 0, 0, hr.BORDER_SKIP, 1, 40, 10, 0, 64, 64),
    (0, 2, 0, 0, hr.BORDER_WRAP, 0, 40, 0, 0, 64, 32),
]


def crops():
    z = np.load(os.path.join(OUT, "fast_rosten.npz"))
    out = {}
    for name, key in (("lenna", "lenna_256x192_img"), ("hut", "hut_320x200_img")):
        img = z[key]
        h, w = img.shape
        out[name] = np.ascontiguousarray(img[:h & ~3, :w & ~3])
    return out


def run(img, c):
    return hr.detect(img, (c[9], c[10]), c[0], c[1], (c[2], c[3]), c[4], bool(c[5]), c[6] / 1000.0, c[7] / 100.0, c[8])


def make():
    out = {}
    for name, img in crops().items():
        for c in CONFIGS:
            pos, sc, lv, keep, _ = run(img, c)
            k = "%s__%s" % (name, "_".join(str(v) for v in c))
            out[k + "_pos"], out[k + "_score"], out[k + "_level"], out[k + "_keep"] = pos, sc, lv, keep
    return out


if __name__ == "__main__":
    arrays = make()
    np.savez_compressed(os.path.join(OUT, "harrisgrid.npz"), **arrays)
    print("wrote harrisgrid.npz:", len(arrays), "arrays")
