#!/usr/bin/env python3
"""Generate tests/golden/lk_hut_long.npz: the 384x256 crops (rows 112:368, columns 184:568) of frames 01-05 of the
reference's smooth tracking sequence test/images/scenery/hut_long (752x480 colour PNGs; grey = OpenCV's 8-bit weights,
(4899 R + 9617 G + 1868 B + 8192) >> 14), and what tests/lk_ref.py computes for the cases of tests/lk_cases.py, as
uint32 / int32 arrays.  The outputs pin the restatement against regressions; they are not reference outputs (the
reference's tracker is CUDA).

    python tests/golden/make_lk_golden.py [directory of hut_long]     # the frames are re-read only if a directory is given
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(OUT, "lk_hut_long.npz")
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


def read_frames(directory):
    from PIL import Image
    out = []
    for i in range(1, 6):
        rgb = np.array(Image.open(os.path.join(directory, "%02d.png" % i)).convert("RGB")).astype(np.uint32)
        grey = (4899 * rgb[..., 0] + 9617 * rgb[..., 1] + 1868 * rgb[..., 2] + 8192) >> 14
        out.append(grey[112:368, 184:568].astype(np.uint8))
    return np.stack(out)


def make(frames):
    np.savez_compressed(PATH, frames=frames)  # lk_cases reads the frames from the file
    import lk_cases as LC
    LC.frames.cache_clear()
    out = dict(frames=frames)
    for name in LC.cases():
        T, last, _ = LC.run_ref(name)
        for k, v in last.items():
            out["%s__%s" % (name, k)] = v
        if name == "precompute":
            out["precompute__patches"], out["precompute__invh"] = LC.templates(T)
    return out


if __name__ == "__main__":
    frames = read_frames(sys.argv[1]) if len(sys.argv) > 1 else np.load(PATH)["frames"]
    np.savez_compressed(PATH, **make(frames))
    print("%s: %d bytes" % (PATH, os.path.getsize(PATH)))
