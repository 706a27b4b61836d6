#!/usr/bin/env python3
"""Writes tests/golden/two_view_hut.npz: the inputs and the yardstick's outputs of the two-view consensus on real pixels.
hut_stereo 01 / 02 (tests/golden/real_images.npz) through the CPU oracle's extraction (5000 features, lapping area 0..1000)
and SearchForInitialization (window 100), hypotheses from tests/two_view_cases.svd_hypotheses (np.linalg.svd over seeded
8-point sets; stored, because another LAPACK build may round them differently), results from tests/two_view_ref.py.
Run from the repository root:  python tests/golden/make_two_view_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import orbo
import two_view_cases as TC
import two_view_ref as TR

z = np.load(os.path.join(HERE, "real_images.npz"))
e = orbo.Extractor(5000)
k1, d1, _ = e.compute(z["hut1"], lap=(0, 1000))
k2, d2, _ = e.compute(z["hut2"], lap=(0, 1000))
h, w = z["hut1"].shape
nm, m12, _ = orbo.search_for_initialization(k1, d1, k2, d2, w, h, window=100)
xy1 = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
xy2 = np.stack([k2["x"], k2["y"]], 1).astype(np.float32)
H21, H12, F21 = TC.svd_hypotheses(TR.gather(xy1, xy2, TR.pair_list(m12)), 200, TC.REAL_SEED)
r = TR.two_view_score(dict(xy1=xy1, xy2=xy2, matches12=m12, H21=H21, H12=H12, F21=F21, sigma=1.0))
assert r["rc"] == 0 and r["n_pairs"] == nm and min(r["inliers_h"].sum(), r["inliers_f"].sum()) >= 30
out = dict(xy1=xy1, xy2=xy2, matches12=m12.astype(np.int32), H21=H21, H12=H12, F21=F21, sigma=np.float32(1.0))
out.update({"want_" + k: np.asarray(v) for k, v in r.items() if k != "rc"})
path = os.path.join(HERE, "two_view_hut.npz")
np.savez_compressed(path, **out)
print("%s: %d bytes, %d pairs, best H %d (%d inliers), best F %d (%d inliers)"
      % (path, os.path.getsize(path), r["n_pairs"], r["best_h"], r["inliers_h"].sum(), r["best_f"], r["inliers_f"].sum()))
