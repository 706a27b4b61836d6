#!/usr/bin/env python3
"""Write the cases of tests/local_points_rig_cases.py with the reference's results, one file per case, for
tests/tools/local_points_rig_host_check.cpp (a stand-alone sanitizer run of the host twin on the CPU).
  dump_local_points_rig_case.py OUTDIR"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_points_rig_cases as LC
import local_points_rig_ref as RR
import vi_slam_amd as V

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
sf = np.ascontiguousarray(LC.golden()["sf"], np.float32)
for name, c in LC.cases().items():
    nm, m, _ = RR.search_by_projection_rig(c["tl"], c["tr"], c["desc"], c["kl"], c["dl"], c["kr"], c["dr"], c["l2r"], c["r2l"], sf,
                                           LC.BOUNDS, c["th"], c["nnratio"], c["occ"])
    with open(os.path.join(out, name + ".bin"), "wb") as f:
        f.write(np.array([len(c["tl"]), len(c["kl"]), len(c["kr"]), c["occ"] is not None, len(sf)], np.int32).tobytes())
        f.write(np.array([c["th"], c["nnratio"]] + list(LC.BOUNDS), np.float32).tobytes())
        f.write(sf.tobytes())
        for a, dt in ((c["tl"], V.MP_TRACK_DTYPE), (c["tr"], V.MP_TRACK_DTYPE), (c["desc"], np.uint8), (c["kl"], V.KP_DTYPE),
                      (c["dl"], np.uint8), (c["kr"], V.KP_DTYPE), (c["dr"], np.uint8), (c["l2r"], np.int32),
                      (c["r2l"], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        if c["occ"] is not None:
            f.write(np.ascontiguousarray(c["occ"], np.uint8).tobytes())
        f.write(np.array([nm], np.int32).tobytes())
        f.write(np.ascontiguousarray(m, np.int32).tobytes())
    print(name)
