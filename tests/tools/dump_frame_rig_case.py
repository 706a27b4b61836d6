#!/usr/bin/env python3
"""Write the cases of tests/frame_projection_rig_cases.py with the reference's results, one file per case, for
tests/tools/frame_rig_host_check.cpp (a stand-alone sanitizer run of the host twin on the CPU).
  dump_frame_rig_case.py OUTDIR"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_projection_rig_cases as FP
import kb8_cases as KC
import vi_slam_amd as V

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
sf = np.ascontiguousarray(FP.golden()["sf"], np.float32)
for name, c in FP.cases().items():
    nm, m, _ = FP.reference(c)
    P = V.proj_params(c["Tcw"], KC.LOCAL_CAM[:4], c["th"], FP.IMG, c["forward"], c["backward"], c["ori"], c["gf"])
    with open(os.path.join(out, name + ".bin"), "wb") as f:
        f.write(np.array([len(c["last_kps"]), len(c["kl"]), len(c["kr"]), c["occ"] is not None, len(sf)], np.int32).tobytes())
        f.write(bytes(P))
        f.write(bytes(V.kb8_camera(*KC.LOCAL_CAM)))
        f.write(np.ascontiguousarray(c["Trl"], np.float32).tobytes())
        f.write(np.array(FP.BOUNDS, np.float32).tobytes())
        f.write(sf.tobytes())
        for a, dt in ((c["last_kps"], V.KP_DTYPE), (c["flags"], np.uint8), (c["x3dw"], np.float32), (c["desc"], np.uint8),
                      (c["kl"], V.KP_DTYPE), (c["dl"], np.uint8), (c["kr"], V.KP_DTYPE), (c["dr"], np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        if c["occ"] is not None:
            f.write(np.ascontiguousarray(c["occ"], np.uint8).tobytes())
        f.write(np.array([nm], np.int32).tobytes())
        f.write(np.ascontiguousarray(m, np.int32).tobytes())
    print(name)
