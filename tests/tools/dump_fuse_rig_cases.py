#!/usr/bin/env python3
"""Write the cases of tests/fuse_rig_cases.py with the restatement's results, one file per case, for
tests/tools/fuse_rig_host_check.cpp (a stand-alone run of the host twin vslamh_fuse_search_rig on the CPU, under sanitizers when
built so).  The cases the device entry refuses are written too: the twin takes any number of jobs and keypoints.
  dump_fuse_rig_cases.py OUTDIR [case ..]"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuse_rig_cases as FC
from oracle import orbo

F32 = np.float32


def cam_floats(c):
    return np.array([c["fx"], c["fy"], c["cx"], c["cy"]] + list(c["k"]) + [c["precision"]], F32)


out = sys.argv[1]
os.makedirs(out, exist_ok=True)
g = FC.golden()
for name in (sys.argv[2:] or sorted(FC.cases())):
    c = FC.cases()[name]
    bi, bd, _ = FC.reference(name)
    n = len(c["pts"])
    with open(os.path.join(out, name + ".bin"), "wb") as fh:
        fh.write(np.array([len(c["jobs"]), n, len(g["sf"]), int(c["gf"])], np.int32).tobytes())
        fh.write(np.array([c["th"], FC.LSF] + list(FC.BOUNDS), F32).tobytes())
        fh.write(cam_floats(g["cams"][0]).tobytes())
        fh.write(cam_floats(g["cams"][1]).tobytes())
        fh.write(np.asarray(g["rig"]["Tlr"], F32).tobytes())
        fh.write(np.asarray(g["rig"]["Trl"], F32).tobytes())
        fh.write(np.asarray(g["sf"], F32).tobytes())
        fh.write(np.asarray(g["is2"], F32).tobytes())
        fh.write(np.ascontiguousarray(c["pts"], orbo.FUSE_POINT_DTYPE).tobytes())
        fh.write(np.ascontiguousarray(c["desc"], np.uint8).tobytes())
        for j in c["jobs"]:
            v = j["valid"]
            fh.write(np.array([j["camera"], int(j["sim3"]), len(j["kps"]), j["idx_offset"], int(v is not None)], np.int32).tobytes())
            fh.write(np.concatenate([np.asarray(a, F32).reshape(-1) for a in j["pose"]]).tobytes())
            fh.write(np.ascontiguousarray(j["kps"], orbo.KP_DTYPE).tobytes())
            fh.write(np.ascontiguousarray(j["desc"], np.uint8).tobytes())
            if v is not None:
                fh.write(np.ascontiguousarray(v, np.uint8).tobytes())
        fh.write(np.ascontiguousarray(bi, np.int32).tobytes())
        fh.write(np.ascontiguousarray(bd, np.int32).tobytes())
    print(name)
