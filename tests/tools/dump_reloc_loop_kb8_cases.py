#!/usr/bin/env python3
"""Write the cases of tests/reloc_loop_kb8_cases.py with the restatement's results, one file per case, for
tests/tools/reloc_loop_kb8_host_check.cpp (a stand-alone run of the host twins vslamh_search_by_projection_keyframe_kb8 and
vslamh_search_by_projection_sim3_kb8 on the CPU, under sanitizers when built so).  The case whose job the device entry refuses is
written too: the twin takes any number of survivors.
  dump_reloc_loop_kb8_cases.py OUTDIR [case ..]"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kb8_ref as KR
import reloc_loop_kb8_cases as RC
from oracle import orbo

F32 = np.float32


def cam_floats(c):
    return np.array([c["fx"], c["fy"], c["cx"], c["cy"]] + list(c["k"]) + [c["precision"]], F32)


out = sys.argv[1]
os.makedirs(out, exist_ok=True)
g = RC.golden()
names = sys.argv[2:] or sorted(RC.a_cases()) + sorted(RC.b_cases())
for name in names:
    with open(os.path.join(out, name + ".bin"), "wb") as fh:
        if name in RC.a_cases():
            c = RC.a_cases()[name]
            nm, m, _ = RC.reference_a(name)
            n, n2 = len(c["kf_kps"]), len(c["cur_kps"])
            occ = c["occupied"]
            fh.write(np.array([0, n, n2, len(g["sf"]), int(c["gf"]), int(c["check_ori"]), c["orb_dist"], int(occ is not None)],
                              np.int32).tobytes())
            fh.write(np.array([c["th"], RC.LSF] + list(RC.BOUNDS), F32).tobytes())
            fh.write(cam_floats(KR.camera(*c["cam"])).tobytes())
            fh.write(np.asarray(g["sf"], F32).tobytes())
            fh.write(np.asarray(c["T"], F32).tobytes())
            fh.write(np.asarray(c["Ow"], F32).tobytes())
            fh.write(np.ascontiguousarray(c["kf_kps"], orbo.KP_DTYPE).tobytes())
            for k, t in (("flags", np.uint8), ("x3dw", F32), ("mn", F32), ("mx", F32), ("desc", np.uint8)):
                fh.write(np.ascontiguousarray(c[k], t).tobytes())
            fh.write(np.ascontiguousarray(c["cur_kps"], orbo.KP_DTYPE).tobytes())
            fh.write(np.ascontiguousarray(c["cur_desc"], np.uint8).tobytes())
            if occ is not None:
                fh.write(np.ascontiguousarray(occ, np.uint8).tobytes())
            fh.write(np.array([nm], np.int32).tobytes())
            fh.write(np.ascontiguousarray(m, np.int32).tobytes())
        else:
            c = RC.b_cases()[name]
            m, nm, ng, _ = RC.reference_b(name)
            n = len(c["pts"])
            fh.write(np.array([1, len(c["jobs"]), n, len(g["sf"]), int(c["gf"]), c["th"], 0, 0], np.int32).tobytes())
            fh.write(np.array([c["ratio"], RC.LSF] + list(RC.BOUNDS), F32).tobytes())
            fh.write(cam_floats(g["cams"][0]).tobytes())
            fh.write(np.asarray(g["sf"], F32).tobytes())
            fh.write(np.ascontiguousarray(c["pts"], orbo.FUSE_POINT_DTYPE).tobytes())
            fh.write(np.ascontiguousarray(c["desc"], np.uint8).tobytes())
            for k, j in enumerate(c["jobs"]):
                v, mt = j.get("valid"), j.get("matched")
                fh.write(np.array([len(j["kps"]), int(mt is not None), int(v is not None)], np.int32).tobytes())
                fh.write(np.concatenate([np.asarray(a, F32).reshape(-1) for a in j["pose"]]).tobytes())
                fh.write(np.ascontiguousarray(j["kps"], orbo.KP_DTYPE).tobytes())
                fh.write(np.ascontiguousarray(j["desc"], np.uint8).tobytes())
                if mt is not None:
                    fh.write(np.ascontiguousarray(mt, np.uint8).tobytes())
                if v is not None:
                    fh.write(np.ascontiguousarray(v, np.uint8).tobytes())
                fh.write(np.array([nm[k], ng[k]], np.int32).tobytes())
                fh.write(np.ascontiguousarray(m[k], np.int32).tobytes())
    print(name)
