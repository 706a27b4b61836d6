#!/usr/bin/env python3
"""Write the cases of tests/bow_rig_cases.py (the single-keyframe cases, the overflow case and the batch's jobs) with the
restatement's results, one file per case, for tests/tools/bow_rig_host_check.cpp (a stand-alone run of the host twin on the
CPU, under sanitizers when built so).
  dump_bow_rig_cases.py OUTDIR"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bow_rig_cases as BC
from oracle import orbo

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
todo = dict(BC.cases())
todo["overflow_2049"] = BC.overflow()
jobs, f, ratio, ori = BC.batch()
for j, k in enumerate(jobs):
    todo["batch_job%d" % j] = dict(kf=k, f=f, ratio=ratio, ori=ori)
for name, c in todo.items():
    nm, m = BC.reference(c)
    k, fr = c["kf"], c["f"]
    with open(os.path.join(out, name + ".bin"), "wb") as fh:
        fh.write(np.array([len(k["kps"]), k["n_left"], len(k["fv"]["fv_nodes"]), len(k["fv"]["fv_feat"]), len(fr["kps"]),
                           fr["n_left"], len(fr["fv"]["fv_nodes"]), len(fr["fv"]["fv_feat"]), int(c["ori"])], np.int32).tobytes())
        fh.write(np.array([c["ratio"]], np.float32).tobytes())
        for side, flags in ((k, True), (fr, False)):
            fh.write(np.ascontiguousarray(side["kps"], orbo.KP_DTYPE).tobytes())
            fh.write(np.ascontiguousarray(side["desc"], np.uint8).tobytes())
            if flags:
                fh.write(np.ascontiguousarray(side["flags"], np.uint8).tobytes())
            for key in ("fv_nodes", "fv_off", "fv_feat"):
                fh.write(np.ascontiguousarray(side["fv"][key], np.int32).tobytes())
        fh.write(np.array([nm], np.int32).tobytes())
        fh.write(np.ascontiguousarray(m, np.int32).tobytes())
    print(name)
