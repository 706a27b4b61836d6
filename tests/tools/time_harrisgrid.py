#!/usr/bin/env python3
"""The grid Harris / Shi-Tomasi detector (vilib::HarrisGPU's job) on the GPU box: parity with tests/harris_ref.py first,
then a batch of 32 device-resident KITTI-size frames per call at 1 and 3 levels for both scores, with the grid FAST
detector on the same frames in the same run as the yardstick (the CUDA reference cannot run here).
Writes profiles/harrisgrid_timing.txt.      python tests/tools/time_harrisgrid.py [out.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import harris_ref as hr  # noqa: E402
from vi_slam_amd import synth  # noqa: E402
from vi_slam_amd.fastgrid import FASTGPU  # noqa: E402
from vi_slam_amd.harrisgrid import HarrisGPU  # noqa: E402

W, H, B, CALLS, ROUNDS = 1240, 376, 32, 1500, 3  # a window is 0.3-0.5 s
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "harrisgrid_timing.txt")

if torch.cuda.device_count() == 0:
    sys.exit("time_harrisgrid.py: no GPU; nothing is measured without one")
frames = [np.ascontiguousarray(synth.make_frame(1241, 376, step=s)[:, :W]) for s in range(B)]
dev = torch.zeros((B, H, 1280), dtype=torch.uint8, device="cuda")
for s in range(B):
    dev[s, :, :W] = torch.from_numpy(frames[s]).cuda()
torch.cuda.synchronize()
ptrs = [dev[s].data_ptr() for s in range(B)]


def timed(dets):
    """ms per call of each detector: best of ROUNDS windows of CALLS calls, the detectors taking turns window by window;
    every call ends in the detector's own stream synchronise."""
    best = {name: float("inf") for name in dets}
    for det in dets.values():
        for _ in range(3):
            det.detect_batch(dev_ptrs=ptrs, pitch=1280)
    for _ in range(ROUNDS):
        for name, det in dets.items():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                det.detect_batch(dev_ptrs=ptrs, pitch=1280)
            best[name] = min(best[name], (time.perf_counter() - t0) / CALLS * 1e3)
    return best


rows = []
for levels in (1, 3):
    px = sum((W >> l) * (H >> l) for l in range(levels))  # bytes the algorithm must read per frame: every level once
    dets = {"fast": FASTGPU(W, H, max_level=levels, max_batch=B),
            "harris": HarrisGPU(W, H, max_level=levels, use_harris=True, max_batch=B),
            "shi_tomasi": HarrisGPU(W, H, max_level=levels, use_harris=False, max_batch=B)}
    try:
        for name in ("harris", "shi_tomasi"):  # parity before any timing
            got = dets[name].detect_batch(dev_ptrs=ptrs[:2], pitch=1280)
            t0 = time.perf_counter()
            want = hr.detect(frames[0], (32, 32), 0, levels, (0, 0), hr.BORDER_SKIP, name == "harris", 0.04, 0.1, 0)
            t_ref = time.perf_counter() - t0
            same = all(np.array_equal(np.asarray(g[0]).view(np.uint8), np.asarray(w_).view(np.uint8))
                       for g, w_ in zip(got[:4], want[:4])) and int(got[4][0]) == want[4]
            if not same:
                sys.exit("time_harrisgrid.py: %s, %d level(s): the device grid differs from tests/harris_ref.py" % (name, levels))
            rows.append({"detector": name + "_restatement_1core", "levels": levels, "ms_per_frame": round(t_ref * 1e3, 2)})
        ms = timed(dets)
        for name, t in ms.items():
            rows.append({"detector": name, "levels": levels, "frames_per_call": B, "ms_per_call": round(t, 4),
                         "frames_per_s": round(B / t * 1e3, 1), "algorithmic_GBps": round(px * B / t / 1e6, 2),
                         "ms_over_fast": round(t / ms["fast"], 3), "equal_to_restatement": name != "fast" or None})
    finally:
        for d in dets.values():
            d.close()

with open(OUT, "w") as f:
    f.write("# tests/tools/time_harrisgrid.py, 1 x MI355X: %d device-resident %dx%d frames per call, host clock around calls that\n"
            "# end in a stream synchronise, best of %d windows of %d calls; algorithmic GB/s = level bytes read once / time\n"
            % (B, W, H, ROUNDS, CALLS))
    for r in rows:
        f.write(json.dumps(r) + "\n")
for r in rows:
    print(json.dumps(r))
