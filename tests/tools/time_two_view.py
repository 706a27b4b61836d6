#!/usr/bin/env python3
"""The two-view consensus (vslam_two_view_score) on the GPU box.  Checks parity with tests/two_view_ref.py first (every
result as uint32 words, on the planar and the general case and on each timed shape), then reports, for N = 100 / 300 / 1000 /
4000 pairs x (200 + 200) hypotheses x 1 and 32 jobs with the keypoints and matches in HBM,

  * k_tv_pairs, k_tv_score and k_tv_select alone by HIP events (vslam_fe_set_profiling brackets the three launches;
    vslam_fe_get_two_view_profile),
  * the whole call, vslam_two_view_score_async + _wait, as wall time (the C entry points over prebuilt job tables: the
    Python mirror's own packing is not counted),
  * the yardstick of the same run: vslamh_two_view_score, the same arithmetic on ONE host core, per job (the reference runs
    the two models on two threads).

Writes profiles/two_view_timing.txt (or the path given as the first argument).  Sets no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import two_view_cases as TC
import two_view_ref as TR
import vi_slam_amd as V

WARM, REPS = 3, 30
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "two_view_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=REPS):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


import torch

fe = V.FExtractor(1000, 1.2, 8, 20, 7, 640, 480, max_batch=1)
L, HL = V.lib(), V.host_lib()
HL.vslamh_two_view_score.argtypes = [C.POINTER(V._TwoViewJob), C.POINTER(V._TwoViewResult)]

for c in (TC.planar_case(), TC.general_case()):
    TC.assert_equal_words(fe.two_view_score([TC.job_of(c)])[0], TR.two_view_score(c), c["name"])
say("parity with tests/two_view_ref.py: ok (planar and general case, 300 pairs, 200 + 200 hypotheses)")
say("us per launch by HIP events (mean of %d) | whole call, wall ms (median, min) | host twin on one core, ms per job (median)"
    % REPS)
keep = []
for n in (100, 300, 1000, 4000):
    case = TC.make("timing", n, 200, 200, planar=False, seed=100 + n, n_unmatched1=n // 3, n_extra2=n // 5, f_spread=3.0)
    want = TR.two_view_score(case)
    host = TC.job_of(case)
    dev = []
    for a in (host["kps1"], host["kps2"], host["matches12"]):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        keep.append(t)
        dev.append(t.data_ptr())
    torch.cuda.synchronize()
    job = dict(host, kps1=dev[0], kps2=dev[1], n1=len(host["kps1"]), n2=len(host["kps2"]), matches12=dev[2])
    hcall = V._TwoViewCall([host])
    host_ms, _ = timed(lambda: HL.vslamh_two_view_score(hcall.jobs, hcall.res), reps=5)
    TC.assert_equal_words(hcall.results()[0], want, "host twin")
    for njobs in (1, 32):
        call = V._TwoViewCall([job] * njobs)

        def run():
            assert L.vslam_two_view_score_async(fe._h, call.n, call.jobs) == 0
            assert L.vslam_two_view_score_wait(fe._h, call.res) == 0
        run()
        for r in call.results():
            TC.assert_equal_words(r, want, "N=%d x %d jobs" % (n, njobs))
        for _ in range(WARM):
            run()
        before = fe.get_two_view_profile()
        fe.set_profiling(True)
        for _ in range(REPS):
            run()
        after = fe.get_two_view_profile()
        fe.set_profiling(False)
        assert after[3] - before[3] == REPS
        us = [(a - b) / REPS * 1e3 for a, b in zip(after[:3], before[:3])]
        med, mn = timed(run)
        say("  N = %4d x %2d jobs: k_tv_pairs %6.1f  k_tv_score %7.1f  k_tv_select %5.1f | %.3f %.3f | %.3f (x %d = %.1f)"
            % (n, njobs, us[0], us[1], us[2], med, mn, host_ms, njobs, host_ms * njobs))
fe.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
