#!/usr/bin/env python3
"""Frame::isInFrustum + SearchLocalPoints on the GPU box.  Checks parity with tests/frustum_ref.py first (records bit for
bit, matches against the oracle's matcher on the uncompacted records), then reports wall time per call of

  * k_frustum and k_frustum_compact alone by HIP events (vslam_fe_set_profiling brackets the two launches;
    vslam_fe_get_local_points_profile) for 4096 / 16384 / 65536 MapPoints in device memory, about 3 % of them in view,
  * the frustum stage as a call (vslam_frame_in_frustum: upload, k_frustum, records back) for the same sizes,
  * the whole vslam_search_local_points call for 16384 MapPoints of which about 2000 are in view, from host memory and
    from device memory,
  * the baseline: the existing vslam_search_by_projection_mappoints fed with the same surviving records computed
    beforehand (the caller's CPU isInFrustum is not counted).

Writes profiles/local_points_timing.txt (or the path given as the first argument).  Sets no gate."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frustum_cases as FC
import frustum_ref as FR
import vi_slam_amd as V

WARM, REPS = 3, 30
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "local_points_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


s = FC.hut_scene()
fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
k, d, _ = fe.compute_batch([s["C"]])[0]
kp, dp, _ = fe.slot_dev_ptrs(0)
n_cur = len(k)

# parity first
keep = np.zeros(3000, bool)
keep[np.random.default_rng(41).permutation(3000)[:700]] = True
P, pts, desc = FC.big_scene(3000, keep)
want = FR.search_local_points_ref(FR.params(**P), pts, desc, s["kC"], s["dC"], None, s["sf"], 3.0, 0.8, None)
got = fe.search_local_points(V.frustum_params(**P), pts, desc, kp, dp, n_cur, None, None, 3.0, 0.8, want_track=True)
assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:4] == want[2:4], "parity"
assert got[4].tobytes() == want[4].tobytes(), "records"
say("parity with tests/frustum_ref.py: ok (3000 MapPoints, %d in view, %d matches)" % (want[3], want[0]))

import torch

say("kernels alone by HIP events (us per launch, mean of %d) | vslam_frame_in_frustum as a call (wall ms: median, min)" % REPS)
for n in (4096, 16384, 65536):
    keep = np.random.default_rng(n).random(n) < 0.03
    P, pts, desc = FC.big_scene(n, keep)
    vp = V.frustum_params(**P)
    dp_ = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint8).copy()).cuda()
    dd_ = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
    torch.cuda.synchronize()
    call = lambda: fe.search_local_points(vp, dp_.data_ptr(), dd_.data_ptr(), kp, dp, n_cur, None, None, 3.0, 0.8, n_mp=n)
    for _ in range(WARM):
        call()
    fe.set_profiling(True)
    for _ in range(REPS):
        call()
    fr_ms, co_ms, passes = fe.get_local_points_profile()
    fe.set_profiling(False)
    assert passes == REPS
    med, mn = timed(lambda: fe.frame_in_frustum(vp, pts))
    say("  n = %5d (%4d in view): k_frustum %.1f  k_frustum_compact %.1f | %.3f %.3f"
        % (n, keep.sum(), fr_ms / passes * 1e3, co_ms / passes * 1e3, med, mn))

n = 16384
keep = np.zeros(n, bool)
keep[np.random.default_rng(42).permutation(n)[:2000]] = True
P, pts, desc = FC.big_scene(n, keep)
vp = V.frustum_params(**P)
say("whole call, %d MapPoints, %d in view, %d current keypoints (wall ms per call: median, min)" % (n, keep.sum(), n_cur))
med, mn = timed(lambda: fe.search_local_points(vp, pts, desc, kp, dp, n_cur, None, None, 3.0, 0.8))
say("  from host memory:   %.3f %.3f" % (med, mn))
dpts = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint8).copy()).cuda()
ddesc = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
torch.cuda.synchronize()
med, mn = timed(lambda: fe.search_local_points(vp, dpts.data_ptr(), ddesc.data_ptr(), kp, dp, n_cur, None, None, 3.0, 0.8,
                                               n_mp=n))
say("  from device memory: %.3f %.3f" % (med, mn))
track, depth, _, _, _ = FR.frame_in_frustum(FR.params(**P), pts, FR.bounds_of(FR.params(**P)), FC.NLEVELS)
sel = np.nonzero(track["flags"] & 1)[0]
m = V.FMatcher(fe, 0.8, True)
med, mn = timed(lambda: m.SearchByProjectionMapPoints(track[sel], desc[sel], kp, dp, n_cur, None, 3.0, None))
say("  baseline, vslam_search_by_projection_mappoints on the %d surviving records: %.3f %.3f" % (len(sel), med, mn))
fe.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
