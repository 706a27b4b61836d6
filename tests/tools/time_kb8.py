#!/usr/bin/env python3
"""The fisheye camera on the GPU box.  Checks parity with tests/kb8_ref.py first (project, unproject, the frustum records,
the chain's matches), then reports

  * k_frustum with a KB8 camera against the pinhole k_frustum of the same build on the same 4096 / 16384 / 65536 MapPoints in
    device memory (same fx, fy, cx, cy), by HIP events (vslam_fe_get_local_points_profile): ROUNDS means of REPS launches
    each; the spread of the pinhole rounds is the run-to-run spread a comparison with another build has to respect,
  * vslam_kb8_project / vslam_kb8_unproject as calls for 4096 and 65536 points (wall ms: median, min),
  * the whole vslam_search_local_points call with a KB8 camera for 16384 MapPoints from host and from device memory.

Writes profiles/kb8_timing.txt (or the path given as the first argument).  Sets no gate."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frustum_cases as FC
import frustum_ref as FR
import kb8_cases as KC
import kb8_ref as KR
import vi_slam_amd as V
from oracle import orbo

WARM, REPS, ROUNDS = 3, 30, 5
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kb8_timing.txt")
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


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


s = KC.local_scene()
fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
k, d, _ = fe.compute_batch([s["C"]])[0]
kp, dp, _ = fe.slot_dev_ptrs(0)
n_cur = len(k)
import torch

# parity first
P = s["P"]
vp = V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                      (P["img_w"], P["img_h"]), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])
fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
xyz, px = KC.project_points(), KC.unproject_pixels("tum")
assert same(fe.kb8_project(xyz), KR.project(s["cam"], xyz)) and same(fe.kb8_unproject(px), KR.unproject(s["cam"], px)[0]), "camera"
track, depth, ntm, _, _ = KR.frame_in_frustum(P, s["cam"], s["pts"], FR.bounds_of(P), FC.NLEVELS)
nm, m = orbo.search_by_projection_mappoints(FR.far_filtered(P, track, depth), s["desc"], s["kC"], s["dC"],
                                            np.full(n_cur, -1, np.float32), s["sf"], P["img_w"], P["img_h"], 3.0, 0.8, None)
got = fe.search_local_points(vp, s["pts"], s["desc"], kp, dp, n_cur, None, None, 3.0, 0.8, want_track=True)
assert got[0] == nm and np.array_equal(got[1], m) and got[2] == ntm and got[4].tobytes() == track.tobytes(), "chain"
say("parity with tests/kb8_ref.py: ok (%d points projected, %d pixels unprojected, %d MapPoints, %d in view, %d matches)"
    % (len(xyz), len(px), len(s["pts"]), ntm, nm))

hut = FC.hut_scene()
kb8 = V.kb8_camera(*hut["cam"][:4], KC.K_TUM)  # the pinhole scene's own intrinsics: the same points serve both kernels
say("k_frustum by HIP events, us per launch: mean of %d rounds of %d launches [min .. max of the rounds]" % (ROUNDS, REPS))
for n in (4096, 16384, 65536):
    keep = np.random.default_rng(n).random(n) < 0.03
    Pb, pts, desc = FC.big_scene(n, keep)
    vb = V.frustum_params(**Pb)
    dp_ = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint8).copy()).cuda()
    dd_ = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
    torch.cuda.synchronize()
    call = lambda: fe.search_local_points(vb, dp_.data_ptr(), dd_.data_ptr(), kp, dp, n_cur, None, None, 3.0, 0.8, n_mp=n)
    res = {}
    for cam in ("pinhole", "kb8", "pinhole ", "kb8 "):  # interleaved: both cameras see the same drift of the machine
        fe.set_kb8_camera(kb8 if cam.strip() == "kb8" else None)
        for _ in range(WARM):
            call()
        for _ in range(ROUNDS):
            fe.set_profiling(True)
            a0 = fe.get_local_points_profile()
            for _ in range(REPS):
                call()
            a1 = fe.get_local_points_profile()
            fe.set_profiling(False)
            assert a1[2] - a0[2] == REPS
            res.setdefault(cam.strip(), []).append((a1[0] - a0[0]) / REPS * 1e3)
    for cam in ("pinhole", "kb8"):
        r = res[cam]
        say("  n = %5d  %-7s k_frustum %.1f [%.1f .. %.1f]" % (n, cam, np.mean(r), min(r), max(r)))
fe.set_kb8_camera(kb8)
say("vslam_kb8_project / vslam_kb8_unproject as calls (wall ms per call: median, min)")
rng = np.random.default_rng(7)
for n in (4096, 65536):
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0.2, 4, n)], 1).astype(np.float32)
    px = np.stack([rng.uniform(0, FC.HUT_W, n), rng.uniform(0, FC.HUT_H, n)], 1).astype(np.float32)
    a, b = timed(lambda: fe.kb8_project(xyz)), timed(lambda: fe.kb8_unproject(px))
    say("  n = %5d  project %.3f %.3f  unproject %.3f %.3f" % (n, a[0], a[1], b[0], b[1]))
n = 16384
keep = np.zeros(n, bool)
keep[np.random.default_rng(42).permutation(n)[:2000]] = True
Pb, pts, desc = FC.big_scene(n, keep)
vb = V.frustum_params(**Pb)
say("whole vslam_search_local_points call with a KB8 camera, %d MapPoints, %d current keypoints (wall ms: median, min)"
    % (n, n_cur))
med, mn = timed(lambda: fe.search_local_points(vb, pts, desc, kp, dp, n_cur, None, None, 3.0, 0.8))
say("  from host memory:   %.3f %.3f" % (med, mn))
dpts = torch.from_numpy(np.ascontiguousarray(pts).view(np.uint8).copy()).cuda()
ddesc = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
torch.cuda.synchronize()
med, mn = timed(lambda: fe.search_local_points(vb, dpts.data_ptr(), ddesc.data_ptr(), kp, dp, n_cur, None, None, 3.0, 0.8,
                                               n_mp=n))
say("  from device memory: %.3f %.3f" % (med, mn))
fe.set_kb8_camera(None)
fe.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
