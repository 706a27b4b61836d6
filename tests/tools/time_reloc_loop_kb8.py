#!/usr/bin/env python3
"""The relocalisation and the loop-closing SearchByProjection for fisheye cameras (vslam_search_by_projection_keyframe_kb8,
vslam_search_by_projection_sim3_kb8) on the GPU box.  Parity first: every served case of tests/reloc_loop_kb8_cases.py against
the numpy restatement, and every synthetic scene below against the host twin (which the CPU suite pins to the restatement).
Then, for a frame / KeyFrames of 1250 keypoints (640 x 480), 5 rounds of 30 calls each, arguments prepared once:

  (a) A, and a blocking 1-job B over 1500 MapPoints, against the pinhole vslam_search_by_projection_keyframe / _sim3 of the same
      build on the same arrays (their own context without a KB8 camera; the projections differ, the counts do not).
      Expectation to confirm or refute: the pinhole call plus one KB8 projection per point (B also pays the gate pass and the
      compaction, two launches more).
  (b) B with 5 and 16 jobs in one call, against as many blocking 1-job calls in sequence.
  (c) B over a 6000-point list, one job, against the host twin on one thread.
  (d) the split of vslam_fe_get_sim3_kb8_profile (HIP events): gate + compaction | ranking | resolution.

Wall ms per call: mean of the rounds [least .. greatest].  Writes profiles/reloc_loop_kb8_timing.txt (or the path given as the
first argument).  Sets no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frustum_cases as HC
import kb8_cases as KC
import kb8_ref as KR
import reloc_loop_kb8_cases as RC
import vi_slam_amd as V

import torch

WARM, ROUNDS, CALLS = 3, 5, 30
W, H, TH, NK = 640, 480, 3, 1250
CAM = (236.0, 237.0, 319.5, 240.25, KC.K_TUM, 0.0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reloc_loop_kb8_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, calls=CALLS):
    for _ in range(WARM):
        fn()
    r = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        r.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.mean(r)), "%.3f [%.3f .. %.3f]" % (float(np.mean(r)), min(r), max(r))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- parity on the suite's cases
g = RC.golden()
fe0 = V.FExtractor(HC.HUT_NF, 1.2, 8, 20, 7, HC.HUT_W, HC.HUT_H, max_batch=1)
keep, served = [], 0
for name, c in sorted(RC.a_cases().items()):
    fe0.set_kb8_camera(V.kb8_camera(*c["cam"]))
    t = (dev(np.ascontiguousarray(c["cur_kps"], V.KP_DTYPE)), dev(c["cur_desc"]))
    torch.cuda.synchronize()
    nm, m = V.FMatcher(fe0, checkOri=c["check_ori"]).SearchByProjectionKeyFrameKB8(
        c["T"], c["Ow"], c["cam"][:4], c["th"], c["orb_dist"], RC.LSF, c["kf_kps"], c["flags"], c["x3dw"], c["mn"], c["mx"], c["desc"],
        t[0].data_ptr(), t[1].data_ptr(), len(c["cur_kps"]), c["occupied"], RC.IMG, c["gf"])
    want = RC.reference_a(name)
    assert nm == want[0] and np.array_equal(m, want[1]), ("parity", name)
    served += 1
fe0.set_kb8_camera(V.kb8_camera(*RC.CAM1))
for name, c in sorted(RC.b_cases().items()):
    if c["refuse"] is not None:
        continue
    jobs = []
    for j in c["jobs"]:
        n = len(j["kps"])
        t = (dev(np.ascontiguousarray(j["kps"], V.KP_DTYPE)), dev(j["desc"])) if n else (None, None)
        keep.append(t)
        jobs.append(V.sim3_kb8_job(*j["pose"], t[0].data_ptr() if n else 0, t[1].data_ptr() if n else 0, n, j.get("matched"),
                                   j.get("valid")))
    torch.cuda.synchronize()
    m, nm, ng = fe0.search_by_projection_sim3_kb8(jobs, c["pts"], c["desc"], c["th"], c["ratio"], RC.LSF, RC.IMG, c["gf"])
    want = RC.reference_b(name)
    assert np.array_equal(nm, want[1]) and np.array_equal(ng, want[2]) and all(np.array_equal(a, b) for a, b in zip(m, want[0])), \
        ("parity", name)
    served += 1
fe0.close()
keep.clear()
say("parity with tests/reloc_loop_kb8_ref.py on %d cases: ok" % served)

# ---- synthetic scenes
fe = V.FExtractor(1000, 1.2, 8, 20, 7, W, H, max_batch=1)
fe.set_kb8_camera(V.kb8_camera(*CAM))
fe_pin = V.FExtractor(1000, 1.2, 8, 20, 7, W, H, max_batch=1)
sf = fe.GetScaleFactors()
cam = KR.camera(*CAM)
L = V.lib()
rng = np.random.default_rng(NK)
kps = np.zeros(NK, V.KP_DTYPE)
kps["x"], kps["y"] = rng.uniform(19, W - 19, NK).astype(np.float32), rng.uniform(19, H - 19, NK).astype(np.float32)
kps["octave"] = np.minimum(rng.geometric(0.35, NK) - 1, 7)
kps["angle"] = rng.uniform(0, 360, NK).astype(np.float32)
kps["size"] = 31.0
desc = rng.integers(0, 256, (NK, 32)).astype(np.uint8)
t_k, t_d = dev(kps), dev(desc)
rays = KR.unproject(cam, np.stack([kps["x"], kps["y"]], 1))[0].astype(np.float64)
poses = []
for k in range(16):
    T, Ow = HC.pose(HC.rotation(0.002 * k, -0.003 * k, 0.001 * k), (0.01 * k, -0.005 * k, 0.012 * k))
    poses.append((np.ascontiguousarray(T[:, :3]), np.ascontiguousarray(T[:, 3]), Ow, T))


def points_on(m, bad):
    """m MapPoints on the rays of random keypoints as pose 0 sees them, a few descriptor bits off, a quarter of them scattered
    around the camera; the fraction `bad` of them isBad() (at 6000 points 0.4, so that no job keeps more than 4096 behind its
    gates: the wide camera sees most of the scattered ones too)"""
    R, t, Ow = (np.asarray(a, np.float64) for a in poses[0][:3])
    sel = rng.integers(0, NK, m)
    xc = rays[sel] * rng.uniform(2.0, 6.0, m)[:, None]
    junk = rng.random(m) < 0.25
    xc[junk] = np.stack([rng.uniform(-6, 6, junk.sum()), rng.uniform(-6, 6, junk.sum()), rng.uniform(-1, 6, junk.sum())], 1)
    pw = (xc - t) @ R
    po = pw - Ow
    d = np.linalg.norm(po, axis=1)
    p = np.zeros(m, V.FUSE_POINT_DTYPE)
    p["pos"], p["normal"] = pw.astype(np.float32), (po / d[:, None]).astype(np.float32)
    p["min_distance"] = (0.6 * d).astype(np.float32)
    p["max_distance"] = (d * 1.2 ** (kps["octave"][sel] + 0.5)).astype(np.float32)
    p["valid"] = rng.random(m) > bad
    dd = desc[sel].copy()
    dd[np.arange(m), sel % 32] ^= np.uint8(5)
    dd[junk] = rng.integers(0, 256, (int(junk.sum()), 32))
    return p, dd, sel


def job(k, host=False):
    kp, dp = (kps.ctypes.data, desc.ctypes.data) if host else (t_k.data_ptr(), t_d.data_ptr())
    return V.sim3_kb8_job(*poses[k][:3], kp, dp, NK)


def outputs(K):
    ms = [np.zeros(NK, np.int32) for _ in range(K)]
    return ms, (C.c_void_p * K)(*[a.ctypes.data for a in ms]), np.zeros(K, np.int32), np.zeros(K, np.int32)


torch.cuda.synchronize()
for m, bad in ((1500, 0.05), (6000, 0.4)):
    pts, dd, sel = points_on(m, bad)
    got = fe.search_by_projection_sim3_kb8([job(k) for k in range(16)], pts, dd, TH, 1.0, RC.LSF, (W, H))
    want = V.search_by_projection_sim3_kb8_host(V.kb8_camera(*CAM), [job(k, True) for k in range(16)], pts, dd, TH, 1.0, RC.LSF,
                                                (W, H), sf)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and \
        all(np.array_equal(a, b) for a, b in zip(got[0], want[0])), ("parity", m)
    say("%d keypoints, %d MapPoints, 16 jobs: parity with the host twin ok; survivors per job %s, matches %s"
        % (NK, m, got[2].tolist()[:4], got[1].tolist()[:4]))
    ms = {}
    for K in (1, 5, 16):
        head, hold = fe._sim3_kb8_call([job(k) for k in range(K)], pts, dd, TH, 1.0, RC.LSF, (W, H), False, None)
        o = outputs(K)

        def call():
            assert L.vslam_search_by_projection_sim3_kb8(*head, o[1], o[2].ctypes.data_as(C.c_void_p),
                                                         o[3].ctypes.data_as(C.c_void_p)) == V.VSLAM_OK

        ms[K], txt = timed(call)
        fe.set_profiling(True)
        for _ in range(CALLS):
            call()
        a, b, c, passes = fe.get_sim3_kb8_profile()
        fe.set_profiling(False)
        assert passes == CALLS
        say("  B, %2d job(s) in one call, wall ms: %s   (d) by HIP events, us: gate + compaction %.1f | ranking %.1f | resolution %.1f"
            % (K, txt, a / CALLS * 1e3, b / CALLS * 1e3, c / CALLS * 1e3))
    singles = [fe._sim3_kb8_call([job(k)], pts, dd, TH, 1.0, RC.LSF, (W, H), False, None) for k in range(16)]
    o1 = outputs(1)
    for K in (5, 16):
        def seq():
            for s in singles[:K]:
                assert L.vslam_search_by_projection_sim3_kb8(*s[0], o1[1], o1[2].ctypes.data_as(C.c_void_p),
                                                             o1[3].ctypes.data_as(C.c_void_p)) == V.VSLAM_OK

        s_ms, txt = timed(seq)
        say("  (b) %2d blocking 1-job calls in sequence, wall ms: %s   -> one %d-job call / sequence = %.2f" % (K, txt, K, ms[K] / s_ms))
    if m == 1500:
        # (a) the pinhole entries of the same build on the same arrays, through the Python mirror both
        R0, t0, O0, T0 = poses[0]
        mk, mp = V.FMatcher(fe), V.FMatcher(fe_pin)
        fl = pts["valid"].astype(np.uint8)
        a_args = (T0, O0, CAM[:4], 3.0, 100, RC.LSF, kps[sel], fl, pts["pos"], pts["min_distance"], pts["max_distance"], dd,
                  t_k.data_ptr(), t_d.data_ptr(), NK, None, (W, H))
        got_a = mk.SearchByProjectionKeyFrameKB8(*a_args)
        want_a = V.search_by_projection_keyframe_kb8_host(V.kb8_camera(*CAM), T0, O0, 3.0, 100, RC.LSF, kps[sel], fl, pts["pos"],
                                                          pts["min_distance"], pts["max_distance"], dd, kps, desc, (W, H), sf)
        assert got_a[0] == want_a[0] and np.array_equal(got_a[1], want_a[1]), "parity of A"
        _, txt_k = timed(lambda: mk.SearchByProjectionKeyFrameKB8(*a_args))
        _, txt_p = timed(lambda: mp.SearchByProjectionKeyFrame(*a_args))
        say("  (a) A, %d KeyFrame entries, %d matches: pinhole vslam_search_by_projection_keyframe %s | _keyframe_kb8 %s"
            % (m, got_a[0], txt_p, txt_k))
        _, txt_p = timed(lambda: mp.SearchByProjectionSim3(T0, O0, CAM[:4], TH, 1.0, RC.LSF, fl, pts["pos"], pts["normal"],
                                                           pts["min_distance"], pts["max_distance"], dd, t_k.data_ptr(),
                                                           t_d.data_ptr(), NK, None, (W, H)))
        _, txt_k = timed(lambda: fe.search_by_projection_sim3_kb8([job(0)], pts, dd, TH, 1.0, RC.LSF, (W, H)))
        say("  (a) B, 1 job: pinhole vslam_search_by_projection_sim3 %s | _sim3_kb8 %s" % (txt_p, txt_k))
    else:
        hj = [job(0, True)]
        _, txt = timed(lambda: V.search_by_projection_sim3_kb8_host(V.kb8_camera(*CAM), hj, pts, dd, TH, 1.0, RC.LSF, (W, H), sf),
                       calls=5)
        say("  (c) host twin on one thread, one job, %d points, wall ms: %s" % (m, txt))
fe.close()
fe_pin.close()
say("expectations (not thresholds): (a) the pinhole call plus one KB8 projection per point; (b) a K-job call saves K - 1 "
    "stagings, copies and waits against K blocking 1-job calls")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
