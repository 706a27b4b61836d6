#!/usr/bin/env python3
"""The search half of Fuse for a two-fisheye rig (vslam_fuse_search_rig, k_fuse_rank_rig) on the GPU box.  Parity first: every
case of tests/fuse_rig_cases.py against the numpy restatement, and every synthetic scene below against the host twin (which the
CPU suite pins to the restatement).  Then, for KeyFrames of 2 x 600, 2 x 1250 and 2 x 2000 keypoints (640 x 480) and about 1500
and 6000 candidate MapPoints, 5 rounds of 30 calls each, arguments prepared once:

  (a) the blocking 1-job call, against the pinhole vslam_fuse_search of the same build on the same counts (its own context
      without a KB8 camera; MapPoints on the pinhole rays of the same keypoints).  Expectation to confirm or refute: the pinhole
      call plus the KB8 projection's extra per point.
  (b) the blocking 2-job and 16-job calls, against 2 and 16 blocking 1-job calls in sequence.  Expectation: the saving of K - 1
      stagings, copies and waits.
  (c) the host twin on one thread, one job.
  (d) k_fuse_rank_rig alone by HIP events (vslam_fe_get_fuse_rig_profile), for 1, 2 and 16 jobs.

Wall ms per call: mean of the rounds [least .. greatest].  Writes profiles/fuse_rig_timing.txt (or the path given as the first
argument).  Sets no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frustum_cases as HC
import fuse_rig_cases as FC
import kb8_cases as KC
import kb8_ref as KR
import vi_slam_amd as V

import torch

WARM, ROUNDS, CALLS = 3, 5, 30
W, H, TH = 640, 480, 3.0
CAM1 = (236.0, 237.0, 319.5, 240.25, KC.K_TUM, 0.0)
CAM2 = (243.0, 241.5, 322.25, 237.5, KC.K_STRONG, 0.0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fuse_rig_timing.txt")
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
g = FC.golden()
fe0 = V.FExtractor(HC.HUT_NF, 1.2, 8, 20, 7, HC.HUT_W, HC.HUT_H, max_batch=1)
fe0.set_kb8_camera(V.kb8_camera(*FC.CAM1))
rig0 = V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"])
keep = []
served = 0
for name, c in sorted(FC.cases().items()):
    if c["refuse"]:
        continue
    jobs = []
    for j in c["jobs"]:
        n = len(j["kps"])
        t = (dev(np.ascontiguousarray(j["kps"], V.KP_DTYPE)), dev(j["desc"])) if n else (None, None)
        keep.append(t)
        jobs.append(V.fuse_rig_job(*j["pose"], t[0].data_ptr() if n else 0, t[1].data_ptr() if n else 0, n, j["camera"],
                                   j["idx_offset"], j["valid"], j["sim3"]))
    torch.cuda.synchronize()
    bi, bd = fe0.fuse_search_rig(rig0, jobs, c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG, c["gf"])
    want = FC.reference(name)
    assert np.array_equal(bi, want[0]) and np.array_equal(bd, want[1]), ("parity", name)
    served += 1
fe0.close()
keep.clear()
say("parity with tests/fuse_rig_ref.py on %d cases: ok" % served)

# ---- synthetic scenes
fe = V.FExtractor(1000, 1.2, 8, 20, 7, W, H, max_batch=1)
fe.set_kb8_camera(V.kb8_camera(*CAM1))
fe_pin = V.FExtractor(1000, 1.2, 8, 20, 7, W, H, max_batch=1)
sf, is2 = fe.GetScaleFactors(), np.asarray(fe.GetInverseScaleSigmaSquares(), np.float32)
cams = (KR.camera(*CAM1), KR.camera(*CAM2))
rig_np = KC.rig()
rig = V.kb8_rig(V.kb8_camera(*CAM2), rig_np["Tlr"], rig_np["Trl"])
L = V.lib()


def keypoints(rng, n):
    k = np.zeros(n, V.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(19, W - 19, n).astype(np.float32), rng.uniform(19, H - 19, n).astype(np.float32)
    k["octave"] = np.minimum(rng.geometric(0.35, n) - 1, 7)
    k["size"] = 31.0
    return k, rng.integers(0, 256, (n, 32)).astype(np.uint8)


def pose_pair(T):
    Trl = np.asarray(rig_np["Trl"], np.float64)
    T = np.asarray(T, np.float64)
    Tr = np.hstack([Trl[:, :3] @ T[:, :3], (Trl[:, :3] @ T[:, 3] + Trl[:, 3]).reshape(3, 1)])
    out = []
    for M in (T, Tr):
        M32, Ow = HC.pose(M[:, :3], M[:, 3])
        out.append((np.ascontiguousarray(M32[:, :3]), np.ascontiguousarray(M32[:, 3]), Ow))
    return out


def points_on(rng, pose, rays, kps, desc, m):
    """m MapPoints on the rays of random keypoints of one camera, a few descriptor bits off; a quarter of them scattered"""
    R, t, Ow = (np.asarray(a, np.float64) for a in pose)
    sel = rng.integers(0, len(kps), m)
    xc = rays[sel] * rng.uniform(2.0, 6.0, m)[:, None]
    junk = rng.random(m) < 0.25
    xc[junk] = np.stack([rng.uniform(-6, 6, junk.sum()), rng.uniform(-6, 6, junk.sum()), rng.uniform(-1, 6, junk.sum())], 1)
    pw = (xc - t) @ R
    po = pw - Ow
    d = np.linalg.norm(po, axis=1)
    p = np.zeros(m, V.FUSE_POINT_DTYPE)
    p["pos"], p["normal"] = pw.astype(np.float32), (po / d[:, None]).astype(np.float32)
    p["min_distance"] = (0.6 * d).astype(np.float32)
    p["max_distance"] = (d * 1.2 ** (kps["octave"][sel] - 0.5).clip(0)).astype(np.float32)
    p["valid"] = rng.random(m) > 0.05
    dd = desc[sel].copy()
    dd[np.arange(m), sel % 32] ^= np.uint8(5)
    dd[junk] = rng.integers(0, 256, (int(junk.sum()), 32))
    return p, dd


for n in (600, 1250, 2000):
    rng = np.random.default_rng(n)
    (kl, dl), (kr, dr) = keypoints(rng, n), keypoints(rng, n)
    t = [dev(kl), dev(dl), dev(kr), dev(dr)]
    rays = [KR.unproject(cams[c], np.stack([k["x"], k["y"]], 1))[0].astype(np.float64) for c, k in ((0, kl), (1, kr))]
    pin_rays = np.stack([(kl["x"] - CAM1[2]) / CAM1[0], (kl["y"] - CAM1[3]) / CAM1[1], np.ones(n)], 1).astype(np.float64)
    poses = [pose_pair(HC.pose(HC.rotation(0.002 * k, -0.003 * k, 0.001 * k), (0.01 * k, -0.005 * k, 0.012 * k))[0]) for k in range(8)]
    for m in (1500, 6000):
        half = m // 2
        pa, da = points_on(rng, poses[0][0], rays[0], kl, dl, half)
        pb, db = points_on(rng, poses[0][1], rays[1], kr, dr, m - half)
        pts, desc = np.concatenate([pa, pb]), np.concatenate([da, db])
        valid = (rng.random(m) > 0.1).astype(np.uint8)

        def job(k, host=False):
            pose = poses[k // 2][k % 2]
            a = (kl, dl, t[0], t[1]) if k % 2 == 0 else (kr, dr, t[2], t[3])
            kp, dp = (a[0].ctypes.data, a[1].ctypes.data) if host else (a[2].data_ptr(), a[3].data_ptr())
            return V.fuse_rig_job(*pose, kp, dp, n, k % 2, n if k % 2 else 0, valid)

        torch.cuda.synchronize()
        jobs16 = [job(k) for k in range(16)]
        got = fe.fuse_search_rig(rig, jobs16, pts, desc, TH, FC.LSF, (W, H))
        want = V.fuse_search_rig_host(V.kb8_camera(*CAM1), rig, [job(k, True) for k in range(16)], pts, desc, TH, FC.LSF, (W, H), sf,
                                      is2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("parity", n, m)
        say("2 x %d keypoints, %d MapPoints, 16 jobs: parity with the host twin ok; found per job %s, of them <= TH_LOW %s"
            % (n, m, (got[0] >= 0).sum(1).tolist()[:4], ((got[0] >= 0) & (got[1] <= 50)).sum(1).tolist()[:4]))
        ms = {}
        for K in (1, 2, 16):
            head, hold, npts = fe._fuse_rig_call(rig, jobs16[:K], pts, desc, TH, FC.LSF, (W, H), False, None)
            bi, bd = np.zeros(K * m, np.int32), np.zeros(K * m, np.int32)

            def call():
                assert L.vslam_fuse_search_rig(*head, bi.ctypes.data_as(C.c_void_p), bd.ctypes.data_as(C.c_void_p)) == V.VSLAM_OK

            ms[K], txt = timed(call)
            fe.set_profiling(True)
            for _ in range(CALLS):
                call()
            k_ms, passes = fe.get_fuse_rig_profile()
            fe.set_profiling(False)
            assert passes == CALLS
            say("  %2d job(s) in one call, wall ms: %s   (d) k_fuse_rank_rig alone by HIP events: %.1f us" % (K, txt, k_ms / CALLS * 1e3))
        singles = [fe._fuse_rig_call(rig, jobs16[k:k + 1], pts, desc, TH, FC.LSF, (W, H), False, None) for k in range(16)]
        b1, d1 = np.zeros(m, np.int32), np.zeros(m, np.int32)
        for K in (2, 16):
            def seq():
                for s in singles[:K]:
                    assert L.vslam_fuse_search_rig(*s[0], b1.ctypes.data_as(C.c_void_p), d1.ctypes.data_as(C.c_void_p)) == V.VSLAM_OK

            s_ms, txt = timed(seq)
            say("  (b) %2d blocking 1-job calls in sequence, wall ms: %s   -> one %d-job call / sequence = %.2f" % (K, txt, K, ms[K] / s_ms))
        # (a) the pinhole entry of the same build, same counts
        pp, pd = points_on(rng, poses[0][0], pin_rays, kl, dl, m)
        m_pin = V.FMatcher(fe_pin)
        R0, t0, O0 = poses[0][0]
        pin_ms, txt = timed(lambda: m_pin.FuseSearch(pp, pd, t[0].data_ptr(), t[1].data_ptr(), n, None, R0, t0, O0,
                                                     CAM1[:4] + (0.0,), TH, FC.LSF, (W, H)))
        _, txt_rig = timed(lambda: fe.fuse_search_rig(rig, jobs16[:1], pts, desc, TH, FC.LSF, (W, H)))
        say("  (a) through the Python mirror both: pinhole vslam_fuse_search %s | 1-job rig call %s" % (txt, txt_rig))
        if m == 1500:
            hj = [job(0, True)]
            _, txt = timed(lambda: V.fuse_search_rig_host(V.kb8_camera(*CAM1), rig, hj, pts, desc, TH, FC.LSF, (W, H), sf, is2))
            say("  (c) host twin on one thread, one job, wall ms: %s" % txt)
fe.close()
fe_pin.close()
say("expectations (not thresholds): (a) the 1-job call costs the pinhole call plus the KB8 projection's extra per point; (b) a "
    "K-job call saves K - 1 stagings, copies and waits against K blocking 1-job calls")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
