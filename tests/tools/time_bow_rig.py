#!/usr/bin/env python3
"""SearchByBoW(KeyFrame, Frame) of a two-fisheye rig on the GPU box.  Parity first: every case of tests/bow_rig_cases.py against
the numpy restatement, and every synthetic scene below against the host twin (which the CPU suite pins to the restatement).
Then, for rig frames of 2 x 600, 2 x 1250 and 2 x 2000 features against K = 1, 4 and 16 rig keyframes of the same size (a
k = 10, L = 4 vocabulary at levelsup 2: 100 nodes, as ORBvoc at levelsup 4), 5 rounds of 30 calls each:

  * the whole blocking vslam_search_by_bow_rig call with its arguments prepared once (wall ms per call: mean of the rounds
    [least .. greatest]),
  * k_sbow_nodes_rig and k_sbow_finish_rig alone by HIP events (vslam_fe_get_bow_rig_profile),
  * the yardsticks, same run and build: vslam_search_by_bow on a pinhole frame and keyframe with as many features in total
    (K = 1), K blocking calls of it in sequence (the batch), and the host twin on one thread (one keyframe).

Expectations recorded beside the numbers, not thresholds: K = 1 costs no more than the pinhole call plus the third reduction;
the batch costs clearly less than K blocking calls.

Writes profiles/bow_rig_timing.txt (or the path given as the first argument).  Sets no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bow_rig_cases as BC
import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

import torch

WARM, ROUNDS, CALLS = 3, 5, 30
RATIO, ORI, LEVELSUP = 0.7, True, 2
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bow_rig_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, calls=CALLS):
    """ms per call: mean of the rounds, least and greatest round"""
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


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


fe = V.FExtractor(1000, 1.2, 8, 20, 7, 640, 480, max_batch=1)
keep = []


def job_of(k):
    nl = k["n_left"]
    t = [dev(k["desc"][:nl]) if nl else None, dev(k["desc"][nl:]) if len(k["desc"]) > nl else None]
    keep.append(t)
    return dict(kps=k["kps"], flags=k["flags"], fv=k["fv"], n_left=nl, n_right=len(k["kps"]) - nl,
                dev_desc_left=t[0].data_ptr() if t[0] is not None else 0, dev_desc_right=t[1].data_ptr() if t[1] is not None else 0)


def frame_of(f):
    nl, n = f["n_left"], len(f["kps"])
    t = [dev(np.ascontiguousarray(f["kps"][:nl], V.KP_DTYPE)), dev(f["desc"][:nl]), dev(np.ascontiguousarray(f["kps"][nl:], V.KP_DTYPE)),
         dev(f["desc"][nl:])]
    keep.append(t)
    return V.rig_frame(t[0].data_ptr(), t[1].data_ptr(), nl, t[2].data_ptr(), t[3].data_ptr(), n - nl, None, None)


# ---- parity on the suite's cases
for name, c in BC.cases().items():
    want = BC.reference(c)
    job, fr = job_of(c["kf"]), frame_of(c["f"])
    torch.cuda.synchronize()
    got = V.FMatcher(fe, c["ratio"], c["ori"]).SearchByBoWRig([job], fr, c["f"]["fv"])[0]
    assert got[0] == want[0] and np.array_equal(got[1], want[1]), ("parity", name)
torch.cuda.synchronize()
say("parity with tests/bow_rig_ref.py on %d cases: ok" % len(BC.cases()))

# ---- synthetic scenes
voc = synth.make_vocabulary(10, 4, seed=17)
leaves = np.nonzero(voc["child_count"] == 0)[0]


def noisy(rng, d, lo, hi):
    d = d.copy()
    for i in range(len(d)):
        for b in rng.choice(256, int(rng.integers(lo, hi)), replace=False):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def side(rng, desc, n_left):
    k = np.zeros(len(desc), V.KP_DTYPE)
    k["angle"] = rng.uniform(0, 360, len(desc)).astype(np.float32)
    t = orbo.bow_transform(voc, desc, LEVELSUP)
    return dict(kps=k, desc=np.ascontiguousarray(desc), n_left=n_left, fv={q: t[q] for q in ("fv_nodes", "fv_off", "fv_feat")})


def scene(n, K, seed):
    """a world of 2n descriptors near vocabulary words; K rig keyframes see noisy copies of it, the frame another copy"""
    rng = np.random.default_rng(seed)
    world = noisy(rng, voc["desc"][rng.choice(leaves, 2 * n)], 4, 12)
    kfs = []
    for _ in range(K):
        k = side(rng, noisy(rng, world[rng.permutation(2 * n)], 2, 30), n)
        k["flags"] = (rng.random(2 * n) < 0.85).astype(np.uint8)
        kfs.append(k)
    return kfs, side(rng, noisy(rng, world[rng.permutation(2 * n)], 2, 30), n)


L = V.lib()
for n in (600, 1250, 2000):
    for K in (1, 4, 16):
        kfs, f = scene(n, K, seed=n + K)
        m = V.FMatcher(fe, RATIO, ORI)
        jobs, fr = [job_of(k) for k in kfs], frame_of(f)
        torch.cuda.synchronize()
        got = m.SearchByBoWRig(jobs, fr, f["fv"])
        for j, k in enumerate(kfs):
            want = V.search_by_bow_rig_host(k["kps"], k["desc"], k["n_left"], k["flags"], k["fv"], f["kps"], f["desc"], f["n_left"],
                                            f["fv"], RATIO, ORI)
            assert got[j][0] == want[0] and np.array_equal(got[j][1], want[1]), ("parity", n, K, j)
        per_node = np.diff(f["fv"]["fv_off"])
        say("2 x %d frame features against %d rig keyframe(s) of 2 x %d: parity with the host twin ok; %d frame nodes, at most %d "
            "features under one; matches of keyframe 0: %d (%d left, %d right)"
            % (n, K, n, len(per_node), int(per_node.max()), got[0][0], int((got[0][1][:n] >= 0).sum()), int((got[0][1][n:] >= 0).sum())))
        head, hold, N = m._bow_rig_call(jobs, fr, f["fv"])
        tab, ptrs, nm = m._bow_rig_outputs(K, N)

        def rig_call():
            assert L.vslam_search_by_bow_rig(*head, ptrs, nm) == V.VSLAM_OK

        rig_ms, txt = timed(rig_call)
        say("  whole rig call, wall ms per call, mean of %d rounds of %d [least .. greatest]: %s" % (ROUNDS, CALLS, txt))
        fe.set_profiling(True)
        a0, b0, p0 = C.c_double(0), C.c_double(0), C.c_long(0)
        L.vslam_fe_get_bow_rig_profile(fe._h, C.byref(a0), C.byref(b0), C.byref(p0))
        for _ in range(CALLS):
            rig_call()
        a1, b1, p1 = C.c_double(0), C.c_double(0), C.c_long(0)
        L.vslam_fe_get_bow_rig_profile(fe._h, C.byref(a1), C.byref(b1), C.byref(p1))
        fe.set_profiling(False)
        assert p1.value - p0.value == CALLS
        say("  by HIP events, us per call: k_sbow_nodes_rig %.1f | k_sbow_finish_rig %.1f"
            % ((a1.value - a0.value) / CALLS * 1e3, (b1.value - b0.value) / CALLS * 1e3))
        # the pinhole entry on as many features in total, once per keyframe
        pin = []
        for k in kfs:
            t = (dev(k["desc"]), dev(f["desc"]))
            keep.append(t)
            a = [np.ascontiguousarray(k["fv"][q], np.int32) for q in ("fv_nodes", "fv_off", "fv_feat")]
            b = [np.ascontiguousarray(f["fv"][q], np.int32) for q in ("fv_nodes", "fv_off", "fv_feat")]
            out, cnt = np.full(2 * n, -1, np.int32), C.c_int(0)
            keep.append((a, b, out, cnt))
            pin.append((fe._h, _p(k["kps"]), C.c_void_p(t[0].data_ptr()), _p(k["flags"]), 2 * n, _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]),
                        _p(f["kps"]), C.c_void_p(t[1].data_ptr()), 2 * n, _p(b[0]), _p(b[1]), _p(b[2]), len(b[0]), C.c_float(RATIO),
                        int(ORI), _p(out), C.byref(cnt)))
        torch.cuda.synchronize()

        def pinhole_calls():
            for a in pin:
                assert L.vslam_search_by_bow(*a) == V.VSLAM_OK

        pin_ms, txt = timed(pinhole_calls)
        say("  yardstick: vslam_search_by_bow, %d blocking call(s) in sequence (pinhole, 2 x %d features in one array), wall ms: %s"
            "   -> rig / pinhole = %.2f" % (K, n, txt, rig_ms / pin_ms))
        if K == 1:
            k = kfs[0]
            _, txt = timed(lambda: V.search_by_bow_rig_host(k["kps"], k["desc"], k["n_left"], k["flags"], k["fv"], f["kps"], f["desc"],
                                                            f["n_left"], f["fv"], RATIO, ORI))
            say("  yardstick: host twin on one thread, one keyframe, wall ms: %s" % txt)
        keep.clear()
fe.close()
say("expectations (not thresholds): K = 1 costs no more than the pinhole call plus the third reduction; the batch costs clearly "
    "less than K blocking calls, since one staging, one copy and one wait replace K")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
