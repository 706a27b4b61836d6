#!/usr/bin/env python3
"""SearchByProjection(CurrentFrame, LastFrame) of a two-fisheye rig on the GPU box.  Parity first: every case of
tests/frame_projection_rig_cases.py against the numpy restatement, and every synthetic frame below against the host twin (which
the CPU suite pins to the restatement), by the parallel resolution and by the sequential wave.  Then, for synthetic rig frames of
2 x 600, 2 x 1250 and 2 x 2000 current keypoints with as many last-frame entries, 5 rounds of 30 calls each:

  * the whole blocking vslam_search_by_projection_frame_rig call (wall ms per call: mean of the rounds [least .. greatest]),
  * the yardsticks, same run and build: vslam_search_by_projection_frame twice back to back on the same counts without a KB8
    camera (the whole last frame against the left keypoints, then against the right ones), and the host twin on one thread,
  * the two-job k_sbp_rank_rig launch and the resolution behind it alone by HIP events (vslam_fe_get_frame_rig_profile),
  * whether the sequential hand-over was taken (windows re-scanned per call; 0 = k_sbp_rig_replay returned at once).

Expectation recorded beside the numbers, not a threshold: no more than the two pinhole calls together, plus what
profiles/kb8_timing.txt shows KB8 projection costs over pinhole; one staging and one result copy replace two.

Writes profiles/frame_projection_rig_timing.txt (or the path given as the first argument).  Sets no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_projection_rig_cases as FP
import frustum_cases as FC
import kb8_cases as KC
import kb8_ref as KR
import vi_slam_amd as V

import torch

F32 = np.float32
WARM, ROUNDS, CALLS = 3, 5, 30
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frame_projection_rig_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """ms per call: mean of the rounds, least and greatest round"""
    for _ in range(WARM):
        fn()
    r = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        r.append((time.perf_counter() - t0) * 1e3 / CALLS)
    return "%.3f [%.3f .. %.3f]" % (float(np.mean(r)), min(r), max(r))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fallbacks(fe):
    n = C.c_int(0)
    V.lib().vslam_dbg_search_init_fallbacks(fe._h, C.byref(n))
    return n.value


def host_lib():
    L = C.CDLL(V.HOST_LIB_PATH)
    vp, i = C.c_void_p, C.c_int
    L.vslamh_search_by_projection_frame_rig.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, vp, vp, i, vp, vp, i, vp, vp,
                                                        C.POINTER(i)]
    return L


# ---- parity on the suite's cases
g = FP.golden()
fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
d = {k: dev(np.ascontiguousarray(g[k], V.KP_DTYPE if k[0] == "k" else np.uint8)) for k in ("kl", "dl", "kr", "dr")}
torch.cuda.synchronize()
fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
for name, c in FP.cases().items():
    wn, wm, _ = FP.reference(c)
    nl, nr = len(c["kl"]), len(c["kr"])
    fr = V.rig_frame(d["kl"].data_ptr() if nl else 0, d["dl"].data_ptr() if nl else 0, nl, d["kr"].data_ptr() if nr else 0,
                     d["dr"].data_ptr() if nr else 0, nr, None, None, c["occ"])
    P = V.proj_params(c["Tcw"], KC.LOCAL_CAM[:4], c["th"], FP.IMG, c["forward"], c["backward"], c["ori"], c["gf"])
    rig = V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), g["rig"]["Tlr"], c["Trl"])
    for seq in (0, 1):
        fe.set_tuning(sbp_sequential=seq, sbp_topm=8)
        nm, m = fe.search_by_projection_frame_rig(P, rig, c["last_kps"], c["flags"], c["x3dw"], c["desc"], fr)
        assert nm == wn and np.array_equal(m, wm), ("parity", name, seq)
fe.set_tuning(sbp_sequential=0, sbp_topm=8)
fe.close()
say("parity with tests/frame_projection_rig_ref.py on %d cases, parallel and sequential resolution: ok" % len(FP.cases()))


# ---- synthetic frames
def frame_scene(W, H, nk, sf, seed):
    """nk keypoints per camera in both frames (the scene stands still), a MapPoint on every keypoint of both cameras of the last
    frame, the rig moved by FP.current_pose()"""
    rng = np.random.default_rng(seed)

    def kps():
        k = np.zeros(nk, V.KP_DTYPE)
        k["x"], k["y"] = rng.uniform(19, W - 19, nk).astype(F32), rng.uniform(19, H - 19, nk).astype(F32)
        k["octave"] = np.minimum(rng.geometric(0.3, nk) - 1, 7)
        k["size"], k["angle"] = 31.0, rng.uniform(0, 360, nk).astype(F32)
        return k, rng.integers(0, 256, (nk, 32)).astype(np.uint8)

    (kl, dl), (kr, dr) = kps(), kps()
    f = 0.37 * W
    cam_t = (f, f * 1.004, W / 2 - 0.5, H / 2 + 0.25, KC.K_TUM, 0.0)
    cam = KR.camera(*cam_t)
    rig = KC.rig()
    Tlr = np.asarray(rig["Tlr"], np.float64)
    rl, _, _ = KR.unproject(cam, np.stack([kl["x"], kl["y"]], 1))
    rr, _, _ = KR.unproject(cam, np.stack([kr["x"], kr["y"]], 1))
    xl = rl.astype(np.float64) * rng.uniform(2.0, 6.0, (nk, 1))
    xr = (rr.astype(np.float64) * rng.uniform(2.0, 6.0, (nk, 1))) @ Tlr[:, :3].T + Tlr[:, 3]
    x3dw = np.concatenate([xl, xr]).astype(F32)  # the last frame's left camera is the world frame
    desc = np.concatenate([dl, dr])
    desc[np.arange(2 * nk), np.arange(2 * nk) % 32] ^= np.uint8(1)
    flags = np.where(np.arange(2 * nk) % 5 == 0, 1, 3).astype(np.uint8)
    return dict(kl=kl, dl=dl, kr=kr, dr=dr, cam_t=cam_t, rig=rig, last_kps=np.concatenate([kl, kr]), x3dw=x3dw, desc=desc,
                flags=flags, Tcw=FP.current_pose())


HL = host_lib()
TH = 15.0
for (W, H, nk) in ((1280, 720, 600), (1280, 720, 1250), (1280, 720, 2000)):
    fe = V.FExtractor(2000, 1.2, 8, 20, 7, W, H, max_batch=1)
    sf = np.ascontiguousarray(fe.GetScaleFactors(), F32)
    s = frame_scene(W, H, nk, sf, seed=nk)
    d = {k: dev(s[k]) for k in ("kl", "dl", "kr", "dr")}
    torch.cuda.synchronize()
    fr = V.rig_frame(d["kl"].data_ptr(), d["dl"].data_ptr(), nk, d["kr"].data_ptr(), d["dr"].data_ptr(), nk, None, None)
    P = V.proj_params(s["Tcw"], s["cam_t"][:4], TH, (W, H))
    rig = V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), s["rig"]["Tlr"], s["rig"]["Trl"])
    kcam = V.kb8_camera(*s["cam_t"])
    Trl = np.ascontiguousarray(s["rig"]["Trl"], F32)
    b = np.asarray((0.0, W, 0.0, H), F32)
    hm, hn = np.full(2 * nk, -1, np.int32), C.c_int(0)

    def twin():
        rc = HL.vslamh_search_by_projection_frame_rig(C.byref(P), C.byref(kcam), _p(Trl), _p(s["last_kps"]), 2 * nk, _p(s["flags"]),
                                                      _p(s["x3dw"]), _p(s["desc"]), _p(s["kl"]), _p(s["dl"]), nk, _p(s["kr"]),
                                                      _p(s["dr"]), nk, None, _p(sf), len(sf), _p(b), _p(hm), C.byref(hn))
        assert rc == V.VSLAM_OK

    def call():
        return fe.search_by_projection_frame_rig(P, rig, s["last_kps"], s["flags"], s["x3dw"], s["desc"], fr)

    twin()
    fe.set_kb8_camera(kcam)
    for seq in (0, 1):
        fe.set_tuning(sbp_sequential=seq, sbp_topm=8)
        nm, m = call()
        assert nm == hn.value and np.array_equal(m, hm), ("parity", nk, seq)
    fe.set_tuning(sbp_sequential=0, sbp_topm=8)
    say("2 x %d current keypoints (%d x %d), %d last-frame entries: parity with the host twin ok, %d matches (%d left, %d right)"
        % (nk, W, H, 2 * nk, hn.value, int((hm[:nk] >= 0).sum()), int((hm[nk:] >= 0).sum())))
    say("  whole rig call, wall ms per call, mean of %d rounds of %d [least .. greatest]: %s" % (ROUNDS, CALLS, timed(call)))
    for seq, name in ((0, "parallel resolution"), (1, "sequential wave")):
        fe.set_tuning(sbp_sequential=seq, sbp_topm=8)
        for _ in range(WARM):
            call()
        fallbacks(fe)
        fe.set_profiling(True)
        for _ in range(CALLS):
            call()
        rank_ms, res_ms, passes = fe.get_frame_rig_profile()
        fe.set_profiling(False)
        assert passes == CALLS
        say("  %-20s by HIP events, us per call: k_sbp_rank_rig (two jobs) %.1f | k_sbp_rig_resolve + k_sbp_rig_replay %.1f | "
            "windows re-scanned per call %.1f%s" % (name, rank_ms / passes * 1e3, res_ms / passes * 1e3, fallbacks(fe) / CALLS,
                                                    "" if seq else " (0: no hand-over)"))
    fe.set_tuning(sbp_sequential=0, sbp_topm=8)
    fe.set_kb8_camera(None)
    # the pinhole entry twice on the same counts: the whole last frame against the left keypoints, then against the right ones
    fm = V.FMatcher(fe, 0.9, True)
    cam6 = tuple(s["cam_t"][:4]) + (0.0, 1.0)
    eye = np.eye(3, 4, dtype=F32)

    def pinhole_twice():
        fm.SearchByProjection(s["Tcw"], eye, cam6, TH, s["last_kps"], s["flags"], s["x3dw"], s["desc"],
                              d["kl"].data_ptr(), d["dl"].data_ptr(), nk, None, True, (W, H))
        fm.SearchByProjection(s["Tcw"], eye, cam6, TH, s["last_kps"], s["flags"], s["x3dw"], s["desc"],
                              d["kr"].data_ptr(), d["dr"].data_ptr(), nk, None, True, (W, H))

    say("  yardstick: vslam_search_by_projection_frame twice (%d entries x %d keypoints each, pinhole), wall ms: %s" % (2 * nk, nk, timed(pinhole_twice)))
    say("  yardstick: host twin on one thread, wall ms: %s" % timed(twin))
    fe.close()
say("expectation (not a threshold): the rig call costs no more than the two pinhole calls together plus the KB8 projection's "
    "extra over pinhole (profiles/kb8_timing.txt); one staging and one result copy replace two")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
