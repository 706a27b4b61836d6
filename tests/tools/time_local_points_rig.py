#!/usr/bin/env python3
"""SearchLocalPoints of a two-fisheye rig on the GPU box.  Parity first: the device's whole chain against
tests/local_points_rig_ref.py run over the device's own frustum records (those are pinned bit for bit by the test suite), by the
prefix walk and by the full re-scan walk.  Then, for synthetic frames of 2000 and 4000 keypoints per side and local maps of
4096 / 16384 MapPoints of which about 2000 are in view:

  * the whole vslam_search_local_points_rig call from host and from device points (wall ms: median, min),
  * the yardstick, same run and build: the monocular-fisheye vslam_search_local_points on the left frame alone with the same
    MapPoints,
  * the two-job k_sbp_rank launch and k_rig_resolve alone by HIP events (vslam_fe_get_local_points_rig_profile), for the
    prefix walk and for the full re-scan walk (sbp_sequential = 1),
  * how many windows the prefix walk re-scanned in full (the hand-over).

Writes profiles/local_points_rig_timing.txt (or the path given as the first argument).  Sets no gate."""
import ctypes as C
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
import local_points_rig_cases as LC
import local_points_rig_ref as RR
import vi_slam_amd as V

import torch

F32 = np.float32
WARM, REPS = 3, 30
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "local_points_rig_timing.txt")
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def fallbacks(fe):
    n = C.c_int(0)
    V.lib().vslam_dbg_search_init_fallbacks(fe._h, C.byref(n))
    return n.value


def frame_scene(W, H, nk, n_mp, n_view, sf, seed):
    """synthetic rig frame and local map: nk keypoints per side, about n_view MapPoints on their rays, the rest behind"""
    rng = np.random.default_rng(seed)

    def kps():
        k = np.zeros(nk, V.KP_DTYPE)
        k["x"], k["y"] = rng.uniform(16, W - 16, nk).astype(F32), rng.uniform(16, H - 16, nk).astype(F32)
        k["octave"] = np.minimum(rng.geometric(0.3, nk) - 1, 7)
        k["size"], k["angle"] = 31.0, rng.uniform(0, 360, nk).astype(F32)
        return k, rng.integers(0, 256, (nk, 32)).astype(np.uint8)

    (kl, dl), (kr, dr) = kps(), kps()
    l2r = np.full(nk, -1, np.int32)
    r2l = np.full(nk, -1, np.int32)
    a, b = rng.permutation(nk)[:nk // 3], rng.permutation(nk)[:nk // 3]
    l2r[a], r2l[b] = b, a
    f = 0.37 * W
    cam_t = (f, f * 1.004, W / 2 - 0.5, H / 2 + 0.25, KC.K_TUM, 0.0)
    cam2_t = (f * 1.05, f * 1.05, W / 2 + 0.25, H / 2 - 0.5, KC.K_STRONG, 0.0)
    cam, cam2 = KR.camera(*cam_t), KR.camera(*cam2_t)
    rig = dict(KC.rig(), cam2=cam2)
    T, Ow = FC.pose(FC.rotation(-0.12, 0.2, 0.05), (0.2, -0.1, 0.3))
    P = FR.params(T, Ow, cam_t[:4] + (KC.MBF,), FC.LSF, (W, H), 0.5, far_points=True, th_far_points=40.0)
    M, twc_r = KR.rig_right_pose(P, rig)
    half = n_view // 2
    il, ir = rng.permutation(nk)[:half], rng.permutation(nk)[:half]
    left = LC._on_rays(cam, T[:, :3], T[:, 3], Ow, kl[il], rng.uniform(2.0, 6.0, half), sf)
    right = LC._on_rays(cam2, M[:, :3], M[:, 3], twc_r, kr[ir], rng.uniform(2.0, 6.0, half), sf)
    desc = np.concatenate([dl[il], dr[ir]])
    desc[np.arange(len(desc)), np.arange(len(desc)) % 32] ^= np.uint8(1)
    m = n_mp - 2 * half
    junk = FC.random_points(rng, m, T, Ow, spread=2.6, zr=(-9.0, -1.0))  # behind the camera: tested, never in view
    pts = np.concatenate([left, right, junk])
    desc = np.concatenate([desc, rng.integers(0, 256, (m, 32)).astype(np.uint8)])
    order = rng.permutation(n_mp)
    pts, desc = pts[order], desc[order]
    pts["flags"] = np.where(np.arange(n_mp) % 3 == 0, 3, 1)
    return dict(kl=kl, dl=dl, kr=kr, dr=dr, l2r=l2r, r2l=r2l, P=P, cam_t=cam_t, cam2_t=cam2_t, rig=rig, pts=pts, desc=desc)


for (W, H, nk) in ((1280, 720, 2000), (1920, 1080, 4000)):
    fe = V.FExtractor(nk, 1.2, 8, 20, 7, W, H, max_batch=1)
    sf = np.asarray(fe.GetScaleFactors(), F32)
    for n_mp in (4096, 16384):
        s = frame_scene(W, H, nk, n_mp, 2000, sf, seed=nk + n_mp)
        d = {k: dev(s[k]) for k in ("kl", "dl", "kr", "dr")}
        torch.cuda.synchronize()
        frame = V.rig_frame(d["kl"].data_ptr(), d["dl"].data_ptr(), nk, d["kr"].data_ptr(), d["dr"].data_ptr(), nk, s["l2r"],
                            s["r2l"])
        P = s["P"]
        vp = V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                              (W, H), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])
        crig = V.kb8_rig(V.kb8_camera(*s["cam2_t"]), s["rig"]["Tlr"], s["rig"]["Trl"])
        fe.set_kb8_camera(V.kb8_camera(*s["cam_t"]))
        # parity: the reference matcher over the device's records
        tl, tr, dl_, dr_, nv = fe.frame_in_frustum_rig(vp, crig, s["pts"])
        fl, fr = RR.far_filtered_rig(P, tl, tr, dl_)
        wn, wm, cen = RR.search_by_projection_rig(fl, fr, s["desc"], s["kl"], s["dl"], s["kr"], s["dr"], s["l2r"], s["r2l"], sf,
                                                  (0.0, float(W), 0.0, float(H)), 3.0, 0.8, None)
        kept = len(RR.kept_indices(fl, fr))
        for seq in (0, 1):
            fe.set_tuning(sbp_sequential=seq, sbp_topm=8)
            got = fe.search_local_points_rig(vp, crig, s["pts"], s["desc"], frame, 3.0, 0.8)
            assert got[0] == wn and np.array_equal(got[1], wm) and got[2] == nv and got[3] == kept, ("parity", seq)
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        say("%d keypoints per side (%d x %d), %d MapPoints, %d in view, %d handed on: parity ok (%d writes; cross-writes %d left, "
            "%d right)" % (nk, W, H, n_mp, nv, kept, wn, cen["left_cross"], cen["right_cross"]))
        dpts, ddesc = dev(np.ascontiguousarray(s["pts"], V.MAP_POINT_DTYPE)), dev(s["desc"])
        torch.cuda.synchronize()
        host = timed(lambda: fe.search_local_points_rig(vp, crig, s["pts"], s["desc"], frame, 3.0, 0.8))
        devi = timed(lambda: fe.search_local_points_rig(vp, crig, dpts.data_ptr(), ddesc.data_ptr(), frame, 3.0, 0.8, n_mp=n_mp))
        mono_h = timed(lambda: fe.search_local_points(vp, s["pts"], s["desc"], d["kl"].data_ptr(), d["dl"].data_ptr(), nk, None,
                                                      None, 3.0, 0.8))
        mono_d = timed(lambda: fe.search_local_points(vp, dpts.data_ptr(), ddesc.data_ptr(), d["kl"].data_ptr(),
                                                      d["dl"].data_ptr(), nk, None, None, 3.0, 0.8, n_mp=n_mp))
        say("  whole call, wall ms (median, min): rig from host %.3f %.3f | rig from device %.3f %.3f | mono (left frame alone) "
            "from host %.3f %.3f | mono from device %.3f %.3f | rig / mono from device %.2f"
            % (host + devi + mono_h + mono_d + (devi[0] / mono_d[0],)))
        for seq, name in ((0, "prefix walk"), (1, "full re-scan walk")):
            fe.set_tuning(sbp_sequential=seq, sbp_topm=8)
            call = lambda: fe.search_local_points_rig(vp, crig, dpts.data_ptr(), ddesc.data_ptr(), frame, 3.0, 0.8, n_mp=n_mp)
            for _ in range(WARM):
                call()
            fallbacks(fe)
            fe.set_profiling(True)
            for _ in range(REPS):
                call()
            rank_ms, res_ms, passes = fe.get_local_points_rig_profile()
            fe.set_profiling(False)
            assert passes == REPS
            say("  %-18s by HIP events, us per call: k_sbp_rank (two jobs) %.1f | k_rig_resolve %.1f | windows re-scanned per "
                "call %.1f" % (name, rank_ms / passes * 1e3, res_ms / passes * 1e3, fallbacks(fe) / REPS))
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        fe.set_kb8_camera(None)
    fe.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
