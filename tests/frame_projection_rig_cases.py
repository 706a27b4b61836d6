"""Deterministic inputs of the rig (two-fisheye, Nleft != -1) SearchByProjection(CurrentFrame, LastFrame) tests:
tests/test_frame_projection_rig_cpu.py, tests/test_gpu_frame_projection_rig.py, tests/test_cpp_frame_rig.py,
tests/tools/time_frame_projection_rig.py.

Keypoints and descriptors are the committed golden's (tests/golden/pipeline_hut_320x240.npz): kL / dL as the left camera, kR / dR
as the right one, of the last AND of the current frame (the scene stands still, the rig moves).  The left camera is
kb8_cases.LOCAL_CAM, the rig kb8_cases.rig(): its cam2 ("strong") differs from the left camera, and the function never reads it.
The last frame's left camera is the world frame.

A MapPoint "on left keypoint i" lies on the ray of kL[i] of the last frame's left camera.  A MapPoint "on right keypoint j" lies
where the function will look for it: on the ray that the LEFT camera's model gives pixel kR[j] in the right camera's frame
(fmatcher.cpp:2596 projects x3Dr through mpCamera).  `aim` shifts the pixel.

cases() -> name -> dict(Tcw, Trl, th, last_kps, nll (LastFrame.Nleft), flags, x3dw, desc, kl, dl, kr, dr, occ, forward,
backward, ori, gf, takes); `takes` names the census entries of tests/frame_projection_rig_ref.py the case is there for.
reference(c) evaluates one with the numpy restatement (cached)."""
import os

import numpy as np

import frame_projection_rig_ref as RR
import frustum_cases as FC
import kb8_cases as KC
import kb8_ref as KR
from oracle import orbo
from projection_bounds_ref import _gemm_row, _in_closed, _query
from undistort_ref import Grid, hamming

F32 = np.float32
BOUNDS = (0.0, float(FC.HUT_W), 0.0, float(FC.HUT_H))
IMG = (FC.HUT_W, FC.HUT_H)
_cache = {}


def golden():
    if "g" not in _cache:
        p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
        sf = np.asarray(orbo.Extractor(FC.HUT_NF).tables()["scale"], F32)
        _cache["g"] = dict(kl=p["kL"], dl=p["dL"], kr=p["kR"], dr=p["dR"], sf=sf, cam=KR.camera(*KC.LOCAL_CAM), rig=KC.rig())
    return _cache["g"]


def current_pose():
    """the current frame's Tcw: the rig has moved a few centimetres and turned a little since the last frame"""
    T, _ = FC.pose(FC.rotation(0.004, -0.006, 0.003), (0.03, -0.01, 0.04))
    return np.asarray(T, F32)


def _world(T, xc):
    """x_w with Rcw * x_w + tcw = xc"""
    T = np.asarray(T, np.float64)
    return ((np.asarray(xc, np.float64) - T[:, 3]) @ T[:, :3]).astype(F32)


def on_left(g, T, i, z, aim=(0.0, 0.0)):
    """a MapPoint whose left projection under T is kL[i] + aim, at depth-scale z"""
    ray, _, _ = KR.unproject(g["cam"], np.array([[g["kl"]["x"][i] + aim[0], g["kl"]["y"][i] + aim[1]]], F32))
    return _world(T, ray[0].astype(np.float64) * z)


def on_right(g, T, j, z, aim=(0.0, 0.0)):
    """a MapPoint whose right projection under T (through the left camera's model) is kR[j] + aim"""
    ray, _, _ = KR.unproject(g["cam"], np.array([[g["kr"]["x"][j] + aim[0], g["kr"]["y"][j] + aim[1]]], F32))
    Tlr = np.asarray(g["rig"]["Tlr"], np.float64)
    xr = ray[0].astype(np.float64) * z
    return _world(T, Tlr[:, :3] @ xr + Tlr[:, 3])


def _kp(src, k, angle=None):
    out = np.zeros((), src.dtype)
    for f in src.dtype.names:
        out[f] = src[f][k]
    if angle is not None:
        out["angle"] = F32(angle % 360.0)
    return out


def left_state(g, T, xw, octave, th, lv=None):
    """what the left branch does with a MapPoint: 'invz', 'out', 'empty' (the three `continue`s) or the window's keypoints"""
    T = np.asarray(T, F32).reshape(3, 4)
    xc = [_gemm_row(T[r, :3], xw, T[r, 3], True) for r in range(3)]
    with np.errstate(all="ignore"):
        if F32(np.float64(1.0) / np.float64(xc[2])) < 0:
            return "invz"
    u, v = RR.kb8_project(g["cam"], *xc)
    if not _in_closed(u, v, [F32(b) for b in BOUNDS]):
        return "out"
    if "grid_l" not in _cache:
        _cache["grid_l"] = Grid(g["kl"], BOUNDS)
    w = _query(_cache["grid_l"], u, v, F32(F32(th) * g["sf"][octave]), *(lv or (octave - 1, octave + 1)))
    return w if w else "empty"


def _case(g, T, rows, **kw):
    """rows: (last-frame keypoint record, flags, world position, descriptor)"""
    c = dict(Tcw=np.asarray(T, F32), Trl=np.asarray(g["rig"]["Trl"], F32), th=15.0, kl=g["kl"], dl=g["dl"], kr=g["kr"],
             dr=g["dr"], occ=None, forward=False, backward=False, ori=True, gf=False, takes=())
    c["last_kps"] = np.array([r[0] for r in rows], g["kl"].dtype).reshape(-1)
    c["flags"] = np.array([r[1] for r in rows], np.uint8).reshape(-1)
    c["x3dw"] = np.array([r[2] for r in rows], F32).reshape(-1, 3)
    c["desc"] = np.array([r[3] for r in rows], np.uint8).reshape(-1, 32)
    c["nll"] = len(rows)
    c.update(kw)
    return c


def _right_rows(g, T, th, want, limit, flags=3, aim=(0.0, 0.0), z=3.0, pick=None, angle_bin=None):
    """up to `limit` MapPoints on right keypoints whose left branch ends as `want` ('invz', 'out', 'empty' or 'window')"""
    rows = []
    for j in (range(len(g["kr"])) if pick is None else pick):
        xw = on_right(g, T, j, z, aim)
        o = int(g["kr"]["octave"][j])
        st = left_state(g, T, xw, o, th)
        if (st if isinstance(st, str) else "window") != want:
            continue
        ang = None if angle_bin is None else float(g["kr"]["angle"][j]) + 30.0 * angle_bin
        rows.append((_kp(g["kr"], j, ang), flags, xw, g["dr"][j]))
        if len(rows) == limit:
            break
    assert rows, want
    return rows


def scene(n_left=None, n_right=None):
    """the realistic one: a MapPoint on every keypoint of both cameras of the last frame, one bit of its descriptor flipped; one
    in five has no observations, one in eleven is an outlier; twelve MapPoints sit in a left AND a right slot of the last frame"""
    g = golden()
    T = current_pose()
    rng = np.random.default_rng(61)
    kl, kr = g["kl"], g["kr"]
    nl, nr = len(kl), len(kr)
    rows = []
    for i in range(nl):
        d = g["dl"][i].copy()
        d[i % 32] ^= np.uint8(1)
        rows.append((_kp(kl, i), 0, on_left(g, np.eye(3, 4), i, rng.uniform(2.0, 6.0)), d))
    for j in range(nr):
        d = g["dr"][j].copy()
        d[j % 32] ^= np.uint8(2)
        rows.append((_kp(kr, j), 0, on_right(g, np.eye(3, 4), j, rng.uniform(2.0, 6.0)), d))
    c = _case(g, T, rows, nll=nl)
    k = np.arange(nl + nr)
    c["flags"] = np.where(k % 11 == 5, 0, np.where(k % 5 == 0, 1, 3)).astype(np.uint8)
    for n, i in enumerate(range(7, 7 + 12 * 9, 9)):  # the same MapPoint in left slot i and right slot j of the last frame
        j = nl + 3 + 5 * n
        c["x3dw"][j], c["desc"][j] = c["x3dw"][i], c["desc"][i]
        c["flags"][i], c["flags"][j] = 1, 3
    return c


def cases():
    if "c" in _cache:
        return _cache["c"]
    g = golden()
    T = current_pose()
    kl, dl, kr, dr, sf = g["kl"], g["dl"], g["kr"], g["dr"], g["sf"]
    nl, nr = len(kl), len(kr)
    out = {}
    s = scene()
    out["scene"] = dict(s, takes=("neither", "left_match", "right_match", "last_octave_from_right_array", "same_point_both_slots",
                                  "overwrite_without_observations"))
    out["scene_forward"] = dict(s, forward=True, takes=("forward",))
    out["scene_backward"] = dict(s, backward=True, takes=("backward",))
    occ = (np.random.default_rng(62).random(nl + nr) < 0.2).astype(np.uint8)
    out["scene_occupied"] = dict(s, occ=occ, th=7.0, takes=("left_all_occupied_right_matches",))
    out["scene_gemm_float"] = dict(s, gf=True)
    out["scene_no_orientation"] = dict(s, ori=False, th=30.0)
    e_k, e_d = kl[:0], dl[:0]
    out["no_right"] = dict(s, kr=e_k, dr=e_d, takes=("right_empty_window",))
    out["no_left"] = dict(s, kl=e_k, dl=e_d)
    out["no_last"] = dict(s, last_kps=s["last_kps"][:0], flags=s["flags"][:0], x3dw=s["x3dw"][:0], desc=s["desc"][:0], nll=0)
    # a left `continue` in front of a right window that would match, once per kind
    out["left_invz"] = _case(g, T, _right_rows(g, T, 15.0, "invz", 12), takes=("left_invz_skips_right",))
    out["left_out_of_frame"] = _case(g, T, _right_rows(g, T, 15.0, "out", 12), takes=("left_out_of_frame_skips_right",))
    out["left_empty_window"] = _case(g, T, _right_rows(g, T, 2.0, "empty", 12), th=2.0,
                                     takes=("left_empty_window_skips_right",))
    # left candidates all occupied from the start, a right match behind
    occ = np.zeros(nl + nr, np.uint8)
    occ[:nl] = 1
    out["left_all_occupied"] = _case(g, T, _right_rows(g, T, 30.0, "window", 12), th=30.0, occ=occ,
                                     takes=("left_all_occupied_right_matches",))
    # a right projection a few pixels outside the bounds whose window still reaches the keypoint
    # (keypoints keep 19 px and more from the border: the aim is 4 px outside, the radius 30 px times the scale factor)
    rows = []
    for j in range(nr):
        x, y = float(kr["x"][j]), float(kr["y"][j])
        aims = [a for a, d in (((-(x + 4.0), 0.0), x), ((0.0, -(y + 4.0)), y), ((FC.HUT_W - x + 4.0, 0.0), FC.HUT_W - x),
                               ((0.0, FC.HUT_H - y + 4.0), FC.HUT_H - y)) if d < 25.0]
        if not aims:
            continue
        aim = aims[0]
        if not isinstance(left_state(g, T, on_right(g, T, j, 3.0, aim), int(kr["octave"][j]), 30.0), str):
            rows += _right_rows(g, T, 30.0, "window", 1, aim=aim, pick=[j])
    assert rows
    out["right_outside_bounds"] = _case(g, T, rows[:20], th=30.0, occ=occ, takes=("right_uv_outside_bounds_matches",))
    # x3Dr behind the right camera (theta > pi / 2 lands beyond the image; the window reaches border keypoints)
    rows = []
    for i in range(nl):
        if len(rows) == 40:
            break
        for z in (0.4, 1.0, 3.0):
            xw = on_left(g, T, i, z)
            Tc = np.asarray(T, np.float64)
            xc = Tc[:, :3] @ xw.astype(np.float64) + Tc[:, 3]
            Trl = np.asarray(g["rig"]["Trl"], np.float64)
            if (Trl[:, :3] @ xc + Trl[:, 3])[2] < -0.05:
                rows.append((_kp(kl, i), 3, xw, dl[i]))
                break
    assert rows
    out["right_behind"] = _case(g, T, rows, th=40.0, takes=("right_behind_camera",))
    # a non-blocking overwrite pair: two MapPoints on one left keypoint, the first without observations
    rows = []
    for i in range(0, 40, 2):
        rows.append((_kp(kl, i), 1, on_left(g, T, i, 3.0), dl[i]))
        rows.append((_kp(kl, i), 3, on_left(g, T, i, 4.0), dl[i]))
    out["overwrite"] = _case(g, T, rows, takes=("overwrite_without_observations",))
    # last-frame arrays whose octaves differ at equal local index: entry nll + k reads keypointsRight_[k], not keypoints_[k]
    ks = [k for k in range(min(nl, nr)) if kl["octave"][k] != kr["octave"][k]][:16]
    rows = [(_kp(kl, k), 3, on_left(g, T, k, 3.0), dl[k]) for k in ks]
    rows += [(_kp(kr, k), 3, on_left(g, T, k, 3.5), dl[k]) for k in ks]
    out["octave_arrays"] = _case(g, T, rows, nll=len(ks), th=7.0, takes=("last_octave_from_right_array",))
    # one histogram over both sides: five left matches in bin 2, right matches 8 / 7 / 6 in bins 5, 8, 11; the left slots but
    # the five targets are occupied, so that the right-side MapPoints' left windows hold candidates and match nothing
    free = list(range(3, 3 + 5 * 7, 7))
    occ = np.zeros(nl + nr, np.uint8)
    occ[:nl] = 1
    occ[free] = 0
    rows = [(_kp(kl, i, float(kl["angle"][i]) + 60.0), 3, on_left(g, T, i, 3.0), dl[i]) for i in free]
    right = _right_rows(g, T, 30.0, "window", 21)
    assert len(right) == 21
    for n, r in enumerate(right):
        b = 5 if n < 8 else 8 if n < 15 else 11
        kp = r[0].copy()
        kp["angle"] = F32((float(kp["angle"]) + 30.0 * b) % 360.0)
        rows.append((kp, 3, r[2], r[3]))
    out["joint_histogram"] = _case(g, T, rows, th=30.0, occ=occ, nll=len(free), takes=("joint_histogram_rejects",))
    # a window with more occupied candidates than the sorted prefix holds: the ten nearest descriptors of the window are taken
    # from the start, the eleventh is the match (sbp_topm 1, 2, 8 all run out)
    rows, occ = [], np.zeros(nl + nr, np.uint8)
    H = hamming(dl, dl)
    for i in range(nl):
        o = int(kl["octave"][i])
        w = left_state(g, T, on_left(g, T, i, 3.0), o, 40.0)
        if isinstance(w, str) or len(w) < 12:
            continue
        ordered = sorted(w, key=lambda c: (H[i, c], c))
        if H[i, ordered[10]] > 100 or occ[ordered[:11]].any():
            continue
        occ[ordered[:10]] = 1
        rows.append((_kp(kl, i), 3, on_left(g, T, i, 3.0), dl[i]))
        if len(rows) == 4:
            break
    assert rows
    out["prefix_overflow"] = _case(g, T, rows, th=40.0, occ=occ, takes=("left_match",))
    _cache["c"] = out
    return out


PREFIX_CASES = ("prefix_overflow", "scene_occupied", "left_all_occupied")


def reference(c, **kw):
    """the numpy restatement on a case -> (nmatches, match, census); kw overrides (per_side_hist, project)"""
    key = ("ref", id(c), tuple(sorted(kw)))
    if kw or key not in _cache:
        r = RR.search_by_projection_frame_rig(c["Tcw"], c["Trl"], golden()["cam"], c["th"], c["last_kps"], c["flags"], c["x3dw"],
                                              c["desc"], c["kl"], c["dl"], c["kr"], c["dr"], golden()["sf"], BOUNDS, c["forward"],
                                              c["backward"], c["ori"], c["occ"], not c["gf"], n_last_left=c["nll"], **kw)
        if kw:
            return r
        _cache[key] = r
    return _cache[key]
