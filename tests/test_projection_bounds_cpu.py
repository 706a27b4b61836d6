"""CPU: the float-bounds reference of the projection / fusion / Sim3 matchers (tests/projection_bounds_ref.py).

1. The restatement is pinned: at bounds {0, w, 0, h} every function equals the oracle, on the scenes of
   tests/test_gpu_projection.py and tests/test_gpu_mapping.py (rebuilt with the CPU oracle: same poses, th, flags, both
   gemm settings) and on tests/golden/tracking_hut_320x240.npz.
2. The inputs of the GPU tests bite: per camera and matcher the result at the float bounds differs from the one at
   {0, w, 0, h}, an accepted query projects outside the image but inside the bounds, and a matched keypoint's undistorted
   position lies outside the image.
3. The band inputs tell a KeyFrame's integer bounds from the Frame's float ones: a projection between floor(mnMaxX) and
   mnMaxX (and between mnMinX and ceil(mnMinX)) matches over the floats and is outside over the integers."""
import os

import numpy as np
import pytest

import projection_bounds_cases as PC
import projection_bounds_ref as R
from oracle import orbo
from vi_slam_amd import synth

W, H, NF = 1241, 376, 2000
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
MB = BF / FX
B = (0, W, 0, H)
LSF = float(np.log(np.float32(1.2)).astype(np.float32))
_pose = PC.pose


@pytest.fixture(scope="module")
def scene():
    """the scene of the two GPU test modules, from the CPU oracle"""
    L0, R0 = synth.make_stereo_pair(W, H, step=0)
    L1, R1 = synth.make_stereo_pair(W, H, step=1)
    ex = [orbo.Extractor(NF) for _ in range(4)]
    (k0, de0, _), (kr0, dr0, _), (k1, de1, _), (kr1, dr1, _) = [e.compute(i) for e, i in zip(ex, (L0, R0, L1, R1))]
    u0, z0, _, _ = orbo.stereo(ex[0], ex[1], k0, de0, kr0, dr0, BF, FX)
    u1, z1, _, _ = orbo.stereo(ex[2], ex[3], k1, de1, kr1, dr1, BF, FX)
    z = np.where(z0 > 0, z0, 20.0).astype(np.float32)
    X = np.stack([(k0["x"] - CX) / FX * z, (k0["y"] - CY) / FY * z, z], 1).astype(np.float32)
    tab = ex[0].tables()
    return dict(k0=k0, de0=de0, k1=k1, de1=de1, u0=u0, u1=u1, z0=z0, z1=z1, X=X, z=z, has_depth=z0 > 0, sf=tab["scale"],
                isig2=tab["inv_sigma2"])


def _shift(s, zmed):
    return _pose(tx=3.0 / FX * zmed, ty=1.0 / FY * zmed)


def _frame(s, Tcw, th, flags, mono=False, check_ori=True, u_right=True, occupied=None, gemm_float=False):
    cam = (FX, FY, CX, CY, BF, MB)
    ur = s["u1"] if u_right else np.full(len(s["k1"]), -1, np.float32)
    a = (Tcw, _pose(), cam, th, s["k0"], flags, s["X"], s["de0"], s["k1"], s["de1"], ur, s["sf"])
    wn, wm, wd = orbo.search_by_projection_frame(*a, W, H, mono=mono, check_ori=check_ori, occupied=occupied,
                                                 gemm_double=not gemm_float)
    n, m, d = R.search_by_projection_frame(*a, B, mono, check_ori, occupied, not gemm_float)
    assert (n, d) == (wn, wd) and np.array_equal(m, wm)
    return n


def test_frame_form_equals_oracle(scene):
    s = scene
    zmed = float(np.median(s["z"][s["has_depth"]]))
    T = _shift(s, zmed)
    n0 = len(s["k0"])
    flags = np.where(s["has_depth"], 3, 0).astype(np.uint8)
    assert _frame(s, T, 15, flags) > 200
    _frame(s, T, 7, flags)
    _frame(s, T, 30, flags)
    _frame(s, T, 15, flags, gemm_float=True)
    full = np.full(n0, 3, np.uint8)
    _frame(s, T, 30, np.random.default_rng(3).integers(0, 4, n0).astype(np.uint8))
    _frame(s, _pose(tz=-1.0), 15, full)
    _frame(s, _pose(tz=1.0), 15, full)
    _frame(s, _pose(tz=-1.0), 15, full, mono=True, u_right=False)
    _frame(s, _pose(tx=0.05, yaw=0.01), 15, full, check_ori=False)
    rng = np.random.default_rng(7)
    fl = rng.integers(0, 4, n0).astype(np.uint8)
    occ = (rng.random(len(s["k1"])) < 0.2).astype(np.uint8)
    _frame(s, T, 15, fl, occupied=occ)
    _frame(s, T, 30, np.full(n0, 1, np.uint8))
    assert _frame(s, _pose(tz=-1000.0), 15, full) == 0


def _local_map(s, seed, jitter=2.0, frac_in_view=0.85):
    rng = np.random.default_rng(seed)
    k0 = s["k0"]
    n = len(k0)
    mps = np.zeros(n, orbo.MP_TRACK_DTYPE)
    mps["proj_x"] = (k0["x"] + 3.0 + rng.normal(0, jitter, n)).astype(np.float32)
    mps["proj_y"] = (k0["y"] + 1.0 + rng.normal(0, jitter, n)).astype(np.float32)
    mps["proj_xr"] = (mps["proj_x"] - BF / np.maximum(s["z"], 1.0)).astype(np.float32)
    mps["view_cos"] = rng.choice(np.array([0.9, 0.9985, 1.0], np.float32), n)
    mps["level"] = np.clip(k0["octave"] + rng.integers(-1, 2, n), 0, 7)
    inview = rng.random(n) < frac_in_view
    obs = rng.random(n) < 0.9
    mps["flags"] = (inview.astype(np.uint32)) | (obs.astype(np.uint32) << 1)
    return mps


@pytest.mark.parametrize("th,nnratio,seed", [(1.0, 0.8, 1), (3.0, 0.8, 2), (5.0, 0.6, 3)])
def test_mappoints_form_equals_oracle(scene, th, nnratio, seed):
    s = scene
    mps = _local_map(s, seed)
    occ = (np.random.default_rng(100 + seed).random(len(s["k1"])) < 0.3).astype(np.uint8)
    for occupied in (None, occ):
        wn, wm = orbo.search_by_projection_mappoints(mps, s["de0"], s["k1"], s["de1"], s["u1"], s["sf"], W, H, th, nnratio,
                                                     occupied)
        n, m = R.search_by_projection_mappoints(mps, s["de0"], s["k1"], s["de1"], s["u1"], s["sf"], B, th, nnratio, occupied)
        assert n == wn and np.array_equal(m, wm) and n > 100
    if seed == 1:
        mps = _local_map(s, 9, jitter=4.0)
        mps["flags"] |= np.uint32(1)
        mono = np.full(len(s["k1"]), -1, np.float32)
        wn, wm = orbo.search_by_projection_mappoints(mps, s["de0"], s["k1"], s["de1"], mono, s["sf"], W, H, 5.0, 0.8)
        n, m = R.search_by_projection_mappoints(mps, s["de0"], s["k1"], s["de1"], mono, s["sf"], B, 5.0, 0.8)
        assert n == wn and np.array_equal(m, wm)


def _kf_points(s):
    d = np.linalg.norm(s["X"], axis=1).astype(np.float32)
    mx = (np.float32(1.2) * d * s["sf"][s["k0"]["octave"]]).astype(np.float32)
    mn = (np.float32(0.8) * d * s["sf"][s["k0"]["octave"]] / s["sf"][-1]).astype(np.float32)
    return mn, mx


def _kf(s, Tcw, th, orb_dist, flags, mn, mx, check_ori=True, occupied=None, gemm_float=False):
    Ow = (-Tcw[:, :3].T @ Tcw[:, 3]).astype(np.float32)
    a = (Tcw, Ow, (FX, FY, CX, CY), th, orb_dist, LSF, s["k0"], flags, s["X"], mn, mx, s["de0"], s["k1"], s["de1"], s["sf"])
    wn, wm = orbo.search_by_projection_keyframe(*a, W, H, check_ori, occupied, not gemm_float)
    n, m = R.search_by_projection_keyframe(*a, B, check_ori, occupied, not gemm_float)
    assert n == wn and np.array_equal(m, wm)
    return n


def test_keyframe_form_equals_oracle(scene):
    s = scene
    rng = np.random.default_rng(12)
    mn, mx = _kf_points(s)
    T = _shift(s, float(np.median(s["z"][s["has_depth"]])))
    flags = np.ones(len(s["k0"]), np.uint8)
    assert _kf(s, T, 10, 100, flags, mn, mx) > 200
    _kf(s, T, 3, 64, flags, mn, mx)
    _kf(s, T, 10, 100, flags, mn, mx, check_ori=False)
    _kf(s, T, 10, 100, flags, mn, mx, gemm_float=True)
    fl = (rng.random(len(flags)) < 0.6).astype(np.uint8)
    occ = (rng.random(len(s["k1"])) < 0.3).astype(np.uint8)
    _kf(s, T, 10, 100, fl, mn, mx, occupied=occ)
    mx2 = mx.copy()
    mx2[rng.random(len(mx)) < 0.33] *= 0.3
    _kf(s, T, 10, 30, flags, mn, mx2)
    _kf(s, T, 40, 100, flags, mn, mx)
    _kf(s, _pose(tz=-60.0), 10, 100, flags, mn, mx)
    _kf(s, _pose(tx=0.5, yaw=0.1, tz=-3.0), 10, 100, flags, mn, mx)
    _kf(s, T, 20, 80, flags, mn, mx)


def _sim3(s, Tcw, th, ratio, flags, normals, mn, mx, variant=0, matched=None, gemm_float=False):
    Ow = (-Tcw[:, :3].T @ Tcw[:, 3]).astype(np.float32)
    a = (Tcw, Ow, (FX, FY, CX, CY), th, ratio, LSF, flags, s["X"], normals, mn, mx, s["de0"], s["k1"], s["de1"], s["sf"])
    wn, wm = orbo.search_by_projection_sim3(*a, W, H, variant, matched, not gemm_float)
    n, m = R.search_by_projection_sim3(*a, B, variant, matched, not gemm_float)
    assert n == wn and np.array_equal(m, wm)
    return n


def test_sim3_projection_forms_equal_oracle(scene):
    s = scene
    rng = np.random.default_rng(21)
    mn, mx = _kf_points(s)
    X = s["X"]
    normals = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    T = _shift(s, float(np.median(s["z"][s["has_depth"]])))
    flags = np.ones(len(X), np.uint8)
    assert _sim3(s, T, 8, 1.5, flags, normals, mn, mx) > 200
    _sim3(s, T, 8, 1.5, flags, normals, mn, mx, variant=1)
    _sim3(s, T, 3, 1.0, flags, normals, mn, mx)
    _sim3(s, T, 8, 0.45, flags, normals, mn, mx, variant=1)
    _sim3(s, T, 8, 1.5, flags, normals, mn, mx, gemm_float=True)
    fl = (rng.random(len(flags)) < 0.6).astype(np.uint8)
    matched = (rng.random(len(s["k1"])) < 0.3).astype(np.uint8)
    _sim3(s, T, 8, 1.5, fl, normals, mn, mx, matched=matched)
    nr2 = normals.copy()
    nr2[rng.random(len(X)) < 0.5] *= -1.0
    _sim3(s, T, 8, 1.5, flags, nr2, mn, mx)
    _sim3(s, _pose(tz=-60.0), 8, 1.5, flags, normals, mn, mx)
    _sim3(s, _pose(tx=0.5, yaw=0.1, tz=-3.0), 30, 1.5, flags, normals, mn, mx, variant=1)


def _fuse_points(s, rng, valid_p=0.9):
    k0, z0, sf = s["k0"], s["z0"], s["sf"]
    z = np.where(z0 > 0, z0, 25.0).astype(np.float32)
    X = np.stack([(k0["x"] - CX) / FX * z, (k0["y"] - CY) / FY * z, z], 1).astype(np.float32)
    pts = np.zeros(len(k0), orbo.FUSE_POINT_DTYPE)
    pts["pos"] = X
    d = np.linalg.norm(X, axis=1).astype(np.float32)
    pts["normal"] = X / d[:, None]
    pts["max_distance"] = 1.2 * d * sf[k0["octave"]]
    pts["min_distance"] = 0.8 * d * sf[k0["octave"]] / sf[-1]
    pts["valid"] = (rng.random(len(k0)) < valid_p).astype(np.int32)
    return pts


def _fuse(s, pts, desc, Rcw, tcw, Ow, th, sim3=False, gemm_float=False, u_right=True):
    ur = s["u1"] if u_right else np.full(len(s["k1"]), -1, np.float32)
    a = (pts, desc, s["k1"], s["de1"], ur, s["sf"], s["isig2"], Rcw, tcw, Ow, (FX, FY, CX, CY, BF), th, LSF)
    wi, wd = orbo.fuse_search(*a, W, H, sim3, not gemm_float)
    bi, bd = R.fuse_search(*a, B, sim3, not gemm_float)
    assert np.array_equal(bi, wi) and np.array_equal(bd, wd)
    return bi


def test_fuse_search_equals_oracle(scene):
    s = scene
    rng = np.random.default_rng(8)
    pts = _fuse_points(s, rng)
    zmed = float(np.median(s["z0"][s["z0"] > 0]))
    Rm = np.eye(3, dtype=np.float32)
    t = np.array([3.0 / FX * zmed, 1.0 / FY * zmed, 0.0], np.float32)
    Ow = (-Rm.T @ t).astype(np.float32)
    assert (_fuse(s, pts, s["de0"], Rm, t, Ow, 3.0) >= 0).sum() > 300
    _fuse(s, pts, s["de0"], Rm, t, Ow, 4.0, sim3=True)
    _fuse(s, pts, s["de0"], Rm, t, Ow, 3.0, gemm_float=True)
    _fuse(s, pts, s["de0"], Rm, t, Ow, 3.0, u_right=False)
    c, sn = np.cos(0.15), np.sin(0.15)
    R2 = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], np.float32)
    t2 = np.array([0.4, -0.1, -12.0], np.float32)
    _fuse(s, pts, s["de0"], R2, t2, (-R2.T @ t2).astype(np.float32), 3.0)
    pts2 = pts.copy()
    pts2["normal"][rng.random(len(pts)) < 0.5] *= -1.0
    pts2["max_distance"][rng.random(len(pts)) < 0.33] *= 0.3
    _fuse(s, pts2, s["de0"], Rm, t, Ow, 3.0)
    pts3 = pts[:8].copy()
    pts3["pos"][0] = 0
    pts3["max_distance"][1] = 0
    pts3["min_distance"][2] = 0
    pts3["pos"][3] = np.nan
    pts3["pos"][4, 2] = 0
    pts3["valid"] = 1
    _fuse(s, pts3, s["de0"][:8], Rm, np.zeros(3, np.float32), np.zeros(3, np.float32), 3.0)


def test_search_by_sim3_equals_oracle(scene):
    s = scene
    rng = np.random.default_rng(33)
    sf = s["sf"]
    zmed = float(np.median(s["z0"][s["z0"] > 0]))
    t2w = np.array([3.0 / FX * zmed, 1.0 / FY * zmed, 0.0], np.float32)
    I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)

    def points(k, zdep, Rw, tw):
        z = np.where(zdep > 0, zdep, 25.0).astype(np.float32)
        Xc = np.stack([(k["x"] - CX) / FX * z, (k["y"] - CY) / FY * z, z], 1).astype(np.float32)
        d = np.linalg.norm(Xc, axis=1).astype(np.float32)
        pts = np.zeros(len(k), orbo.FUSE_POINT_DTYPE)
        pts["pos"] = ((Xc - tw) @ Rw).astype(np.float32)
        pts["max_distance"] = np.float32(1.2) * d * sf[k["octave"]]
        pts["min_distance"] = np.float32(0.8) * d * sf[k["octave"]] / sf[-1]
        pts["valid"] = (rng.random(len(k)) < 0.85).astype(np.int32)
        return pts

    p1 = points(s["k0"], s["z0"], I3, z3)
    p2 = points(s["k1"], s["z1"], I3, t2w)
    for s12, th in ((1.0, 7.5), (1.03, 7.5), (0.97, 10.0)):
        _, t12, sR12, sR21, t21 = PC.sim3_transforms(t2w, s12)
        for gf in (False, True):
            a = (p1["valid"], p1["pos"], p1["min_distance"], p1["max_distance"], s["de0"], s["k0"], I3, z3, p2["valid"],
                 p2["pos"], p2["min_distance"], p2["max_distance"], s["de1"], s["k1"], I3, t2w, sR12, t12, sR21, t21,
                 (FX, FY, CX, CY), th, LSF, sf)
            wn, wm = orbo.search_by_sim3(*a, W, H, not gf)
            n, m, _ = R.search_by_sim3(*a, B, not gf)
            assert n == wn and np.array_equal(m, wm), (s12, th, gf)


def test_reference_equals_oracle_on_the_golden_fixture(golden_dir):
    p = np.load(os.path.join(golden_dir, "pipeline_hut_320x240.npz"))
    g = np.load(os.path.join(golden_dir, "tracking_hut_320x240.npz"))
    b = (0, 320, 0, 240)
    kC, dC = g["kC"], g["dC"]
    mono = np.full(len(kC), -1, np.float32)
    sf = orbo.Extractor(500).tables()["scale"]
    T0 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    cam = tuple(float(v) for v in g["cam"])
    for gd in (True, False):
        a = (g["Tcw"], T0, cam, 15, p["kL"], g["flags"], g["x3"], p["dL"], kC, dC, mono, sf)
        wn, wm, wd = orbo.search_by_projection_frame(*a, 320, 240, gemm_double=gd)
        n, m, d = R.search_by_projection_frame(*a, b, gemm_double=gd)
        assert (n, d) == (wn, wd) and np.array_equal(m, wm)
        if gd:
            assert n == int(g["sbp_nmatches"]) and np.array_equal(m, g["sbp_match"])
    wn, wm = orbo.search_by_projection_mappoints(g["mps"], p["dL"], kC, dC, mono, sf, 320, 240, 3.0, 0.8, g["occ"])
    n, m = R.search_by_projection_mappoints(g["mps"], p["dL"], kC, dC, mono, sf, b, 3.0, 0.8, g["occ"])
    assert n == wn == int(g["mp_nmatches"]) and np.array_equal(m, wm) and np.array_equal(m, g["mp_match"])
    # the KeyFrame-side forms on the same real keypoints: the last frame's points as candidate MapPoints
    X = np.asarray(g["x3"], np.float32).reshape(-1, 3)
    ok = (g["flags"] & 1).astype(np.uint8)
    d3 = np.linalg.norm(X, axis=1).astype(np.float32)
    mx = (np.float32(1.2) * d3 * sf[p["kL"]["octave"]]).astype(np.float32)
    mn = (np.float32(0.8) * d3 * sf[p["kL"]["octave"]] / sf[-1]).astype(np.float32)
    with np.errstate(all="ignore"):
        nr = np.nan_to_num(X / d3[:, None]).astype(np.float32)
    T = np.asarray(g["Tcw"], np.float32).reshape(-1)[:12].reshape(3, 4)
    Ow = (-T[:, :3].T @ T[:, 3]).astype(np.float32)
    a = (T, Ow, cam[:4], 10, 100, LSF, p["kL"], ok, X, mn, mx, p["dL"], kC, dC, sf)
    wn, wm = orbo.search_by_projection_keyframe(*a, 320, 240)
    n, m = R.search_by_projection_keyframe(*a, b)
    assert n == wn and np.array_equal(m, wm)
    for variant in (0, 1):
        a = (T, Ow, cam[:4], 8, 1.5, LSF, ok, X, nr, mn, mx, p["dL"], kC, dC, sf)
        wn, wm = orbo.search_by_projection_sim3(*a, 320, 240, variant)
        n, m = R.search_by_projection_sim3(*a, b, variant)
        assert n == wn and np.array_equal(m, wm)
    pts = np.zeros(len(X), orbo.FUSE_POINT_DTYPE)
    pts["pos"], pts["normal"], pts["min_distance"], pts["max_distance"], pts["valid"] = X, nr, mn, mx, ok
    isig2 = orbo.Extractor(500).tables()["inv_sigma2"]
    for sim3 in (False, True):
        a = (pts, p["dL"], kC, dC, mono, sf, isig2, T[:, :3], T[:, 3], Ow, cam[:4] + (0.0,), 3.0, LSF)
        wi, wd = orbo.fuse_search(*a, 320, 240, sim3)
        bi, bd = R.fuse_search(*a, b, sim3)
        assert np.array_equal(bi, wi) and np.array_equal(bd, wd)


@pytest.mark.parametrize("matcher", PC.MATCHERS)
@pytest.mark.parametrize("cam", sorted(PC.SIZES))
def test_the_gpu_inputs_bite(cam, matcher):
    """conditions on the inputs of tests/test_gpu_projection_bounds.py, so that a setter that does nothing cannot pass"""
    c = PC.make_case(cam)
    Wc, Hc = c["W"], c["H"]
    b = c["bounds"]
    assert b[0] < 0 and b[1] > Wc and b[2] < 0 and b[3] > Hc
    s = next(r[1] for r in PC.RUNS if r[0] == matcher)
    stats = {}
    at_float = PC.reference(c, matcher, s, b, stats)
    at_int = PC.reference(c, matcher, s, PC.int_bounds(c))
    assert not PC.same(at_float, at_int)
    uk = c["uk1"]
    kp_out = (uk["x"] < 0) | (uk["x"] > Wc) | (uk["y"] < 0) | (uk["y"] > Hc)
    acc = stats["accepted"]
    assert any((u < 0 or u > Wc or v < 0 or v > Hc) and b[0] <= u <= b[1] and b[2] <= v <= b[3] for u, v, _ in acc)
    assert any(kp_out[i] for _, _, i in acc)


@pytest.mark.parametrize("run", [i for i, (_, s) in enumerate(PC.RUNS) if s.get("band")])
@pytest.mark.parametrize("cam", sorted(PC.SIZES))
def test_band_inputs_tell_keyframe_integer_bounds_from_float(cam, run):
    """KeyFrame::mnMinX.. are `const int` (keyframe.h:255-258): the reference rejects what lies in the fractional bands"""
    c = PC.make_case(cam)
    b = c["bounds"]
    matcher, s = PC.RUNS[run]
    assert matcher in PC.KF_MATCHERS
    stats = {}
    over_float = PC.reference(c, matcher, s, b, stats, kf_truncate=False)
    over_int = PC.reference(c, matcher, s, b)
    acc = stats["accepted"]
    assert any(int(b[1]) <= u < b[1] for u, _, _ in acc) and any(b[0] <= u < int(b[0]) for u, _, _ in acc)
    assert {i for _, _, i in acc} == set(c["band"]["kp"])  # matched to the keypoints they were built for
    assert not PC.same(over_float, over_int)
    n_int = over_int[0] if matcher == "sim3proj" else int((over_int[0] >= 0).sum())
    assert n_int == 0
