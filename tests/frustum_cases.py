"""Deterministic scenes for the Frame::isInFrustum / SearchLocalPoints tests (tests/test_frustum_cpu.py,
tests/test_gpu_frustum.py, tests/test_cpp_frustum.py, tests/tools/time_local_points.py).

branch_case      every exit of frame.cpp:529-595 and every closed boundary, made exact with an identity pose, a
                 power-of-two focal length with a dyadic principal point and axis-aligned points; the rest of the case
                 under a general rotation
bounds_case      fractional float grid bounds with projections inside the bands between mnMinX and ceil(mnMinX) etc.
rotation_case    general rotation only: float and double accumulation of the Matx product / dot differ on it
hut_scene        the chain: stereo points of tests/golden/tracking_hut_320x240.npz seen from a moved pose and 100 points on
                 the current keypoints' rays, interleaved with points behind the camera, out of range and facing away
big_scene        n points of which a chosen share is in view (compaction geometry, beyond the old cap, over capacity)
"""
import os

import numpy as np

import frustum_ref as FR
from oracle import orbo

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NLEVELS = 8
LSF = F32(orbo.logf(float(F32(1.2))))  # Frame::mfLogScaleFactor = log(mfScaleFactor), scale factor 1.2f
CHUNK = 256  # VSLAM_FRUSTUM_CHUNK
W, H = 640, 480
CAM = (512.0, 512.0, 320.0, 240.0, 40.0)  # u = 512 * x / z + 320: exact for dyadic x / z
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32)


def _pt(pos, normal=None, mn=0.0, mx=1000.0, flags=3):
    p = np.zeros((), FR.MAP_POINT_DTYPE)
    pos = np.asarray(pos, F32)
    p["pos"] = pos
    p["normal"] = pos / F32(max(float(np.linalg.norm(pos)), 1e-6)) if normal is None else np.asarray(normal, F32)
    p["min_dist"], p["max_dist"], p["flags"] = F32(mn), F32(mx), flags
    return p


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, t):
    """-> (Tcw rows [R | t] as float32, Ow = -R^T t in float32 of the rounded entries)"""
    T = np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)]).astype(F32)
    Ow = (-(T[:, :3].astype(np.float64).T @ T[:, 3].astype(np.float64))).astype(F32)
    return T, Ow


def random_points(rng, n, T, Ow, spread=1.6, zr=(-2.0, 9.0)):
    """points in the camera frame of T spread beyond the frustum, behind it included, with a mix of every flag, normals
    around the viewing ray (some facing away) and invariance ranges around the true distance (some missing it)"""
    R, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    z = rng.uniform(zr[0], zr[1], n)
    pc = np.stack([rng.uniform(-spread, spread, n) * np.abs(z), rng.uniform(-spread, spread, n) * np.abs(z), z], 1)
    pw = (pc - t) @ R  # R^T (pc - t)
    pts = np.zeros(n, FR.MAP_POINT_DTYPE)
    pts["pos"] = pw.astype(F32)
    ray = pw - Ow.astype(np.float64)
    dist = np.linalg.norm(ray, axis=1)
    nrm = ray / dist[:, None] + rng.normal(0, 0.7, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[rng.random(n) < 0.15] *= -1
    pts["normal"] = nrm.astype(F32)
    pts["min_dist"] = (dist * rng.uniform(0.3, 1.1, n)).astype(F32)
    pts["max_dist"] = (dist * rng.uniform(0.9, 6.0, n)).astype(F32)
    pts["flags"] = rng.choice([0, 1, 2, 3, 3, 3, 1, 3], n).astype(np.uint32)
    return pts


def branch_case():
    """-> (params dict, points, grid bounds or None, labels: index of the hand-made points by name)"""
    P = FR.params(I34, np.zeros(3), CAM, LSF, (W, H), 0.5)
    hand = [
        ("not_candidate", _pt((0, 0, 2), flags=2)),
        ("behind", _pt((0.1, 0.1, -1))),
        ("z_zero_pos_inf", _pt((1, 1, 0))),    # PcZ == +0, x != 0, y != 0: u = v = +inf, rejected by the bounds
        ("z_zero_neg_inf", _pt((-1, 1, 0))),   # u = -inf
        ("left", _pt((-0.7, 0, 1))),
        ("right", _pt((0.7, 0, 1))),
        ("top", _pt((0, -0.5, 1))),
        ("bottom", _pt((0, 0.5, 1))),
        ("u_eq_min", _pt((-0.625, 0, 1))),     # 512 * -0.625 + 320 == 0
        ("u_eq_max", _pt((0.625, 0, 1))),      # == 640
        ("v_eq_min", _pt((0, -0.46875, 1))),   # 512 * -0.46875 + 240 == 0
        ("v_eq_max", _pt((0, 0.46875, 1))),    # == 480
        ("too_close", _pt((0, 0, 2), mn=3.0)),
        ("too_far", _pt((0, 0, 2), mx=1.0)),
        ("dist_eq_min", _pt((0, 0, 2), mn=2.0, mx=4.0)),
        ("dist_eq_max", _pt((0, 0, 2), mx=2.0)),                      # ratio 1: log 0, level 0
        ("cos_below", _pt((0, 0, 2), normal=(0, 0, 0.25))),
        ("cos_eq_limit", _pt((0, 0, 2), normal=(0, 3, 0.5))),         # (0*0 + 0*3) + 2*0.5 = 1, / 2 = 0.5
        ("level_top", _pt((0, 0, 2), mx=1000.0)),                     # ceil(log(500) / log(1.2)) = 35 -> nlevels - 1
        ("log_ratio_integer", _pt((0, 0, 2), mx=F32(2) * F32(1.2))),  # ratio == 1.2f: logf(1.2f) / LSF == 1 exactly
        ("bounds_pass_then_far", _pt((0.25, 0.125, 4), mx=1.0, flags=1)),
    ]
    labels = {name: i for i, (name, _) in enumerate(hand)}
    rng = np.random.default_rng(20)
    T, Ow = pose(rotation(0.21, -0.34, 0.13), (0.3, -0.2, 0.5))
    return P, np.array([p for _, p in hand], FR.MAP_POINT_DTYPE), None, labels, (T, Ow, rng)


def branch_cases():
    """the two frames of the branch case: the hand-made points under the identity pose, random points under a general one"""
    P, hand, _, labels, (T, Ow, rng) = branch_case()
    Pg = FR.params(T, Ow, CAM, LSF, (W, H), 0.5, far_points=True, th_far_points=6.0)
    general = random_points(rng, 2 * CHUNK + 77, T, Ow)
    return [("identity", P, hand, None, labels), ("general", Pg, general, None, {})]


FRACTIONAL = (-12.6, 652.3, -7.4, 489.7)


def bounds_case():
    """fractional grid bounds: projections inside [mnMinX, ceil(mnMinX)) and (floor(mnMaxX), mnMaxX] are inside, the ones
    just beyond are outside.  u = 512 * x + 320 at z = 1."""
    P = FR.params(I34, np.zeros(3), CAM, LSF, (W, H), 0.5)

    def at(u, v):
        return _pt(((u - 320.0) / 512.0, (v - 240.0) / 512.0, 1.0))

    hand = [("in_min_x_band", at(-12.25, 100)), ("out_min_x", at(-12.75, 100)), ("in_max_x_band", at(652.25, 100)),
            ("out_max_x", at(652.5, 100)), ("in_min_y_band", at(100, -7.25)), ("out_min_y", at(100, -7.5)),
            ("in_max_y_band", at(100, 489.5)), ("out_max_y", at(100, 489.75))]
    labels = {name: i for i, (name, _) in enumerate(hand)}
    rng = np.random.default_rng(21)
    T, Ow = pose(rotation(-0.1, 0.25, -0.3), (-0.4, 0.1, 0.2))
    Pg = FR.params(T, Ow, CAM, LSF, (W, H), 0.5)
    return [("identity", P, np.array([p for _, p in hand], FR.MAP_POINT_DTYPE), FRACTIONAL, labels),
            ("general", Pg, random_points(rng, CHUNK + 45, T, Ow, spread=0.9), FRACTIONAL, {})]


def rotation_case():
    rng = np.random.default_rng(22)
    T, Ow = pose(rotation(0.4, 0.3, -0.2), (0.15, 0.25, -0.1))
    P = FR.params(T, Ow, CAM, LSF, (W, H), 0.5)
    pts = random_points(rng, 400, T, Ow, spread=0.5, zr=(1.0, 9.0))
    pts["flags"] = 3
    return P, pts


# ---------------------------------------------------------------------------------------------- the chain
HUT_W, HUT_H, HUT_NF = 320, 240, 500
_hut = {}


def hut_scene():
    """~800 MapPoints: the last frame's stereo points (world = the last camera's frame) seen from the golden's moved pose and
    100 points the current frame does see, interleaved with 250 points behind the camera, out of range or facing away so
    that kept and dropped points alternate.  Current keypoints / descriptors: the golden's."""
    if _hut:
        return _hut
    g = np.load(os.path.join(GOLDEN, "tracking_hut_320x240.npz"))
    p = np.load(os.path.join(GOLDEN, "pipeline_hut_320x240.npz"))
    kL, dL = p["kL"], p["dL"]
    sf = np.asarray(orbo.Extractor(HUT_NF).tables()["scale"], F32)  # mvScaleFactor: cumulative float products of 1.2f
    x3 = g["x3"].astype(F32)
    n = len(x3)
    real = np.zeros(n, FR.MAP_POINT_DTYPE)
    real["pos"] = x3
    dist = np.linalg.norm(x3.astype(np.float64), axis=1)
    real["normal"] = (x3 / dist[:, None]).astype(F32)
    real["min_dist"] = (0.6 * dist).astype(F32)
    # PredictScale -> octave + 1 (or the top level): the matcher searches levels [octave, octave + 1]
    real["max_dist"] = (F32(1.05) * dist.astype(F32) * sf[kL["octave"]]).astype(F32)
    real["flags"] = (g["flags"] & 1) | (g["flags"] & 2)
    rng = np.random.default_rng(23)
    kC, dC = g["kC"], g["dC"]
    T = g["Tcw"].astype(F32)
    Ow = (-(T[:, :3].astype(np.float64).T @ T[:, 3].astype(np.float64))).astype(F32)
    cam = tuple(float(v) for v in g["cam"][:5])
    # MapPoints the current frame does see (the map's points of older KeyFrames): on the rays of 100 current keypoints at
    # depths of 2..6, descriptors one bit away from the keypoints'
    nt = 100
    seen = rng.permutation(len(kC))[:nt]
    z = rng.uniform(2.0, 6.0, nt)
    pc = np.stack([(kC["x"][seen] - cam[2]) / cam[0] * z, (kC["y"][seen] - cam[3]) / cam[1] * z, z], 1)
    pw = (pc - T[:, 3].astype(np.float64)) @ T[:, :3].astype(np.float64)
    tracked = np.zeros(nt, FR.MAP_POINT_DTYPE)
    tracked["pos"] = pw.astype(F32)
    ray = pw - Ow.astype(np.float64)
    td = np.linalg.norm(ray, axis=1)
    tracked["normal"] = (ray / td[:, None]).astype(F32)
    tracked["min_dist"] = (0.6 * td).astype(F32)
    tracked["max_dist"] = (F32(1.05) * td.astype(F32) * sf[kC["octave"][seen]]).astype(F32)
    tracked["flags"] = np.where(np.arange(nt) % 4 == 0, 1, 3)
    tdesc = dC[seen].copy()
    tdesc[np.arange(nt), np.arange(nt) % 32] ^= np.uint8(1)
    m = 250
    junk = real[rng.integers(0, n, m)].copy()
    kind = np.arange(m) % 3
    junk["pos"][kind == 0, 2] *= -1                      # behind the camera
    junk["max_dist"][kind == 1] *= F32(0.3)              # out of the scale-invariance range
    junk["normal"][kind == 2] *= -1                      # facing away
    junk["flags"] = 3
    jdesc = rng.integers(0, 256, (m, 32)).astype(np.uint8)
    gdesc = np.concatenate([dL, tdesc])
    gorder = np.random.default_rng(26).permutation(n + nt)
    good, gdesc = np.concatenate([real, tracked])[gorder], gdesc[gorder]
    ng = n + nt
    order = np.argsort(np.concatenate([np.arange(ng) * 2, np.arange(m) * 2 * ng // m + 1]), kind="stable")
    pts = np.concatenate([good, junk])[order]
    desc = np.concatenate([gdesc, jdesc])[order]
    _hut.update(C=g["C"], kC=kC, dC=dC, pts=pts, desc=desc, T=T, Ow=Ow, cam=cam, sf=sf, n_real=n)
    ur = np.full(len(kC), -1, F32)
    half = seen[::2]
    ur[half] = (kC["x"][half] - F32(cam[4]) / z[::2].astype(F32)).astype(F32)  # mvuRight consistent with the tracked points
    occ = (np.random.default_rng(24).random(len(kC)) < 0.15).astype(np.uint8)
    _hut.update(u_right=ur, occupied=occ)
    return _hut


def hut_params(far):
    s = hut_scene()
    return dict(Tcw=s["T"], Ow=s["Ow"], cam=s["cam"], log_scale_factor=LSF, img_size=(HUT_W, HUT_H),
                viewing_cos_limit=0.5, far_points=far, th_far_points=HUT_TH_FAR)


HUT_TH_FAR = 4.5
#: the runs of the chain test: (far_points, th, with u_right / occupied)
HUT_RUNS = [(False, 1.0, False), (True, 1.0, False), (False, 3.0, True), (True, 3.0, True), (True, 3.0, False)]


def big_scene(n, keep_mask, seed=25):
    """n MapPoints on the hut keypoints' rays: keep_mask[i] puts point i in view (identity pose), the others behind the
    camera.  Descriptors cycle through the golden's current descriptors so that kept points do find matches."""
    s = hut_scene()
    kC, dC = s["kC"], s["dC"]
    rng = np.random.default_rng(seed)
    idx = np.arange(n) % len(kC)
    z = rng.uniform(2.0, 6.0, n).astype(F32)
    fx, fy, cx, cy = s["cam"][:4]
    pos = np.stack([(kC["x"][idx] - F32(cx)) / F32(fx) * z, (kC["y"][idx] - F32(cy)) / F32(fy) * z, z], 1).astype(F32)
    pos += rng.normal(0, 0.002, pos.shape).astype(F32)
    keep = np.asarray(keep_mask, bool)
    pos[~keep, 2] *= -1
    pts = np.zeros(n, FR.MAP_POINT_DTYPE)
    pts["pos"] = pos
    d = np.linalg.norm(pos.astype(np.float64), axis=1)
    nrm = pos / d[:, None]
    nrm[~keep] *= -1  # keeps z positive in the normal: irrelevant, the depth test rejects them first
    pts["normal"] = nrm.astype(F32)
    pts["min_dist"] = (0.5 * d).astype(F32)
    pts["max_dist"] = (F32(1.05) * d.astype(F32) * s["sf"][np.minimum(kC["octave"][idx], NLEVELS - 1)]).astype(F32)
    pts["flags"] = np.where(rng.random(n) < 0.8, 3, 1).astype(np.uint32)
    desc = dC[idx].copy()
    flip = rng.integers(0, 256, n)
    desc[np.arange(n), flip % 32] ^= (1 << (flip // 32)).astype(np.uint8)  # one bit off each: distinct but close
    P = dict(Tcw=I34, Ow=np.zeros(3, F32), cam=s["cam"], log_scale_factor=LSF, img_size=(HUT_W, HUT_H),
             viewing_cos_limit=0.5, far_points=False, th_far_points=0.0)
    return P, pts, desc
