"""Inputs shared by tests/test_projection_bounds_cpu.py and tests/test_gpu_projection_bounds.py: per distorted camera two
consecutive synthetic frames, extracted by the CPU oracle (bit-equal to the device extractor) and undistorted by
undistort_ref (bit-equal to k_undistort_kps), the frame's stereo-less MapPoints at a fixed depth, and the list of matcher
runs.  `reference(case, run, bounds)` evaluates one run with projection_bounds_ref."""
import numpy as np

import projection_bounds_ref as R
import undistort_ref as U
from oracle import orbo
from vi_slam_amd import synth

NF = 1000
# image sizes at which every bound of Frame::ComputeImageBounds lies outside the image (zed0's weak distortion needs the
# wider image for that: at 1280 x 720 its right bound is 1278.6)
SIZES = {"euroc": (1280, 720), "zed0": (1600, 900)}
Z = np.float32(12.0)
LSF = float(np.log(np.float32(1.2)).astype(np.float32))
FUSE_POINT_DTYPE = orbo.FUSE_POINT_DTYPE

_cache = {}


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    Rm = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    return np.hstack([Rm, np.array([[tx], [ty], [tz]], np.float32)]).astype(np.float32)


def make_case(name):
    """-> dict: W, H, K, D, bounds, img0 / img1, k0 / k1 (keypoints_), uk0 / uk1 (ukeypoints_), d0 / d1, world points X of
    frame 0's keypoints (its camera = world), scale tables"""
    if name in _cache:
        return _cache[name]
    W, H = SIZES[name]
    K, D = U.CAMERAS[name]
    img0 = synth.make_stereo_pair(W, H, step=0)[0]
    img1 = synth.make_stereo_pair(W, H, step=1)[0]
    e0, e1 = orbo.Extractor(NF), orbo.Extractor(NF)
    k0, d0, _ = e0.compute(img0)
    k1, d1, _ = e1.compute(img1)
    uk0, uk1 = U.undistort_keypoints(k0, K, D), U.undistort_keypoints(k1, K, D)
    fx, fy, cx, cy = (np.float32(v) for v in K)
    X = np.stack([(uk0["x"] - cx) / fx * Z, (uk0["y"] - cy) / fy * Z, np.full(len(uk0), Z)], 1).astype(np.float32)
    tab = e0.tables()
    sf, isig2 = tab["scale"], tab["inv_sigma2"]
    d = np.linalg.norm(X, axis=1).astype(np.float32)
    c = dict(name=name, W=W, H=H, K=K, D=D, bounds=U.image_bounds(K, D, W, H), img0=img0, img1=img1, k0=k0, k1=k1, uk0=uk0,
             uk1=uk1, d0=d0, d1=d1, X=X, sf=np.asarray(sf, np.float32), isig2=np.asarray(isig2, np.float32),
             mx=(np.float32(1.2) * d * np.asarray(sf, np.float32)[uk0["octave"]]).astype(np.float32),
             mn=(np.float32(0.8) * d * np.asarray(sf, np.float32)[uk0["octave"]] / np.float32(sf[-1])).astype(np.float32),
             normals=(X / d[:, None]).astype(np.float32))
    # the synthetic scene shifts by (+3, +1) px per step
    c["shift"] = pose(tx=3.0 / float(fx) * float(Z), ty=1.0 / float(fy) * float(Z))
    rng = np.random.default_rng(17)
    n = len(uk0)
    mps = np.zeros(n, orbo.MP_TRACK_DTYPE)
    mps["proj_x"] = (uk0["x"] + 3.0 + rng.normal(0, 2.0, n)).astype(np.float32)
    mps["proj_y"] = (uk0["y"] + 1.0 + rng.normal(0, 2.0, n)).astype(np.float32)
    mps["proj_xr"] = -1.0
    mps["view_cos"] = rng.choice(np.array([0.9, 0.9985, 1.0], np.float32), n)
    mps["level"] = np.clip(uk0["octave"] + rng.integers(-1, 2, n), 0, 7)
    mps["flags"] = (rng.random(n) < 0.9).astype(np.uint32) | ((rng.random(n) < 0.9).astype(np.uint32) << 1)
    c["mps"] = mps
    pts = np.zeros(n, FUSE_POINT_DTYPE)
    pts["pos"], pts["normal"], pts["max_distance"], pts["min_distance"] = X, c["normals"], c["mx"], c["mn"]
    pts["valid"] = (rng.random(n) < 0.9).astype(np.int32)
    c["pts"] = pts
    # SearchBySim3: KeyFrame 1 = frame 0 (world), KeyFrame 2 = frame 1 at T2w = [I | t]; its points sit at depth Z too
    t2w = c["shift"][:, 3].copy()
    X2c = np.stack([(uk1["x"] - cx) / fx * Z, (uk1["y"] - cy) / fy * Z, np.full(len(uk1), Z)], 1).astype(np.float32)
    d2 = np.linalg.norm(X2c, axis=1).astype(np.float32)
    p2 = np.zeros(len(uk1), FUSE_POINT_DTYPE)
    p2["pos"] = (X2c - t2w).astype(np.float32)
    p2["max_distance"] = np.float32(1.2) * d2 * c["sf"][uk1["octave"]]
    p2["min_distance"] = np.float32(0.8) * d2 * c["sf"][uk1["octave"]] / c["sf"][-1]
    p2["valid"] = (rng.random(len(uk1)) < 0.9).astype(np.int32)
    c["pts2"], c["t2w"] = p2, t2w
    c["band"] = _band_points(c)
    _cache[name] = c
    return c


def _band_points(c):
    """Two MapPoints for the KeyFrame-side forms whose projections land in the fractional bands of the bounds -- between
    floor(mnMaxX) and mnMaxX, and between mnMinX and ceil(mnMinX) -- where the Frame's float bounds say inside and the
    KeyFrame's integer copies say outside.  Each sits at the height of frame 1's outermost keypoint on that side and carries
    that keypoint's descriptor, so that a wide window (the band runs' th) matches it if it is let through."""
    fx, fy, cx, cy = (np.float32(v) for v in c["K"])
    b, uk1, sf = c["bounds"], c["uk1"], c["sf"]
    t = c["shift"][:, 3]
    js = [int(np.argmax(uk1["x"])), int(np.argmin(uk1["x"]))]
    us = [(float(int(b[1])) + float(b[1])) / 2, (float(int(b[0])) + float(b[0])) / 2]
    pts = np.zeros(2, FUSE_POINT_DTYPE)
    for k, (j, u) in enumerate(zip(js, us)):
        Xc = np.array([(np.float32(u) - cx) / fx * Z, (uk1["y"][j] - cy) / fy * Z, Z], np.float32)
        d = np.float32(np.linalg.norm(Xc))
        pts["pos"][k] = Xc - t
        pts["normal"][k] = Xc / d
        pts["max_distance"][k] = np.float32(1.2) * d * sf[uk1["octave"][j]]
        pts["min_distance"][k] = np.float32(0.8) * d * sf[uk1["octave"][j]] / sf[-1]
        pts["valid"][k] = 1
    return dict(pts=pts, desc=c["d1"][js].copy(), kp=js)


def int_bounds(c):
    return np.array([0, c["W"], 0, c["H"]], np.float32)


def sim3_transforms(t2w, s12=1.0):
    """what FMatcher::SearchBySim3 derives (fmatcher.cpp:2262-2264) -- as vi_slam_amd.FMatcher.SearchBySim3 does"""
    R12 = np.eye(3, dtype=np.float32)
    t12 = (-np.asarray(t2w, np.float32)).astype(np.float32)
    sR12 = (np.float32(s12) * R12).astype(np.float32)
    sR21 = ((1.0 / s12) * R12.T).astype(np.float32)
    t21 = (-(sR21.astype(np.float64) @ t12.astype(np.float64))).astype(np.float32)
    return R12, t12, sR12, sR21, t21


# (matcher, settings): every run of the GPU test; the first run of each matcher is the one whose inputs must bite
RUNS = [
    ("frame", dict(T="shift", th=15, gf=False, ori=True, mono=False)),
    ("frame", dict(T="shift", th=15, gf=True, ori=True, mono=False)),
    ("frame", dict(T="shift", th=30, gf=False, ori=False, mono=False)),
    ("frame", dict(T="fwd", th=15, gf=False, ori=True, mono=False)),
    ("frame", dict(T="bwd", th=15, gf=False, ori=True, mono=False)),
    ("frame", dict(T="fwd", th=15, gf=False, ori=True, mono=True)),
    ("keyframe", dict(th=10, orb=100, gf=False, ori=True)),
    ("keyframe", dict(th=10, orb=100, gf=True, ori=False)),
    ("sim3proj", dict(th=8, ratio=1.5, variant=0, gf=False)),
    ("sim3proj", dict(th=8, ratio=1.5, variant=1, gf=True)),
    ("mappoints", dict(th=3.0, nnratio=0.8)),
    ("fuse", dict(th=3.0, sim3=False, gf=False)),
    ("fuse", dict(th=4.0, sim3=True, gf=True)),
    ("sim3", dict(th=7.5, gf=False)),
    ("sim3", dict(th=7.5, gf=True)),
    # the band points (_band_points) through every KeyFrame-side form, with a window wide enough to reach their keypoints
    ("sim3proj", dict(th=64, ratio=1.5, variant=0, gf=False, band=True)),
    ("sim3proj", dict(th=64, ratio=1.5, variant=1, gf=True, band=True)),
    ("fuse", dict(th=64.0, sim3=True, gf=False, band=True)),
    ("sim3dir", dict(th=64.0, gf=False, band=True)),  # one direction of SearchBySim3 (vslam_fuse_search, sim3 = 2)
]
KF_MATCHERS = ["sim3proj", "fuse", "sim3", "sim3dir"]
MATCHERS = ["frame", "keyframe", "sim3proj", "mappoints", "fuse", "sim3"]
MB = 0.5371  # the stereo baseline bForward / bBackward are tested against (mbf = 0: no mvuRight in these frames)


def frame_pose(c, which):
    return {"shift": c["shift"], "fwd": pose(tz=-1.0), "bwd": pose(tz=1.0)}[which]


def kf_points(c, s):
    """the MapPoints of a KeyFrame-side run: (FUSE_POINT records, descriptors)"""
    return (c["band"]["pts"], c["band"]["desc"]) if s.get("band") else (c["pts"], c["d0"])


def reference(c, matcher, s, bounds, stats=None, occupied=None, kf_truncate=True):
    """one run with projection_bounds_ref -> tuple of result arrays / counts"""
    fx, fy, cx, cy = c["K"]
    n1 = len(c["uk1"])
    mono = np.full(n1, -1, np.float32)
    T0 = pose()
    if matcher == "frame":
        flags = np.full(len(c["uk0"]), 3, np.uint8)
        nm, m, d = R.search_by_projection_frame(frame_pose(c, s["T"]), T0, (fx, fy, cx, cy, 0.0, MB), s["th"], c["uk0"], flags,
                                                c["X"], c["d0"], c["uk1"], c["d1"], mono, c["sf"], bounds, s["mono"],
                                                s["ori"], occupied, not s["gf"], stats)
        return nm, m, d
    Tcw = c["shift"]
    Ow = (-Tcw[:, :3].T @ Tcw[:, 3]).astype(np.float32)
    if matcher == "keyframe":
        flags = np.ones(len(c["uk0"]), np.uint8)
        return R.search_by_projection_keyframe(Tcw, Ow, (fx, fy, cx, cy), s["th"], s["orb"], LSF, c["uk0"], flags, c["X"],
                                               c["mn"], c["mx"], c["d0"], c["uk1"], c["d1"], c["sf"], bounds, s["ori"],
                                               occupied, not s["gf"], stats)
    if matcher == "sim3proj":
        if s.get("band"):
            p, pd = kf_points(c, s)
            return R.search_by_projection_sim3(Tcw, Ow, (fx, fy, cx, cy), s["th"], s["ratio"], LSF, np.ones(len(p), np.uint8),
                                               p["pos"], p["normal"], p["min_distance"], p["max_distance"], pd, c["uk1"],
                                               c["d1"], c["sf"], bounds, s["variant"], None, not s["gf"], stats, kf_truncate)
        flags = np.ones(len(c["uk0"]), np.uint8)
        return R.search_by_projection_sim3(Tcw, Ow, (fx, fy, cx, cy), s["th"], s["ratio"], LSF, flags, c["X"], c["normals"],
                                           c["mn"], c["mx"], c["d0"], c["uk1"], c["d1"], c["sf"], bounds, s["variant"], None,
                                           not s["gf"], stats, kf_truncate)
    if matcher == "mappoints":
        return R.search_by_projection_mappoints(c["mps"], c["d0"], c["uk1"], c["d1"], mono, c["sf"], bounds, s["th"],
                                                s["nnratio"], occupied, stats)
    if matcher == "fuse":
        p, pd = kf_points(c, s)
        return R.fuse_search(p, pd, c["uk1"], c["d1"], mono, c["sf"], c["isig2"], Tcw[:, :3], Tcw[:, 3], Ow,
                             (fx, fy, cx, cy, 0.0), s["th"], LSF, bounds, s["sim3"], not s["gf"], stats, kf_truncate)
    if matcher == "sim3dir":
        I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        p, pd = kf_points(c, s)
        return (R._sim3_direction(p["valid"], p["pos"], p["min_distance"], p["max_distance"], pd, I3, z3, I3, c["t2w"],
                                  (fx, fy, cx, cy), s["th"], LSF, c["uk1"], c["d1"], c["sf"], bounds, not s["gf"], stats,
                                  kf_truncate),)
    if matcher == "sim3":
        I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        _, t12, sR12, sR21, t21 = sim3_transforms(c["t2w"])
        (p1, pd1), p2 = kf_points(c, s), c["pts2"]
        n, m12, (vn1, vn2) = R.search_by_sim3(p1["valid"], p1["pos"], p1["min_distance"], p1["max_distance"], pd1, c["uk0"], I3, z3,
                                     p2["valid"], p2["pos"], p2["min_distance"], p2["max_distance"], c["d1"], c["uk1"], I3,
                                     c["t2w"], sR12, t12, sR21, t21, (fx, fy, cx, cy), s["th"], LSF, c["sf"], bounds,
                                     not s["gf"], stats, kf_truncate)
        return n, m12, vn1, vn2  # the two directions too: the agreement check alone hides most of them
    raise KeyError(matcher)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
