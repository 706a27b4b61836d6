"""Deterministic inputs of the fisheye (KannalaBrandt8) tests: tests/test_kb8_cpu.py, tests/test_gpu_kb8.py,
tests/test_cpp_kb8.py, tests/tools/time_kb8.py.

cameras          TUM (a TUM-VI-like calibration: 512 x 512, fx ~ 190, k of mixed sign), ZERO (the same with k = 0), STRONG (a
                 strongly distorting lens), and two precision variants whose Newton loops run longer
libm_edges       arguments on both sides of every branch boundary of the libm restatements, zeros, subnormals, inf, NaN
libm_sample      fixed-seed samples, 2 M and more per function
project_points   all four quadrants of psi, theta from 0 to beyond 90 degrees (z <= 0, z = +0), x = 1 exactly, y = +-0, x = +-0,
                 |y / x| beyond 2^+-60, subnormals
unproject_pixels the principal point (theta_d <= 1e-8), the whole image, pixels beyond the clamp of theta_d
frustum_scene    MapPoints around a fisheye Frame: every exit of Frame::isInFrustum
rig_scene        the same for a two-camera rig whose cameras look 50 degrees apart
local_scene      about 700 MapPoints against the hut frame of tests/frustum_cases.py: points on the rays of its keypoints
"""
import numpy as np

import frustum_cases as FC
import frustum_ref as FR
import kb8_ref as KR

F32, U32 = np.float32, np.uint32
W = H = 512
K_TUM = (0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673)
K_STRONG = (-0.08, 0.02, -0.006, 0.0008)
#: name -> (fx, fy, cx, cy, k, precision)
CAMERAS = {
    "tum": (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, K_TUM, 0.0),
    "zero": (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, (0, 0, 0, 0), 0.0),
    "strong": (200.0, 199.5, 256.25, 255.5, K_STRONG, 0.0),
    "strong_fine": (200.0, 199.5, 256.25, 255.5, K_STRONG, 1e-7),
    "strong_finest": (200.0, 199.5, 256.25, 255.5, K_STRONG, 1e-30),
}


def camera(name):
    return KR.camera(*CAMERAS[name])


def _around(bits_list):
    """b - 1, b, b + 1 of every bit pattern, both signs"""
    u = np.array([b + d for b in bits_list for d in (-1, 0, 1) if 0 <= b + d < 0x80000000], np.int64)
    u = np.unique(np.concatenate([u, u | 0x80000000]))
    return u.astype(U32).view(F32)


_COMMON = [0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x7f7fffff, 0x7f800000, 0x7fc00000]
#: the ix boundaries of the restatements: s_atanf.c, k_tanf.c / s_tanf.c (and floats next to pi/2), s_sincosf.h (and pi)
ATAN_BOUNDS = [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000]
TAN_BOUNDS = [0x39000000, 0x3f2ca140, 0x3f490fda, 0x3fc90fdb, 0x4016cbe4]
SINCOS_BOUNDS = [0x39800000, 0x3f400000, 0x3fc90fdb, 0x40490fdb]


def libm_edges(fn):
    """-> (a,) or (y, x) float32 arrays"""
    if fn == "atanf":
        return (_around(_COMMON + ATAN_BOUNDS),)
    if fn == "tanf":
        return (_around(_COMMON + TAN_BOUNDS),)
    if fn in ("sinf", "cosf"):
        return (_around(_COMMON + SINCOS_BOUNDS),)
    assert fn == "atan2f"
    vals = np.concatenate([_around(_COMMON + ATAN_BOUNDS), np.array([2.0 ** 60, 2.0 ** 61, 2.0 ** 62, 2.0 ** -60, 2.0 ** -61,
                                                                      2.0 ** -62, 2.0, -2.0, 0.5, 1e-40, -1e-40], F32)])
    y, x = np.meshgrid(vals, vals)
    return y.reshape(-1).astype(F32), x.reshape(-1).astype(F32)


LIBM_SAMPLE = 1 << 21  # per half


def libm_sample(fn):
    """fixed seed; per function two halves of 2^21 arguments"""
    rng = np.random.default_rng({"atanf": 1, "tanf": 2, "sinf": 3, "cosf": 4, "atan2f": 5}[fn])
    n = LIBM_SAMPLE
    raw = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32).view(F32)  # noqa: E731
    if fn == "atanf":  # raw bit patterns | the range project feeds it
        return (np.concatenate([raw(), rng.uniform(-4, 4, n).astype(F32)]),)
    if fn == "tanf":  # |x| < 3*pi/4 | dense around pi/2
        return (np.concatenate([rng.uniform(-2.356, 2.356, n).astype(F32), rng.uniform(1.3, 1.8, n).astype(F32)]),)
    if fn in ("sinf", "cosf"):  # [-pi, pi] | raw patterns of small magnitude
        small = (rng.integers(0, 0x40490fdb, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << 31))
        return (np.concatenate([rng.uniform(-np.pi, np.pi, n).astype(F32), small.astype(U32).view(F32)]),)
    return (np.concatenate([raw(), rng.uniform(-10, 10, n).astype(F32)]),
            np.concatenate([raw(), rng.uniform(-10, 10, n).astype(F32)]))


def project_points():
    """n x 3 float32 (n ~ 4300: the GPU test slices 1, 63, 64, 65 and 4099 of them; the hand-made ones come first)"""
    hand = []
    for z in (2.0, 1.0, 0.25, 0.0, -0.25, -3.0):          # theta from small to beyond 90 degrees; z = +0
        for x, y in ((0.7, 0.4), (-0.7, 0.4), (-0.7, -0.4), (0.7, -0.4), (1.0, 0.3), (1.0, -2.0), (0.3, 0.0), (0.3, -0.0),
                     (-0.3, 0.0), (-0.3, -0.0), (0.0, 0.6), (-0.0, 0.6), (0.0, -0.6), (-0.0, -0.6), (0.0, 0.0), (-0.0, -0.0)):
            hand.append((x, y, z))
    big, small = 2.0 ** 62, 2.0 ** -62
    hand += [(2.0, big, 1.0), (2.0, -big, 1.0), (-2.0, big, 1.0), (big, 2.0, 1.0), (-big, 2.0, 1.0), (-big, -2.0, 1.0),
             (small, 0.5, 1.0), (0.5, small, 1.0), (-0.5, small, 1.0), (1e-40, 1e-42, 1.0), (1e-42, -1e-40, 1e-41),
             (1e-20, 1e-20, 1.0), (0.3, 0.3, 2.0 ** 62), (0.3, 0.3, -2.0 ** 62), (3e19, 3e19, 1.0)]
    # |y / x| on both sides of every reduction boundary of atanf, both signs of x
    for b in ATAN_BOUNDS[:5]:
        for d in (-1, 0, 1):
            q = float(np.array([b + d], U32).view(F32)[0])
            hand += [(1.0, q, 1.0), (-2.0, 2.0 * q, 0.5), (0.5, -0.5 * q, -1.0)]
    rng = np.random.default_rng(40)
    n = 4300 - len(hand)
    z = rng.uniform(-1.0, 4.0, n)
    rnd = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), z], 1)
    return np.concatenate([np.array(hand, np.float64), rnd]).astype(F32)


def unproject_pixels(name):
    """n x 2 float32 (n ~ 4300) for camera `name`: the principal point and its neighbours first"""
    fx, fy, cx, cy = (F32(v) for v in CAMERAS[name][:4])
    hand = [(cx, cy), (np.nextafter(cx, F32(1e9)), cy), (cx, np.nextafter(cy, F32(-1e9))), (cx + F32(1e-3), cy),
            (0.0, 0.0), (511.0, 511.0), (0.0, 511.0), (-200.0, 256.0), (256.0, 900.0), (1e6, -1e6), (cx + F32(0.5), cy - F32(0.25))]
    # a radial line from the strong lens' principal point: with precision 1e-7 its Newton loop leaves after 8 steps at the
    # first three radii and after 9 at the last two (found by scanning the line; nine steps are rare: a pixel either converges
    # within eight or oscillates in the last bit until the tenth)
    r = np.linspace(0.0, 330.0, 200001)[[145638, 148365, 159755, 173189, 180721]]
    hand += list(zip(256.25 + r * 0.8, 255.5 + r * 0.6))
    g = np.linspace(0.0, 511.0, 60)
    gx, gy = np.meshgrid(g, g)
    rng = np.random.default_rng(41)
    n = 4300 - len(hand) - gx.size
    rnd = np.stack([rng.uniform(-40, 552, n), rng.uniform(-40, 552, n)], 1)
    return np.concatenate([np.array(hand, np.float64), np.stack([gx.ravel(), gy.ravel()], 1), rnd]).astype(F32)


# ---------------------------------------------------------------------------------------------- frustum
MBF = 19.3


def _params(T, Ow, name, far=False, th_far=0.0):
    fx, fy, cx, cy = CAMERAS[name][:4]
    return FR.params(T, Ow, (fx, fy, cx, cy, MBF), FC.LSF, (W, H), 0.5, far_points=far, th_far_points=th_far)


def frustum_scene(n=4099, seed=42):
    """-> (params, camera, points): points spread over more than the fisheye's field of view"""
    rng = np.random.default_rng(seed)
    T, Ow = FC.pose(FC.rotation(0.21, -0.34, 0.13), (0.3, -0.2, 0.5))
    pts = FC.random_points(rng, n, T, Ow, spread=5.0, zr=(-1.5, 9.0))
    return _params(T, Ow, "tum", far=True, th_far=12.0), camera("tum"), pts


def rig():
    """the right camera 10 cm to the right, looking 50 degrees away from the left one"""
    Rlr = FC.rotation(0.02, 0.87, -0.01)  # right camera's axes in the left camera's frame
    tlr = np.array([0.101, 0.002, -0.004])
    Tlr = np.hstack([Rlr, tlr.reshape(3, 1)]).astype(F32)
    R = Tlr[:, :3].astype(np.float64)
    Trl = np.hstack([R.T, (-R.T @ Tlr[:, 3].astype(np.float64)).reshape(3, 1)]).astype(F32)
    return dict(cam2=camera("strong"), Tlr=Tlr, Trl=Trl)


def rig_scene(n=4099, seed=42):
    P, cam, pts = frustum_scene(n, seed)
    return P, cam, rig(), pts


# ---------------------------------------------------------------------------------------------- SearchLocalPoints
#: the hut frame is 320 x 240; a fisheye of that size
LOCAL_CAM = (118.0, 118.5, 159.5, 120.25, K_TUM, 0.0)
_local = {}


def local_scene():
    """MapPoints on the fisheye rays of the hut frame's keypoints (descriptors one bit off the keypoints'), interleaved with
    200 random points, seen from a general pose -> dict(P, cam, pts, desc, and the hut scene's kC, dC, sf, C)"""
    if _local:
        return _local
    s = FC.hut_scene()
    kC, dC = s["kC"], s["dC"]
    cam = KR.camera(*LOCAL_CAM)
    rng = np.random.default_rng(44)
    T, Ow = FC.pose(FC.rotation(-0.12, 0.2, 0.05), (0.2, -0.1, 0.3))
    nk = len(kC)
    rays, _, _ = KR.unproject(cam, np.stack([kC["x"], kC["y"]], 1))
    z = rng.uniform(2.0, 6.0, nk)
    pc = rays.astype(np.float64) * z[:, None]
    pw = (pc - T[:, 3].astype(np.float64)) @ T[:, :3].astype(np.float64)
    on = np.zeros(nk, FR.MAP_POINT_DTYPE)
    on["pos"] = pw.astype(F32)
    ray = pw - Ow.astype(np.float64)
    d = np.linalg.norm(ray, axis=1)
    on["normal"] = (ray / d[:, None]).astype(F32)
    on["min_dist"] = (0.6 * d).astype(F32)
    on["max_dist"] = (F32(1.05) * d.astype(F32) * s["sf"][kC["octave"]]).astype(F32)
    on["flags"] = np.where(np.arange(nk) % 4 == 0, 1, 3)
    odesc = dC.copy()
    odesc[np.arange(nk), np.arange(nk) % 32] ^= np.uint8(1)
    m = 270
    junk = FC.random_points(rng, m, T, Ow, spread=2.6, zr=(-1.5, 9.0))
    jdesc = rng.integers(0, 256, (m, 32)).astype(np.uint8)
    order = rng.permutation(nk + m)
    fx, fy, cx, cy = LOCAL_CAM[:4]
    P = FR.params(T, Ow, (fx, fy, cx, cy, MBF), FC.LSF, (FC.HUT_W, FC.HUT_H), 0.5, far_points=True, th_far_points=5.5)
    _local.update(P=P, cam=cam, cam_tuple=LOCAL_CAM, pts=np.concatenate([on, junk])[order],
                  desc=np.concatenate([odesc, jdesc])[order], kC=kC, dC=dC, sf=s["sf"], C=s["C"])
    return _local
