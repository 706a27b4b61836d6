"""CPU: distorted pinhole cameras.  The shared undistortion arithmetic (vi_slam_amd/csrc/vslam_undistort.h, host build in
libvslam_host.so) against the numpy restatement of cv::undistortPoints (tests/undistort_ref.py), the restatement
against the radtan forward model, and SearchForInitialization over float grid bounds: the Python restatement pinned to
the oracle at {0, W, 0, H}, the host replay equal to it at the fractional bounds of a distorted camera."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref as U
import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

W, H = 1280, 720


@pytest.fixture(scope="module")
def HL():
    L = C.CDLL(V.HOST_LIB_PATH)
    vp = C.c_void_p
    L.vslamh_undistort_points.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.vslamh_image_bounds.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.vslamh_search_init_bounds.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_undistort(HL, cam, pts):
    K, D = cam
    k = np.asarray(K, np.float32)
    d = np.asarray(D, np.float32)
    xy = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    out = np.zeros_like(xy)
    assert HL.vslamh_undistort_points(_p(k), _p(d), len(d), _p(xy), len(xy), _p(out)) == 0
    return out


def _points(seed=7):
    """a 1280 x 720 lattice (corners and borders included) plus random points, some far off the image"""
    gx, gy = np.meshgrid(np.linspace(0, W, 65), np.linspace(0, H, 37))
    lattice = np.stack([gx.ravel(), gy.ravel()], 1)
    rng = np.random.default_rng(seed)
    inside = rng.uniform((0, 0), (W, H), (3000, 2))
    outside = rng.uniform((-400, -300), (W + 400, H + 300), (1000, 2))
    return np.concatenate([lattice, inside, outside]).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(U.CAMERAS))
def test_host_build_equals_restatement(HL, name):
    cam = U.CAMERAS[name]
    pts = _points()
    got = _host_undistort(HL, cam, pts)
    want = U.frame_undistort(pts, *cam)
    assert np.array_equal(_bits(got), _bits(want)), name
    if name == "k1_zero":  # the reference tests k1 only: p1, p2 != 0 change nothing
        assert np.array_equal(_bits(got), _bits(pts))
    else:
        assert np.abs(got - pts).max() > 0.5
    b = np.zeros(4, np.float32)
    K, D = np.asarray(cam[0], np.float32), np.asarray(cam[1], np.float32)
    assert HL.vslamh_image_bounds(_p(K), _p(D), len(D), W, H, _p(b)) == 0
    assert np.array_equal(_bits(b), _bits(U.image_bounds(*cam, W, H)))


def test_icdist_fallback_is_exercised():
    """the NEG_ICDIST set takes OpenCV's icdist < 0 exit on far points: they come back at their input position"""
    K, D = U.NEG_ICDIST
    far = np.array([[0, 0], [W, H], [-300, 900]], np.float32)
    out = U.undistort_points(far, K, D)
    assert np.allclose(out, far, atol=1e-3)
    near = np.array([[650, 370]], np.float32)
    assert not np.array_equal(U.undistort_points(near, K, D), near)


@pytest.mark.parametrize("name,r2_max", [("zed0", None), ("zed1", None), ("euroc", 0.2)])
def test_restatement_round_trips_through_the_distortion_model(name, r2_max):
    """Distorting the undistorted point gives the point back (a mis-transcribed formula would not).  OpenCV's five
    fixed-point iterations converge over the whole image for the weak ZED lenses; at EuRoC strength (k1 = -0.28) they
    only do so near the centre (normalised r^2 < 0.2) -- towards the corners the reference's ukeypoints_ are off by up to
    ~0.4 px, and so, bit for bit, are this project's."""
    K, D = U.CAMERAS[name]
    rng = np.random.default_rng(11)
    pts = rng.uniform((0, 0), (W, H), (4000, 2)).astype(np.float32)
    if r2_max is not None:
        r2 = ((pts[:, 0] - K[2]) / K[0]) ** 2 + ((pts[:, 1] - K[3]) / K[1]) ** 2
        pts = pts[r2 < r2_max]
        assert len(pts) > 500
    und = U.undistort_points(pts, K, D)
    back = U.distort_points(und, K, D)
    assert np.abs(back - pts).max() < 1e-3


@pytest.fixture(scope="module")
def frames():
    e = orbo.Extractor(1000)
    k1, d1, _ = e.compute(synth.make_frame(W, H, step=0))
    k2, d2, _ = e.compute(synth.make_frame(W, H, step=1))
    return k1, d1, k2, d2


def test_python_matcher_equals_oracle_at_integer_bounds(frames):
    k1, d1, k2, d2 = frames
    for window, ratio, ori in [(100, 0.9, True), (30, 0.9, False)]:
        nm_o, m_o, pm_o = orbo.search_for_initialization(k1, d1, k2, d2, W, H, window=window, nnratio=ratio,
                                                         check_ori=ori)
        nm, m, pm = U.search_for_initialization(k1, d1, k2, d2, (0, W, 0, H), window=window, nnratio=ratio,
                                                check_ori=ori)
        assert nm == nm_o and np.array_equal(m, m_o) and np.array_equal(pm, pm_o.reshape(-1, 2))
        assert nm > 20


@pytest.mark.parametrize("name", ["euroc", "zed0"])
def test_host_replay_equals_restatement_at_fractional_bounds(HL, frames, name):
    K, D = U.CAMERAS[name]
    k1, d1, k2, d2 = frames
    u1, u2 = U.undistort_keypoints(k1, K, D), U.undistort_keypoints(k2, K, D)
    b = U.image_bounds(K, D, W, H)
    assert b[0] != 0 and b[1] != W  # really fractional
    dm = np.minimum(U.hamming(d1, d2), 255).astype(np.uint8)
    for window, ratio, ori in [(100, 0.9, 1), (40, 0.7, 0)]:
        nm_r, m_r, pm_r = U.search_for_initialization(u1, d1, u2, d2, b, window=window, nnratio=ratio,
                                                      check_ori=bool(ori))
        pm = np.stack([u1["x"], u1["y"]], 1).astype(np.float32).copy()
        m = np.zeros(len(u1), np.int32)
        nm = HL.vslamh_search_init_bounds(_p(u1), len(u1), _p(u2), len(u2), _p(dm), _p(b), _p(pm), _p(m), window,
                                          ratio, ori)
        assert nm == nm_r and np.array_equal(m, m_r) and np.array_equal(_bits(pm), _bits(pm_r))
        assert nm > 20
