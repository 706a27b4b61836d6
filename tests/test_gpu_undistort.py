"""GPU: distorted pinhole cameras (vslam_fe_set_camera).  Every pass of a context with a camera writes the slots'
ukeypoints_ with k_undistort_kps; they must equal the numpy restatement of cv::undistortPoints (tests/undistort_ref.py)
of the slot's own keypoints bit for bit, on every extraction path, through graph replays and camera changes.  The
mono initialisation (SearchForInitialization on ukeypoints_ over ComputeImageBounds' float bounds) must equal the
restatement of the reference's matcher, in the host-keypoint and the device-resident forms."""

import numpy as np
import pytest
import torch

import undistort_ref as U
import vi_slam_amd as V
from vi_slam_amd import synth

pytestmark = pytest.mark.gpu

W, H, NF = 1280, 720, 1000


def _fe(max_batch=1, flags=0):
    return V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=max_batch, flags=flags)


def _set(fe, cam):
    K, D = cam
    fe.set_camera(*K, dist=D)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_ukps(kps, ukps, cam, what):
    """ukps == the restatement of kps: x, y bit-exact, every other field identical"""
    want = U.undistort_keypoints(kps, *cam)
    assert len(ukps) == len(kps) > 100, what
    assert np.array_equal(_bits(ukps["x"]), _bits(want["x"])), what
    assert np.array_equal(_bits(ukps["y"]), _bits(want["y"])), what
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(ukps[f].view(np.uint32), kps[f].view(np.uint32)), (what, f)
    if np.float32(cam[1][0]) != 0:
        assert np.abs(ukps["x"] - kps["x"]).max() > 0.5, what


def _dev(img):
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def test_compute_and_batch_write_undistorted_keypoints():
    fe = _fe(max_batch=8)
    try:
        _set(fe, U.ZED_CAM0)
        img = synth.make_frame(W, H, step=0)
        k, _, _ = fe.compute(img)
        _check_ukps(k, fe.ukeypoints(0), U.ZED_CAM0, "compute")
        _set(fe, U.EUROC_LIKE)
        frames = [synth.make_frame(W, H, seed=5, step=s) for s in range(8)]
        res = fe.compute_batch(frames)
        for s in range(8):
            _check_ukps(res[s][0], fe.ukeypoints(s), U.EUROC_LIKE, ("batch", s))
    finally:
        fe.close()


def test_frame_stereo_async_writes_undistorted_keypoints():
    fe = _fe(max_batch=4)
    try:
        _set(fe, U.ZED_CAM1)
        pairs = [synth.make_stereo_pair(W, H, step=s) for s in range(2)]
        dev = [_dev(im) for p in pairs for im in p]
        torch.cuda.synchronize()
        fe.frame_stereo_async([t.data_ptr() for t in dev], W, 386.1448, 718.856)
        feats, _ = fe.frame_stereo_wait()
        feats = [(k.copy(), d.copy()) for k, d in feats]
        for s in range(4):
            _check_ukps(feats[s][0], fe.ukeypoints(s), U.ZED_CAM1, ("stereo", s))
    finally:
        fe.close()


def test_host_quadtree_path_writes_undistorted_keypoints():
    fe = _fe(max_batch=2, flags=V.FLAG_HOST_OCTREE)
    try:
        _set(fe, U.WITH_K3)
        res = fe.compute_batch([synth.make_frame(W, H, step=s) for s in range(2)])
        for s in range(2):
            _check_ukps(res[s][0], fe.ukeypoints(s), U.WITH_K3, ("host quadtree", s))
    finally:
        fe.close()


def test_graph_replay_and_camera_change():
    """host-image passes replay a captured graph: the replay includes the undistortion, and a camera change drops the
    graph so that the next pass does not reuse the old coefficients"""
    fe = _fe(max_batch=2)
    try:
        frames = [synth.make_frame(W, H, step=s) for s in range(2)]
        _set(fe, U.ZED_CAM0)
        for rep in range(2):  # rep 0 captures, rep 1 replays
            res = fe.compute_batch(frames)
            for s in range(2):
                _check_ukps(res[s][0], fe.ukeypoints(s), U.ZED_CAM0, ("rep", rep, s))
        _set(fe, U.EUROC_LIKE)
        for rep in range(2):
            res = fe.compute_batch(frames)
            for s in range(2):
                _check_ukps(res[s][0], fe.ukeypoints(s), U.EUROC_LIKE, ("new camera", rep, s))
    finally:
        fe.close()


def test_k1_zero_no_camera_and_unchanged_extraction():
    fe, plain = _fe(), _fe()
    try:
        img = synth.make_frame(W, H, step=0)
        want_k, want_d, want_m = plain.compute(img)
        _set(fe, U.K1_ZERO)  # k1 == 0: ukeypoints_ = keypoints_ (frame.cpp:762-766), no launch
        k, d, m = fe.compute(img)
        assert fe.slot_ukps_ptr(0) == fe.slot_buffers(0)[0]
        assert np.array_equal(fe.ukeypoints(0).view(np.uint8), k.view(np.uint8))
        assert np.array_equal(fe.image_bounds(), np.float32([0, W, 0, H]))
        _set(fe, U.EUROC_LIKE)
        k2, d2, m2 = fe.compute(img)
        for got in ((k, d, m), (k2, d2, m2)):  # a camera changes nothing of the extraction itself
            assert np.array_equal(got[0].view(np.uint8), want_k.view(np.uint8))
            assert np.array_equal(got[1], want_d) and got[2] == want_m
        assert fe.slot_ukps_ptr(0) != fe.slot_buffers(0)[0]
        fe.set_camera(None)
        for call in (lambda: fe.ukeypoints(0), lambda: fe.slot_ukps_ptr(0),
                     lambda: V.undistort_points(fe, [[1.0, 2.0]])):
            with pytest.raises(V.VslamError) as ei:
                call()
            assert ei.value.code == V.ERR_INVALID
        k3, d3, m3 = fe.compute(img)
        assert np.array_equal(k3.view(np.uint8), want_k.view(np.uint8)) and np.array_equal(d3, want_d)
        assert np.array_equal(fe.image_bounds(), np.float32([0, W, 0, H]))
    finally:
        fe.close()
        plain.close()


def test_image_bounds_and_undistort_points():
    fe = _fe()
    try:
        assert np.array_equal(fe.image_bounds(), np.float32([0, W, 0, H]))
        rng = np.random.default_rng(2)
        pts = np.concatenate([rng.uniform((0, 0), (W, H), (2000, 2)),
                              rng.uniform((-400, -300), (W + 400, H + 300), (500, 2))]).astype(np.float32)
        for name in ("zed0", "zed1", "euroc", "k3", "neg_icdist", "k1_zero"):
            cam = U.CAMERAS[name]
            _set(fe, cam)
            assert np.array_equal(_bits(fe.image_bounds()), _bits(U.image_bounds(*cam, W, H))), name
            assert np.array_equal(_bits(V.undistort_points(fe, pts)), _bits(U.frame_undistort(pts, *cam))), name
        _set(fe, U.ZED_CAM0)
        b = fe.image_bounds()
        assert b[0] != 0 and b[1] != W and b[2] != 0 and b[3] != H
    finally:
        fe.close()


def _job(fe, s1, s2, dev_kps1, dev_kps2):
    p, c = fe.slot_dev_ptrs(s1), fe.slot_dev_ptrs(s2)
    return (dev_kps1, p[1], p[2], dev_kps2, c[1], c[2], 0)


@pytest.mark.parametrize("name", ["euroc", "zed0"])
def test_mono_initialisation_on_a_distorted_camera(name):
    cam = U.CAMERAS[name]
    frames = [synth.make_frame(W, H, step=s) for s in range(2)]
    fe = _fe(max_batch=2)
    pin = V.PinnedImages(2, H, W, W)
    try:
        _set(fe, cam)
        res = fe.compute_batch(frames)
        k = [res[s][0] for s in range(2)]
        d = [res[s][1] for s in range(2)]
        u = [fe.ukeypoints(s) for s in range(2)]
        b = fe.image_bounds()
        assert np.array_equal(_bits(b), _bits(U.image_bounds(*cam, W, H)))
        m = V.FMatcher(fe, 0.9, True)
        for window in (100, 30):
            wn, wm, wp = U.search_for_initialization(u[0], d[0], u[1], d[1], b, window=window, nnratio=0.9)
            assert wn > 20
            pm0 = np.stack([u[0]["x"], u[0]["y"]], 1).astype(np.float32)
            # host-keypoint form
            nm, mm, pm = m.SearchForInitialization(u[0], fe.slot_buffers(0)[1], u[1], fe.slot_buffers(1)[1], pm0,
                                                   windowSize=window, bounds=b)
            assert nm == wn and np.array_equal(mm, wm) and np.array_equal(_bits(pm), _bits(wp)), window
            (bn, bm, bp), = m.SearchForInitializationBatch(
                [(u[0], fe.slot_buffers(0)[1], u[1], fe.slot_buffers(1)[1], pm0)], windowSize=window, bounds=b)
            assert bn == wn and np.array_equal(bm, wm) and np.array_equal(_bits(bp), _bits(wp)), window
            # device-resident form on the slots' ukeypoints_, dev_prev_matched = NULL
            m.search_init_dev_async([_job(fe, 0, 1, fe.slot_ukps_ptr(0), fe.slot_ukps_ptr(1))], window, bounds=b)
            (dn, dm, dp), = m.search_init_dev_wait([len(u[0])], want_prev=True)
            assert dn == wn and np.array_equal(dm, wm) and np.array_equal(_bits(dp), _bits(wp)), window
            # integer bounds: the _ex forms equal the old entry points
            old = m.SearchForInitialization(k[0], fe.slot_buffers(0)[1], k[1], fe.slot_buffers(1)[1],
                                            np.stack([k[0]["x"], k[0]["y"]], 1), windowSize=window)
            new = m.SearchForInitialization(k[0], fe.slot_buffers(0)[1], k[1], fe.slot_buffers(1)[1],
                                            np.stack([k[0]["x"], k[0]["y"]], 1), windowSize=window,
                                            bounds=(0, W, 0, H))
            assert old[0] == new[0] and np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2])
            dj = [_job(fe, 0, 1, fe.slot_buffers(0)[0], fe.slot_buffers(1)[0])]
            m.search_init_dev_async(dj, window)
            o = m.search_init_dev_wait([len(k[0])], want_prev=True)[0]
            o = (o[0], o[1].copy(), o[2].copy())
            m.search_init_dev_async(dj, window, bounds=(0, W, 0, H))
            n_ = m.search_init_dev_wait([len(k[0])], want_prev=True)[0]
            assert o[0] == n_[0] and np.array_equal(o[1], n_[1]) and np.array_equal(o[2], n_[2])
        # deferred delivery (want_host = 2): extraction + matcher on ukeypoints_ leave in ONE transfer
        for s in range(2):
            pin.array[s][:] = frames[s]
        wn, wm, wp = U.search_for_initialization(u[0], d[0], u[1], d[1], b, window=100, nnratio=0.9)
        for rep in range(2):  # capture, then replay
            sent0 = fe.delivery_stats()
            fe.compute_batch_async(pin.ptrs, W, to_host="with_matcher", where=V.IMGS_PINNED)
            m.search_init_dev_async([_job(fe, 0, 1, fe.slot_ukps_ptr(0), fe.slot_ukps_ptr(1))], 100, bounds=b)
            got = fe.wait(copy=True)
            assert fe.delivery_stats()[0] - sent0[0] == 1, rep
            for s in range(2):
                assert np.array_equal(got[s][0].view(np.uint8), k[s].view(np.uint8)), (rep, s)
            (dn, dm, dp), = m.search_init_dev_wait([len(u[0])], want_prev=True)
            assert dn == wn and np.array_equal(dm, wm) and np.array_equal(_bits(dp), _bits(wp)), rep
            _check_ukps(k[0], fe.ukeypoints(0), cam, ("deferred", rep))
    finally:
        pin.close()
        fe.close()


def test_rescan_and_host_replay_paths_use_the_float_bounds():
    """a one-entry sorted prefix (init_topm = 1) forces k_si_replay's full re-scan of a query's window; init_match_host = 1
    takes the host replay (FrameGrid over the float bounds) -- both must equal the restatement at fractional bounds"""
    cam = U.EUROC_LIKE
    frames = [synth.make_frame(W, H, step=s) for s in range(2)]
    for tuning in ({"init_topm": 1}, {"init_match_host": 1}):
        fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2, tuning=tuning)
        try:
            _set(fe, cam)
            res = fe.compute_batch(frames)
            d = [res[s][1] for s in range(2)]
            u = [fe.ukeypoints(s) for s in range(2)]
            b = fe.image_bounds()
            wn, wm, wp = U.search_for_initialization(u[0], d[0], u[1], d[1], b, window=100, nnratio=0.9)
            m = V.FMatcher(fe, 0.9, True)
            m.search_init_fallbacks()
            pm0 = np.stack([u[0]["x"], u[0]["y"]], 1).astype(np.float32)
            nm, mm, pm = m.SearchForInitialization(u[0], fe.slot_buffers(0)[1], u[1], fe.slot_buffers(1)[1], pm0,
                                                   windowSize=100, bounds=b)
            assert nm == wn and np.array_equal(mm, wm) and np.array_equal(_bits(pm), _bits(wp)), tuning
            if "init_topm" in tuning:
                assert m.search_init_fallbacks() > 0
                m.search_init_dev_async([_job(fe, 0, 1, fe.slot_ukps_ptr(0), fe.slot_ukps_ptr(1))], 100, bounds=b)
                (dn, dm, dp), = m.search_init_dev_wait([len(u[0])], want_prev=True)
                assert dn == wn and np.array_equal(dm, wm) and np.array_equal(_bits(dp), _bits(wp))
        finally:
            fe.close()


def test_ex_entry_points_reject_bad_bounds():
    fe = _fe()
    try:
        m = V.FMatcher(fe, 0.9, True)
        k = np.zeros(1, V.KP_DTYPE)
        for bad in ((0, 0, 0, H), (0, W, H, H), (float("nan"), W, 0, H), (0, float("inf"), 0, H)):
            with pytest.raises(V.VslamError) as ei:
                m.SearchForInitialization(k, 0, k, 0, np.zeros((1, 2), np.float32), bounds=bad)
            assert ei.value.code == V.ERR_INVALID
        with pytest.raises(V.VslamError):
            fe.set_camera(600.0, 600.0, 640.0, 360.0, dist=(0.1, 0.0, 0.0))  # 3 coefficients
    finally:
        fe.close()
