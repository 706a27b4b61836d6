"""GPU (-m gpu): nothing is left behind.  Every case reads vslam_dbg_live_memory -- the library's own count of the device
and pinned bytes and blocks its objects hold -- creates, uses and destroys, and finds all four counters exactly where
they were.  (The device's free-memory figure cannot show that on a GPU that other processes use too.)"""
import ctypes as C
import gc

import numpy as np
import pytest

import vi_slam_amd as V
from vi_slam_amd import synth
from vi_slam_amd.fastgrid import FASTGPU
from vi_slam_amd.featuretracker import FeatureTrackerGPU

pytestmark = pytest.mark.gpu

W, H, NF, NL, B = 160, 120, 200, 3, 2


def live():
    """(device bytes, device blocks, pinned bytes, pinned blocks)"""
    v = [C.c_ulonglong() for _ in range(4)]
    assert V.lib().vslam_dbg_live_memory(*[C.byref(x) for x in v]) == V.VSLAM_OK
    return tuple(x.value for x in v)


@pytest.fixture
def base():
    gc.collect()  # an object of an earlier test that is collected later would lower the counters under a case
    return live()


def _dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def _context(**tuning):
    # h2d_route=2: the DMA transport for every batch size, so that two images reach the device staging (d_stage) too
    return V.FExtractor(NF, 1.2, NL, 20, 7, W, H, max_batch=B, tuning=dict(tuning, h2d_route=2))


def test_a_context_through_every_grow_on_demand_path(base):
    rng = np.random.default_rng(5)
    L, R = synth.make_stereo_pair(W, H, seed=11)
    fe = _context()
    try:
        created = live()
        assert all(c > b for c, b in zip(created, base))  # the counters count
        # 1. host images: pinned staging, device staging, the captured graph (second pass replays it)
        res = fe.compute_batch([L, R])
        res = fe.compute_batch([L, R])
        assert len(res[0][0]) > 20 and len(res[1][0]) > 20
        assert live()[0] > created[0] and live()[2] > created[2]
        # 2. a colour format and back: the gray staging is released and allocated again on first use
        fe.set_pixel_format(V.PIX_BGR8)
        bgr = [np.repeat(im[:, :, None], 3, axis=2) for im in (L, R)]
        assert len(fe.compute_batch(bgr)[0][0]) > 20
        fe.set_pixel_format(V.PIX_GRAY8)
        res = fe.compute_batch([L, R])
        # 3. the device SearchForInitialization with more pairs than image slots: the matcher's own output pair
        p, c = fe.slot_dev_ptrs(0), fe.slot_dev_ptrs(1)
        m = V.FMatcher(fe, 0.9, True)
        m.search_init_dev_async([(p[0], p[1], p[2], c[0], c[1], c[2], 0), (c[0], c[1], c[2], p[0], p[1], p[2], 0),
                                 (p[0], p[1], p[2], c[0], c[1], c[2], 0)], 100)
        out = m.search_init_dev_wait([len(res[0][0]), len(res[1][0]), len(res[0][0])])
        assert out[0][0] == out[2][0] and np.array_equal(out[0][1], out[2][1])
        # 4. the brute-force matcher's scratch grows
        q = _dev(rng.integers(0, 256, (500, 32), dtype=np.uint8))
        t = _dev(rng.integers(0, 256, (60, 32), dtype=np.uint8))
        for rows in (50, 500):
            before = live()
            idx, dist = m.hamming_top2_batch([(q.data_ptr(), rows, t.data_ptr(), 60)])[0]
            assert idx.shape == (rows, 2) and (idx >= 0).all()
            assert live()[0] > before[0] and live()[2] > before[2]
        # 5. stereo scratch and the stereo points
        u, dep = V.ComputeStereoMatches(fe, 0, fe, 1, 40.0, 100.0)
        assert len(u) == len(res[0][0])
        before = live()
        Twc = [np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)]
        fe.stereo_points_async(Twc, (W / 2.0, H / 2.0, 0.01, 0.01))
        assert live()[1] == before[1] + 2
        # 6. a distorted camera: the undistorted keypoints
        before = live()
        fe.set_camera(100.0, 100.0, W / 2.0, H / 2.0, dist=[-0.28, 0.07, 0.0002, 0.00002])
        assert live()[1] == before[1] + 1
        fe.compute_batch([L, R])
    finally:
        fe.close()  # 7.
    del q, t
    assert live() == base


def test_the_quadtree_debug_stamps_go_with_the_context(base):
    """vslam_tuning.oct_debug = 1 allocates 512 bytes of stamps: before the owning buffers nothing freed them"""
    fe = _context(oct_debug=1)
    with_stamps = live()
    fe.close()
    assert live() == base
    fe = _context()
    without = live()
    fe.close()
    assert with_stamps[0] == without[0] + 512 and with_stamps[1] == without[1] + 1
    assert live() == base


def test_a_create_that_fails_after_it_has_allocated(base):
    """60 x 60, 2 levels at 1.2: every level is at least 40 px but no 30-px FAST cell fits: create_fast refuses, behind
    the pyramids and resize tables of the two steps before it"""
    with pytest.raises(V.VslamError) as ei:
        V.FExtractor(NF, 1.2, 2, 20, 7, 60, 60, max_batch=B)
    assert ei.value.code == V.ERR_UNSUPPORTED and "no 30-px FAST cell" in str(ei.value)
    assert live() == base


def test_a_grid_detector_and_a_two_camera_tracker(base):
    frames = [synth.make_frame(128, 64, seed=3, step=s) for s in range(4)]
    det = FASTGPU(128, 64, max_level=2, max_batch=2)
    try:
        with_det = live()
        assert all(c > b for c, b in zip(with_det, base))
        ft = FeatureTrackerGPU(det, cameras=2, klt_max_level=2, klt_patch_sizes=(16, 16, 8, 8, 8), pyramid_levels=3,
                               min_tracks_to_detect_new_features=4)
        try:
            assert all(c > b for c, b in zip(live(), with_det))
            first = ft.track_bundle(frames[0:2])
            ft.track_bundle(frames[2:4])
            assert all(d > 0 for _, d in first)
        finally:
            ft.close()
        assert live() == with_det
    finally:
        det.close()
    assert live() == base


def test_a_vocabulary(base):
    voc = V.Vocabulary(synth.make_vocabulary(6, 3))
    assert live()[1] == base[1] + 6 and live()[0] > base[0]
    voc.close()
    assert live() == base


def test_a_keyframe_database_that_grows_and_compacts(base):
    rng = np.random.default_rng(9)
    db = V.KeyFrameDatabase(500, initial_entries=64)
    try:
        assert live()[1] == base[1] + 2  # the pool pair; the slot table comes with the first query
        for k in range(6):  # 6 x 50 entries into a pool of 64: it doubles three times
            ids = np.sort(rng.choice(500, 50, replace=False)).astype(np.int32)
            db.add(k, 0, (ids, np.full(50, 0.02)))
        assert live()[1] == base[1] + 2
        for k in range(4):  # more than half of the entries die: the pool is compacted
            db.erase(k)
        db.add(10, 0, (np.arange(20, dtype=np.int32), np.full(20, 0.05)))
        st = db.stats()
        assert st["growths"] >= 2 and st["compactions"] >= 1 and st["used"] == 120
        assert live()[1] == base[1] + 2
    finally:
        db.close()
    assert live() == base
