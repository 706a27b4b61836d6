"""GPU (-m gpu): vilib::FeatureTrackerGPU over a FrameBundle -- several cameras per tracker object, every step of track()
enqueued once for the bundle (vslam_ft_create_bundle / vslam_ft_track_bundle) -- word for word against the bundle yardstick
tests/lk_bundle_ref.py (C unmodified lk_ref.Tracker objects and one id counter) on the cases of tests/lk_bundle_cases.py."""
import ctypes as C

import numpy as np
import pytest

import lk_bundle_cases as BC
import lk_cases as LC
import lk_ref as lk
import vi_slam_amd as V
from vi_slam_amd.fastgrid import FASTGPU
from vi_slam_amd.featuretracker import FtFeature, FeatureTrackerGPU
from vi_slam_amd.harrisgrid import HarrisGPU

pytestmark = pytest.mark.gpu
FIELDS = ("counts", "track_id", "buffer_id", "life", "first_pos", "cur_pos", "cur_disparity", "f_track_id", "f_level", "f_score", "f_px",
          "disparity")  # the field list of test_gpu_featuretracker._same


def _detector(kind, shape, max_batch):
    h, w = shape
    if kind == "fast":
        return FASTGPU(w, h, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, max_batch=max_batch, **LC.FAST)
    return HarrisGPU(w, h, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, max_batch=max_batch, **LC.HARRIS)


def _summary(ft, counts, camera=0):
    t, f = ft.tracks(camera), ft.features(camera)
    return dict(counts=np.array(counts, np.int32).reshape(-1, 2), first_pos=LC.u32(t["first_pos"]), cur_pos=LC.u32(t["cur_pos"]),
                cur_disparity=LC.u32(t["cur_disparity"]), life=t["life"], track_id=t["track_id"], buffer_id=t["buffer_id"],
                f_px=LC.u32(f["px"]), f_score=LC.u32(f["score"]), f_level=f["level"], f_track_id=f["track_id"],
                disparity=LC.u32(np.array([ft.getDisparity(0.5, camera)], np.float32)))


def _same(got, want, what, fields=FIELDS):
    assert sorted(got) == sorted(want)
    for k in fields:
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


def _run(name, feed=None, max_batch=None):
    """the case on the GPU, every camera compared with the yardstick after every call -> (tracker, detector, per call the
    per-camera summaries)"""
    kind, opts, idx = BC.CASES[name]
    seq = BC.images(name)
    n_cam = len(idx)
    _, per_call, counts = BC.run_ref(name)
    det = _detector(kind, seq[0][0].shape, max_batch or n_cam)
    ft = FeatureTrackerGPU(det, cameras=n_cam, **opts)
    assert ft.cameras == n_cam and ft.capacity == lk.max_ftr_count(lk.Options(**opts), det.cells)
    got_counts, out = [], []
    for k, imgs in enumerate(seq):
        got = feed(ft, imgs) if feed else ft.track_bundle(imgs)
        assert got == [tuple(c) for c in counts[k]], "%s, call %d" % (name, k)  # n_tracked[], n_detected[]
        got_counts.append(got)
        out.append([_summary(ft, [c[cam] for c in got_counts], cam) for cam in range(n_cam)])
        for cam in range(n_cam):
            _same(out[k][cam], per_call[k][cam], "%s, call %d, camera %d" % (name, k, cam))
    return ft, det, out


def _templates(ft, T, camera):
    patches, invh = LC.templates(T)
    levels = list(range(T.opt.klt_max_level, T.opt.klt_min_level - 1, -1))
    assert len(T.book.tracks) == len(ft.tracks(camera)) > 0
    for i in range(len(T.book.tracks)):
        for li, level in enumerate(levels):
            ps = T.opt.klt_patch_sizes[level]
            p, h = ft.template(i, level, camera)
            assert np.array_equal(p.ravel(), patches[i, li, :(ps + 2) ** 2]), (camera, i, level)
            assert np.array_equal(LC.u32(h), invh[i, li]), (camera, i, level)  # a patch that did not fit: what the buffer held before


def test_a_four_cameras_one_of_them_blank():
    ft, det, _ = _run("four")
    try:
        B = BC.run_ref("four")[0]
        for cam in (0, 2):
            _templates(ft, B.T[cam], cam)
    finally:
        ft.close()
        det.close()


def test_b_two_cameras_with_the_last_observation_as_template():
    ft, det, _ = _run("two_last")
    try:
        B = BC.run_ref("two_last")[0]
        for cam in (0, 1):
            _templates(ft, B.T[cam], cam)
    finally:
        ft.close()
        det.close()


def test_c_device_pointers_a_pitch_of_its_own_and_unused_slots():
    import torch

    def feed(ft, imgs):
        h, w = imgs[0].shape
        d = torch.zeros((len(imgs), h, w + 64), dtype=torch.uint8, device="cuda")  # a pitch of its own
        d[:, :, :w] = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda()
        torch.cuda.synchronize()
        return ft.track_bundle(dev_ptrs=[d[i].data_ptr() for i in range(len(imgs))], pitch=d.stride(1))

    ft, det, dev = _run("four", feed, max_batch=6)  # two image slots of every level stay unused
    ft.close()
    det.close()
    ft, det, host = _run("four")
    ft.close()
    det.close()
    for k in range(BC.N_CALLS):
        for cam in range(4):
            _same(dev[k][cam], host[k][cam], "call %d, camera %d" % (k, cam))


def test_d_a_bundle_of_one_is_the_single_camera_tracker():
    kind, opts, get = LC.cases()["step"]
    seq = get()
    z = np.load(LC.GOLD + "/lk_hut_long.npz")
    gold = {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith("step__")}
    for single in (False, True):
        det = _detector(kind, seq[0].shape, 1)
        ft = FeatureTrackerGPU(det, cameras=1, **opts)
        try:
            counts = [ft.track(img) if single else ft.track_bundle([img])[0] for img in seq]  # vslam_ft_track works on it too
            _same(_summary(ft, counts), gold, "golden, vslam_ft_track" if single else "golden, vslam_ft_track_bundle")
        finally:
            ft.close()
            det.close()


def test_e_a_bundle_against_lone_trackers():
    name = "two_last"
    kind, opts, idx = BC.CASES[name]
    ft, det, out = _run(name)
    ft.close()
    det.close()
    fields = tuple(f for f in FIELDS if f not in ("track_id", "f_track_id"))
    for cam in range(len(idx)):
        seq = BC.camera_frames(name, cam)
        det = _detector(kind, seq[0].shape, 1)
        ft = FeatureTrackerGPU(det, **opts)
        try:
            counts = []
            for k, img in enumerate(seq):
                counts.append(ft.track(img))
                _same(_summary(ft, counts), out[k][cam], "call %d, camera %d" % (k, cam), fields)
        finally:
            ft.close()
            det.close()


def test_f_rejections():
    det = _detector("harris", (256, 384), 2)
    try:
        for n in (0, 3):  # below one camera, above the detector's max_batch
            with pytest.raises(V.VslamError) as ei:
                FeatureTrackerGPU(det, cameras=n, **LC.TEST_OPTS)
            assert ei.value.code == V.ERR_INVALID, n
        ft = FeatureTrackerGPU(det, cameras=2, **LC.TEST_OPTS)
        try:
            with pytest.raises(V.VslamError) as ei:
                ft.track(LC.frames()[0])  # vslam_ft_track on a bundle of two
            assert ei.value.code == V.ERR_INVALID
            out, n = np.zeros(ft.capacity, np.dtype([("w", np.uint32, C.sizeof(FtFeature) // 4)])), C.c_int()
            for cam in (-1, 2):  # a camera out of range on the read side
                for call in (lambda: ft.tracks(cam), lambda: ft.features(cam), lambda: ft.getDisparity(0.5, cam), lambda: ft.template(0, 0, cam)):
                    with pytest.raises(V.VslamError) as ei:
                        call()
                    assert ei.value.code == V.ERR_INVALID, cam
            assert ft.L.vslam_ft_features_cam(ft._h, 2, out.ctypes.data_as(C.c_void_p), ft.capacity, C.byref(n)) == V.ERR_INVALID
            assert len(ft.tracks(1)) == 0 and ft.track_bundle([LC.frames()[0], LC.frames()[1]]) == [(0, 50), (0, 50)]
        finally:
            ft.close()
    finally:
        det.close()
