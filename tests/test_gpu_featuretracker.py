"""GPU (-m gpu): the pyramidal Lucas-Kanade feature tracker (vilib::FeatureTrackerGPU) through the C ABI of
include/vslam_featuretracker.h, word for word against the numpy restatement tests/lk_ref.py (itself pinned by
tests/test_lk_cpu.py) and the committed golden file, on the 384x256 crops of the reference's hut_long sequence
(12 x 8 cells of 32 x 32)."""
import numpy as np
import pytest

import lk_cases as LC
import lk_ref as lk
import vi_slam_amd as V
from vi_slam_amd.fastgrid import FASTGPU
from vi_slam_amd.featuretracker import FeatureTrackerGPU
from vi_slam_amd.harrisgrid import HarrisGPU

pytestmark = pytest.mark.gpu
NAN_WORD = np.uint32(lk.NAN_WORD)


def _detector(kind, shape, max_batch=1):
    h, w = shape
    if kind == "fast":
        return FASTGPU(w, h, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, max_batch=max_batch, **LC.FAST)
    return HarrisGPU(w, h, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, max_batch=max_batch, **LC.HARRIS)


def _summary(ft, counts):
    t, f = ft.tracks(), ft.features()
    return dict(counts=np.array(counts, np.int32).reshape(-1, 2), first_pos=LC.u32(t["first_pos"]), cur_pos=LC.u32(t["cur_pos"]),
                cur_disparity=LC.u32(t["cur_disparity"]), life=t["life"], track_id=t["track_id"], buffer_id=t["buffer_id"],
                f_px=LC.u32(f["px"]), f_score=LC.u32(f["score"]), f_level=f["level"], f_track_id=f["track_id"],
                disparity=LC.u32(np.array([ft.getDisparity(0.5)], np.float32)))


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in ("counts", "track_id", "buffer_id", "life", "first_pos", "cur_pos", "cur_disparity", "f_track_id", "f_level", "f_score", "f_px",
              "disparity"):
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


def _run(name, feed=None, max_batch=1):
    """the case on the GPU, compared with the yardstick after every frame -> (tracker, detector, last summary)"""
    kind, opts, get = LC.cases()[name]
    seq = get()
    _, _, per_frame = LC.run_ref(name)
    det = _detector(kind, seq[0].shape, max_batch)
    ft = FeatureTrackerGPU(det, **opts)
    assert ft.capacity == lk.max_ftr_count(lk.Options(**opts), det.cells)
    counts, s = [], None
    for k, img in enumerate(seq):
        counts.append(feed(ft, img) if feed else ft.track(img))
        s = _summary(ft, counts)
        _same(s, per_frame[k], "%s, frame %d" % (name, k))
    return ft, det, s


def _golden(name):
    z = np.load(LC.GOLD + "/lk_hut_long.npz")
    return {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(name + "__")}


def test_a_templates_and_inverse_hessians_alone():
    ft, det, _ = _run("precompute")
    try:
        T, _, _ = LC.run_ref("precompute")
        patches, invh = LC.templates(T)
        gold = _golden("precompute")
        assert np.array_equal(patches, gold["patches"]) and np.array_equal(invh, gold["invh"])
        n, levels = len(T.book.tracks), range(4, -1, -1)
        assert n == len(ft.tracks()) > 60
        for i in range(n):
            for li, level in enumerate(levels):
                ps = T.opt.klt_patch_sizes[level]
                p, h = ft.template(i, level)
                assert np.array_equal(p.ravel(), patches[i, li, :(ps + 2) ** 2]), (i, level)
                assert np.array_equal(LC.u32(h), invh[i, li]), (i, level)
        missing = (invh[:, :, 0] == NAN_WORD).sum(0)
        assert missing[0] > 10 and missing[-1] == 0 and 0 < missing.sum() < invh.shape[0] * invh.shape[1] // 2  # border points: no coarse patch
    finally:
        ft.close()
        det.close()


def test_b_one_tracking_step_with_the_reference_tests_options():
    ft, det, s = _run("step")
    try:
        _same(s, {k: v for k, v in _golden("step").items()}, "golden")
        T = LC.run_ref("step")[0]
        assert s["counts"].tolist() == [[0, 50], [len(T.book.tracks), 0]] and 25 < len(T.book.tracks) < 50  # some died, most did not
        assert list(s["track_id"]) == sorted(s["track_id"]) and len(s["f_px"]) == len(T.book.tracks)
    finally:
        ft.close()
        det.close()


@pytest.mark.parametrize("name", ["seq_harris", "seq_last_template", "seq_reset"])
def test_c_sequence_with_redetection(name):
    ft, det, s = _run(name)
    try:
        _same(s, _golden(name), "golden")
        T = LC.run_ref(name)[0]
        c = s["counts"]
        if name == "seq_reset":
            assert (c[2:, 1] > 0).any() and (c[c[:, 1] > 0][1:, 0] == 0).all()  # a detection drops every track
            assert (s["life"] <= 1).all()
        else:
            assert T.redetected >= 1 and ((c[1:, 0] > 0) & (c[1:, 1] > 0)).any()  # detection with occupied cells happened
            assert s["life"].max() == 4 and s["life"].min() == 0 and s["disparity"].view(np.float32)[0] > 5.0
        assert len(set(s["track_id"])) == len(s["track_id"]) and len(set(s["buffer_id"])) == len(s["buffer_id"])
    finally:
        ft.close()
        det.close()


def test_d_the_four_affine_variants_on_a_dimmed_frame():
    conv = {}
    for name in ("affine_00", "affine_10", "affine_01", "affine_11"):
        ft, det, s = _run(name)
        ft.close()
        det.close()
        _same(s, _golden(name), "golden")
        conv[name] = int(s["counts"][1, 0])
    assert conv["affine_11"] >= conv["affine_00"] > 10


def test_e_patch_size_32_and_an_idle_half_wave():
    ft, det, s = _run("patch32_odd")
    try:
        _same(s, _golden("patch32_odd"), "golden")
        T = LC.run_ref("patch32_odd")[0]
        assert s["counts"][0, 1] % 2 == 1                                   # the last wave of both kernels has one idle half
        assert any(it > 0 for _, _, it in T.trace)                          # a position left the image after an update
    finally:
        ft.close()
        det.close()


def test_f_device_pointer_and_host_memory_give_the_same_words():
    import torch

    def feed(ft, img):
        h, w = img.shape
        d = torch.zeros((h, w + 64), dtype=torch.uint8, device="cuda")  # a pitch of its own
        d[:, :w] = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        torch.cuda.synchronize()
        return ft.track(dev_ptr=d.data_ptr(), pitch=d.stride(0))

    ft, det, s = _run("step", feed, max_batch=3)  # and a detector whose own pyramid holds three images per level
    ft.close()
    det.close()
    _same(s, _golden("step"), "golden")


def test_create_rejects_what_the_reference_asserts():
    det = _detector("fast", (256, 384))
    try:
        for bad in (dict(klt_max_level=0), dict(klt_patch_sizes=(16, 16, 12, 8, 8)), dict(klt_patch_sizes=(64, 16, 16, 8, 8)),
                    dict(pyramid_levels=4), dict(pyramid_levels=9), dict(klt_min_level=-1), dict(klt_max_level=8, pyramid_levels=8),
                    dict(min_tracks_to_detect_new_features=1, use_best_n_features=1)):
            with pytest.raises(V.VslamError) as ei:
                FeatureTrackerGPU(det, **dict(LC.TEST_OPTS, **bad))
            assert ei.value.code == V.ERR_INVALID, bad
    finally:
        det.close()
    det = _detector("fast", (248, 392))  # 392 = 8 * 49: no multiple of 2^(5-1)
    try:
        with pytest.raises(V.VslamError) as ei:
            FeatureTrackerGPU(det, **LC.TEST_OPTS)
        assert ei.value.code == V.ERR_INVALID
        FeatureTrackerGPU(det, **dict(LC.TEST_OPTS, klt_max_level=3, pyramid_levels=4)).close()
    finally:
        det.close()
