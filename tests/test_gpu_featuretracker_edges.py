"""GPU (-m gpu): the Lucas-Kanade tracker on the synthetic edge cases of tests/lk_edge_cases.py -- singular Hessians, inf and
NaN inverses, NaN positions, exits through all four borders, templates at the last fit and the first miss, iteration
exhaustion, thresholds 0 and inf, level ranges other than 0..4, three image shapes -- word for word against the numpy
restatement tests/lk_ref.py after every frame (the `_same` of tests/test_gpu_featuretracker.py: counts, ids, positions,
disparity, the feature table).  tests/test_lk_edge_cases_cpu.py shows on the CPU that every case reaches what it is named for.

Templates and inverse Hessians are read back for the degenerate and the level cases, with ONE rule for NaN:
  * where the patch does not fit, invH[0] is the marker word 0x7fffffff, exactly, on both sides;
  * an arithmetic NaN (0 * inf) must be a NaN on both sides at the same index, and its bits are not compared: x86 produces the
    default NaN 0xffc00000, gfx950 0x7fc00000;
  * every other word, infinities and their signs included, is compared exactly.
Every test builds its own small detector and tracker and closes them."""
import numpy as np
import pytest

import lk_cases as LC
import lk_edge_cases as EC
import lk_ref as lk
import test_gpu_featuretracker as TF
import test_gpu_featuretracker_bundle as TB
from vi_slam_amd.fastgrid import FASTGPU
from vi_slam_amd.featuretracker import FeatureTrackerGPU

pytestmark = pytest.mark.gpu
NAN_WORD = np.uint32(lk.NAN_WORD)


def _detector(shape, border, max_batch=1):
    h, w = shape
    return FASTGPU(w, h, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, border, border, max_batch=max_batch, **LC.FAST)


def _same_invh(got, want, what):
    """the NaN rule of the module docstring on two arrays of words"""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    marker = want == NAN_WORD
    assert np.array_equal(got == NAN_WORD, marker), "%s: marker word" % (what,)
    nan = np.isnan(want.view(np.float32)) & ~marker
    assert np.array_equal(np.isnan(got.view(np.float32)) & ~marker, nan), "%s: arithmetic NaN" % (what,)
    assert np.array_equal(got[~nan], want[~nan]), "%s: words" % (what,)


def _templates(ft, T, camera=0):
    """every live track's template and inverse Hessian on every level in range, through template()"""
    patches, invh = LC.templates(T)
    levels = list(range(T.opt.klt_max_level, T.opt.klt_min_level - 1, -1))
    assert len(T.book.tracks) == len(ft.tracks(camera)) > 0
    for i in range(len(T.book.tracks)):
        for li, level in enumerate(levels):
            ps = T.opt.klt_patch_sizes[level]
            p, h = ft.template(i, level, camera)
            assert np.array_equal(p.ravel(), patches[i, li, :(ps + 2) ** 2]), (camera, i, level)  # no fit: what the buffer held before
            _same_invh(LC.u32(h), invh[i, li], (camera, i, level))
    return invh


def _run(name, templates_after=()):
    """the case on the GPU, compared with the yardstick after every frame; templates_after: the frames (0 = the detection)
    after which the templates are read back too -> the last summary"""
    c = EC.cases()[name]
    seq = EC.frames(name)
    _, _, per_frame = EC.run_ref(name)
    det = _detector(seq[0].shape, c["border"])
    try:
        ft = FeatureTrackerGPU(det, **c["opts"])
        try:
            assert ft.capacity == lk.max_ftr_count(lk.Options(**c["opts"]), det.cells)
            counts, s = [], None
            if templates_after:  # the yardstick once more, in step with the device (run_ref's tracker is at its last frame)
                nc, nr = LC.grid(seq[0])
                T = lk.Tracker(lk.Options(**c["opts"]), LC.ref_detector(c["det"], c["border"]), nc, nr, LC.CELL, LC.CELL)
            for k, img in enumerate(seq):
                counts.append(ft.track(img))
                s = TF._summary(ft, counts)
                TF._same(s, per_frame[k], "%s, frame %d" % (name, k))
                if templates_after:
                    T.track(img)
                    if k in templates_after:
                        _templates(ft, T)
            return s
        finally:
            ft.close()
    finally:
        det.close()


@pytest.mark.parametrize("name", EC.DEGENERATE)
def test_a_degenerate_templates(name):
    """singular Hessians: the level is skipped (arithmetic NaN at invH[0]) or the track dies of a NaN position (inf at invH[0])"""
    s = _run(name, templates_after=(0, 1))
    T = EC.run_ref(name)[0]
    words = LC.u32(T.invh)
    arith = np.isnan(T.invh) & (words != NAN_WORD)
    assert arith.any()
    if name.startswith("edge_h"):
        assert np.isinf(T.invh[:, :, 0]).any() and s["counts"][1, 0] < s["counts"][0, 1]
    else:
        assert arith[[t.buffer_id for t in T.book.tracks]][:, :, 0].any()  # a live track with a skipped level


@pytest.mark.parametrize("name", ["drift_left", "drift_right", "drift_top", "drift_bottom", "drift_patch32"])
def test_b_drift_through_every_border(name):
    s = _run(name)
    assert 0 < s["counts"][-1, 0] < s["counts"][0, 1] and s["life"].max() == len(EC.frames(name)) - 1


@pytest.mark.parametrize("name", EC.FIT)
def test_c_templates_at_the_last_fit_and_the_first_miss(name):
    _run(name, templates_after=(0,))


@pytest.mark.parametrize("name", ["static_zero_threshold", "static_zero_threshold_32"])
def test_d_threshold_zero_exhausts_the_iterations(name):
    s = _run(name)
    assert s["counts"][1, 0] == 0 and s["counts"][1, 1] == s["counts"][0, 1] > 20  # every track dies; detection starts over


def test_e_threshold_inf_converges_at_once():
    s = _run("inf_threshold")
    assert s["counts"][-1, 0] > 30


def test_e_a_faded_frame_uses_up_the_iterations_on_regular_hessians():
    s = _run("faded")
    assert 0 < s["counts"][1, 0] < s["counts"][0, 1] // 2  # some levels converge late, the last one in the 30th iteration


@pytest.mark.parametrize("name", ["drift_last_template", "gain_dimmed_01", "gain_dimmed_11"])
def test_e_template_renewal_and_gain(name):
    s = _run(name, templates_after=(1,) if name == "drift_last_template" else ())
    assert s["counts"][-1, 0] > 20 and s["disparity"].view(np.float32)[0] > 0.5


@pytest.mark.parametrize("name", EC.LEVELS)
def test_f_level_ranges(name):
    s = _run(name, templates_after=(0, 2))
    assert s["counts"][-1, 0] > 20


def test_g_bundle_bottom_exit_above_a_nan_camera():
    """camera 0 leaves through its last row, under which camera 1's first row lies on every level; camera 1's tracks die of NaN"""
    B, per_call, counts = EC.run_bundle_ref()
    seq = EC.bundle_images()
    n_cam = len(seq[0])
    det = _detector(seq[0][0].shape, EC.BUNDLE["border"], n_cam)
    try:
        ft = FeatureTrackerGPU(det, cameras=n_cam, **EC.BUNDLE["opts"])
        try:
            got_counts = []
            for k, imgs in enumerate(seq):
                got = ft.track_bundle(imgs)
                assert got == [tuple(c) for c in counts[k]], "call %d" % k
                got_counts.append(got)
                for cam in range(n_cam):
                    TB._same(TB._summary(ft, [c[cam] for c in got_counts], cam), per_call[k][cam], "call %d, camera %d" % (k, cam))
            for cam in range(n_cam):
                _templates(ft, B.T[cam], cam)
        finally:
            ft.close()
    finally:
        det.close()
