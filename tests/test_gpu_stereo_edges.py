"""GPU (-m gpu): ComputeStereoMatches on the scenes of stereo_edge_cases.py -- the zero-disparity clamp whose result
survives the outlier cut, the `disparity < maxD` edge and the minU gate, a row bucket of more than 64 candidates --
through every entry point, mvuRight / mvDepth compared with the oracle as uint32 words.  Each test first asserts on the
oracle's result that the scene takes the branch it is for (the same checks as test_edge_scene_preconditions_cpu.py)."""
import numpy as np
import pytest

import stereo_edge_cases as SC
import vi_slam_amd as V
from conftest import kp_equal

pytestmark = pytest.mark.gpu

CASES = [(s, bf, fx) for s in SC.A_SEEDS for bf, fx in SC.A_CAMERAS]


@pytest.fixture(scope="module")
def scenes():
    """images and oracle results of scene A per (seed, bf, fx), and of the ordinary pair per camera; computed once"""
    out = {}
    img = {s: SC.scene_a(s) for s in SC.A_SEEDS}
    for s, bf, fx in CASES:
        ref = SC.oracle_stereo(img[s][0], img[s][1], SC.A_NF, bf, fx)
        SC.check_scene_a(ref, bf, fx)
        out[(s, bf, fx)] = (img[s], ref)
    o = SC.ordinary_pair()
    for bf, fx in SC.A_CAMERAS:
        out[("ordinary", bf, fx)] = (o, SC.oracle_stereo(o[0], o[1], SC.A_NF, bf, fx))
    return out


@pytest.fixture(scope="module")
def fe():
    f = V.FExtractor(SC.A_NF, 1.2, 8, 20, 7, SC.A_W, SC.A_H, max_batch=4)
    yield f
    f.close()


def _same_words(got_u, got_d, ref, what):
    assert np.array_equal(SC.words(got_u), SC.words(ref["u"])), what
    assert np.array_equal(SC.words(got_d), SC.words(ref["depth"])), what


@pytest.mark.parametrize("seed,bf,fx", CASES)
def test_scene_a_compute_stereo_matches(fe, scenes, seed, bf, fx):
    (L, R), ref = scenes[(seed, bf, fx)]
    (kL, _, _), (kR, _, _) = fe.compute_batch([L, R])
    assert kp_equal(kL, ref["kL"]) and kp_equal(kR, ref["kR"])
    u, d = V.ComputeStereoMatches(fe, 0, fe, 1, bf, fx)
    _same_words(u, d, ref, (seed, bf, fx))
    got = dict(ref, u=u, depth=d)
    assert SC.clamped_survivors(got, bf).sum() >= SC.A_MIN_CLAMPED


@pytest.mark.parametrize("seed,bf,fx", CASES)
def test_scene_a_as_second_job_of_a_batch(fe, scenes, seed, bf, fx):
    (L, R), ref = scenes[(seed, bf, fx)]
    (oL, oR), oref = scenes[("ordinary", bf, fx)]
    fe.compute_batch([oL, oR, L, R])
    res = V.ComputeStereoMatchesBatch(fe, [0, 2], fe, [1, 3], bf, fx)
    _same_words(res[0][0], res[0][1], oref, ("job 0", seed, bf, fx))
    _same_words(res[1][0], res[1][1], ref, ("job 1", seed, bf, fx))


@pytest.mark.parametrize("seed,bf,fx", CASES)
def test_scene_a_frame_stereo_on_a_two_slot_context(scenes, seed, bf, fx):
    """extraction + matching in one enqueue, results delivered inside the context's block"""
    import torch
    (L, R), ref = scenes[(seed, bf, fx)]
    pitch = 384
    dev = torch.zeros((2, SC.A_H, pitch), dtype=torch.uint8, device="cuda")
    dev[0, :, :SC.A_W] = torch.from_numpy(L).cuda()
    dev[1, :, :SC.A_W] = torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    f = V.FExtractor(SC.A_NF, 1.2, 8, 20, 7, SC.A_W, SC.A_H, max_batch=2)
    try:
        f.frame_stereo_async([dev[0].data_ptr(), dev[1].data_ptr()], pitch, bf, fx)
        feats, st = f.frame_stereo_wait()
        assert kp_equal(feats[0][0], ref["kL"]) and kp_equal(feats[1][0], ref["kR"])
        assert np.array_equal(feats[0][1], ref["dL"]) and np.array_equal(feats[1][1], ref["dR"])
        _same_words(st[0][0], st[0][1], ref, (seed, bf, fx))
    finally:
        f.close()


@pytest.mark.parametrize("flat_rows", [100, SC.A_H])
def test_scene_c_empty_row_buckets_and_no_right_keypoints(fe, flat_rows):
    """left keypoints whose row bucket is empty (zero-trip candidate loop), and a right image without any keypoint
    (nothing accepted: the median cut has no list to work on) -- compared with the oracle, not only with -1"""
    bf, fx = SC.A_CAMERAS[0]
    L, R = SC.scene_c(3, flat_rows)
    ref = SC.oracle_stereo(L, R, SC.A_NF, bf, fx)
    SC.check_scene_c(ref, flat_rows)
    (kL, _, _), (kR, _, _) = fe.compute_batch([L, R])
    assert kp_equal(kL, ref["kL"]) and kp_equal(kR, ref["kR"])
    u, d = V.ComputeStereoMatches(fe, 0, fe, 1, bf, fx)
    _same_words(u, d, ref, flat_rows)


def test_scene_b_row_bucket_of_more_than_64_candidates():
    """The pair of test_stereo_matches_kitti_same_context at 2000 features already fills a row bucket that a left
    keypoint reads with more than 64 right keypoints (asserted here on the oracle's keypoints): the candidate loop of
    k_stereo_best takes a second turn and its result is compared."""
    L, R = SC.scene_b()
    ref = SC.oracle_stereo(L, R, SC.B_NF, SC.B_BF, SC.B_FX)
    assert SC.check_scene_b(ref) > 64
    f = V.FExtractor(SC.B_NF, 1.2, 8, 20, 7, SC.B_W, SC.B_H, max_batch=2)
    try:
        (kL, _, _), (kR, _, _) = f.compute_batch([L, R])
        assert kp_equal(kL, ref["kL"]) and kp_equal(kR, ref["kR"])
        u, d = V.ComputeStereoMatches(f, 0, f, 1, SC.B_BF, SC.B_FX)
        _same_words(u, d, ref, "scene B")
        assert (u >= 0).sum() > 300
    finally:
        f.close()
