"""k_pyramid_group with both LDS layouts of its plan (vslam_tuning.pyr_pingpong: two regions within 20 KB that alternate
levels reuse / every level resident) on the smallest frames at which the tiling can go wrong: every level of every slot,
read back through vslam_fe_level_copy, equals the oracle's pyramid byte for byte.

The planner splits a level evenly between the tiles, and there are never more tile rows or columns than a level of the
group has rows or quads (at least 4 rows and 8 quads of the first level per tile, levels shrink by at most 1.5^3), so a
tile that owns nothing on a deep level does not occur; 4-row tiles on a frame whose last level is 40 px high (a context
accepts no smaller level) come closest: one or two owned rows on the deepest level."""
import numpy as np
import pytest

import vi_slam_amd as V
from vi_slam_amd import synth
from oracle import orbo
from pyramid_tiles_cases import CASES

pytestmark = pytest.mark.gpu


_ref = {}


def _frames_and_pyramids(w, h, n, nlevels, scale):
    key = (w, h, n, nlevels, scale)
    if key not in _ref:
        imgs = [synth.make_frame(w, h, seed=w + h, step=s) for s in range(n)]
        e = orbo.Extractor(200, scale=scale, nlevels=nlevels)
        pyr = []
        for im in imgs:
            e.pyramid_only(im)
            lv = [e.level(l) for l in range(nlevels)]
            for a in lv:
                a.setflags(write=False)
            pyr.append(lv)
        _ref[key] = (imgs, pyr)
    return _ref[key]


@pytest.mark.parametrize("pingpong", [1, 0], ids=["pingpong", "resident"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_r%d_b%d_l%d_s%.1f" % c)
def test_every_level_equals_the_oracle(case, pingpong):
    w, h, rows, n, nlevels, scale = case
    imgs, want = _frames_and_pyramids(w, h, n, nlevels, scale)
    tn = dict(pyr_pingpong=pingpong)
    if rows >= 0:
        tn["pyr_rows"] = rows
    fe = V.FExtractor(200, scale, nlevels, 20, 7, w, h, max_batch=n, tuning=tn)
    try:
        fe.compute_batch(imgs)
        for s in range(n):
            for l in range(nlevels):
                got = fe.mvImagePyramid(l, slot=s)
                assert got.shape == want[s][l].shape
                assert np.array_equal(got, want[s][l]), (case, pingpong, "slot %d level %d" % (s, l))
    finally:
        fe.close()


def test_default_shape_of_a_batch_context():
    """no switch set: what a context of nine images picks by itself"""
    w, h, n = 437, 151, 9
    imgs, want = _frames_and_pyramids(w, h, n, 8, 1.2)
    fe = V.FExtractor(200, 1.2, 8, 20, 7, w, h, max_batch=n)
    try:
        fe.compute_batch(imgs)
        for s in range(n):
            for l in range(8):
                assert np.array_equal(fe.mvImagePyramid(l, slot=s), want[s][l]), (s, l)
    finally:
        fe.close()
