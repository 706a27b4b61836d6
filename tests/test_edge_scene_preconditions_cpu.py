"""CPU: the edge scenes of stereo_edge_cases.py / bow_sparse_cases.py do on the ORACLE what they were built for.  The GPU
tests that use them compare device results with the oracle; that comparison only means something for a branch if the
scene takes the oracle down it and the branch's effect reaches the compared output."""
import numpy as np
import pytest

import bow_sparse_cases as BC
import stereo_edge_cases as SC
from oracle import orbo


@pytest.mark.parametrize("seed", SC.A_SEEDS)
@pytest.mark.parametrize("bf,fx", SC.A_CAMERAS)
def test_stereo_scene_a_clamped_matches_survive_the_cut(seed, bf, fx):
    L, R = SC.scene_a(seed)
    ref = SC.oracle_stereo(L, R, SC.A_NF, bf, fx)
    before_cut, clamped = SC.check_scene_a(ref, bf, fx)
    ok = ref["u"] >= 0
    print("scene A seed %d bf %g fx %g: accepted %d (%d before the cut), clamped survivors %d, median SAD %d"
          % (seed, bf, fx, ok.sum(), before_cut, clamped, SC.median_sad(ref)))
    assert np.all(ref["depth"][ok] > 0) and np.all(ref["depth"][~ok] == -1)
    if fx == 12.0:
        # maxD ~ 12: the lower band (true disparity 12) meets `disparity < maxD` from both sides
        maxD = np.float32(bf) / (np.float32(bf) / np.float32(fx))
        disp = ref["kL"]["x"][ok] - ref["u"][ok]
        assert maxD - 1.0 < disp.max() < maxD
        wide = SC.oracle_stereo(L, R, SC.A_NF, bf, 400.0)
        lost = (wide["sad"] >= 0) & (ref["sad"] < 0) & (wide["kL"]["x"] - wide["u"] >= maxD)
        assert lost.sum() >= 10, "no match is rejected by disparity >= maxD"


def test_stereo_scene_b_has_a_row_bucket_of_more_than_64():
    """the 1241x376 pair of test_stereo_matches_kitti_same_context already has it: nfeatures stays 2000"""
    L, R = SC.scene_b()
    ref = SC.oracle_stereo(L, R, SC.B_NF, SC.B_BF, SC.B_FX)
    print("scene B: largest row bucket read by a left keypoint: %d" % SC.check_scene_b(ref))
    assert (ref["u"] >= 0).sum() > 300


@pytest.mark.parametrize("flat_rows", [100, SC.A_H])
def test_stereo_scene_c_left_keypoints_read_empty_row_buckets(flat_rows):
    bf, fx = SC.A_CAMERAS[0]
    L, R = SC.scene_c(3, flat_rows)
    ref = SC.oracle_stereo(L, R, SC.A_NF, bf, fx)
    print("scene C flat rows %d: empty buckets read %d, matches %d" % ((flat_rows,) + SC.check_scene_c(ref, flat_rows)))


def _shared_only(fv, keep):
    idx = [i for i, n in enumerate(fv["fv_nodes"]) if n in keep]
    off, feat = [0], []
    for i in idx:
        feat.extend(fv["fv_feat"][fv["fv_off"][i]:fv["fv_off"][i + 1]])
        off.append(len(feat))
    return dict(fv_nodes=fv["fv_nodes"][idx], fv_off=np.array(off, np.int32), fv_feat=np.array(feat, np.int32))


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
def test_sparse_bow_scene_node_lists_differ(levelsup):
    voc = BC.vocabulary()
    feats = BC.oracle_features(BC.frames())
    fvs = BC.oracle_fvs(voc, feats, levelsup)
    c = BC.check_sparse(fvs[0], fvs[1], levelsup)
    (ka, da), (kb, db) = feats
    nm, _ = orbo.search_by_bow(ka, da, np.ones(len(ka), np.uint8), fvs[0], kb, db, fvs[1], 0.9, True)
    print("sparse BoW levelsup %d: %s, matches %d" % (levelsup, c, nm))
    assert nm >= 10
    # the walk over two different lists pairs exactly the shared nodes: with every exclusive node taken out of both
    # lists (identical lists, no lower_bound step left) the oracle's result is the same, in both argument orders
    shared = set(np.intersect1d(fvs[0]["fv_nodes"], fvs[1]["fv_nodes"]).tolist())
    fl = BC.flags(len(ka), len(kb))
    for a, b in ((0, 1), (1, 0)):
        (k1, d1), (k2, d2) = feats[a], feats[b]
        want = orbo.search_by_bow_keyframes(k1, d1, fl[a], fvs[a], k2, d2, fl[b], fvs[b], 0.9, True)
        got = orbo.search_by_bow_keyframes(k1, d1, fl[a], _shared_only(fvs[a], shared), k2, d2, fl[b],
                                           _shared_only(fvs[b], shared), 0.9, True)
        assert want[0] == got[0] and np.array_equal(want[1], got[1])
        assert want[0] >= 10
