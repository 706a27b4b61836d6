"""GPU (-m gpu): SearchByBoW, SearchByBoWKeyFrames and SearchForTriangulation on the scene of bow_sparse_cases.py, where
most vocabulary nodes of one frame are missing from the other: the kernels' binary search for the driver's node in the
other list, and its miss exit, decide the result.  Both argument orders, so each list is once the driver and once
the searched side.  Everything equals the oracle; the preconditions are asserted on the oracle's FeatureVectors."""
import numpy as np
import pytest

import bow_sparse_cases as BC
import vi_slam_amd as V
from conftest import kp_equal
from oracle import orbo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    imgs = BC.frames()
    voc = BC.vocabulary()
    feats = BC.oracle_features(imgs)
    fe = V.FExtractor(BC.NF, 1.2, 8, 20, 7, BC.W, BC.H, max_batch=2)
    res = fe.compute_batch(imgs)
    for s in range(2):
        assert kp_equal(res[s][0], feats[s][0]) and np.array_equal(res[s][1], feats[s][1])
    vv = V.Vocabulary(voc)
    fvs = {}
    try:
        for lu in BC.LEVELSUP:
            want = BC.oracle_fvs(voc, feats, lu)
            BC.check_sparse(want[0], want[1], lu)
            vv.transform_slots_async(fe, 0, 2, lu)
            got = vv.transform_slots_wait([len(feats[0][0]), len(feats[1][0])])
            for s in range(2):
                for k in ("fv_nodes", "fv_off", "fv_feat"):
                    assert np.array_equal(got[s][k], want[s][k]), (lu, s, k)
            fvs[lu] = want
    finally:
        vv.close()
    yield dict(fe=fe, feats=feats, fvs=fvs, dev=[fe.slot_buffers(s)[1] for s in range(2)],
               flags=BC.flags(len(feats[0][0]), len(feats[1][0])), sf=fe.GetScaleFactors(), sig2=fe.GetScaleSigmaSquares())
    fe.close()


ORDERS = [(0, 1), (1, 0)]


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
@pytest.mark.parametrize("a,b", ORDERS)
def test_search_by_bow_on_differing_node_lists(scene, levelsup, a, b):
    (ka, da), (kb, db) = scene["feats"][a], scene["feats"][b]
    fva, fvb = scene["fvs"][levelsup][a], scene["fvs"][levelsup][b]
    fl = scene["flags"][a]
    total = 0
    for ratio in (0.9, 0.6):
        for ori in (True, False):
            nm, mf = V.FMatcher(scene["fe"], ratio, ori).SearchByBoW(ka, scene["dev"][a], fl, fva, kb, scene["dev"][b], fvb)
            wn, wm = orbo.search_by_bow(ka, da, fl, fva, kb, db, fvb, ratio, ori)
            assert nm == wn and np.array_equal(mf, wm), (levelsup, a, b, ratio, ori)
            total += wn
    assert total >= 10


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
@pytest.mark.parametrize("a,b", ORDERS)
def test_search_by_bow_keyframes_on_differing_node_lists(scene, levelsup, a, b):
    (ka, da), (kb, db) = scene["feats"][a], scene["feats"][b]
    fva, fvb = scene["fvs"][levelsup][a], scene["fvs"][levelsup][b]
    f1, f2 = scene["flags"][a], scene["flags"][b]
    total = 0
    for ratio in (0.9, 0.6):
        for ori in (True, False):
            nm, m12 = V.FMatcher(scene["fe"], ratio, ori).SearchByBoWKeyFrames(ka, scene["dev"][a], f1, fva, kb,
                                                                               scene["dev"][b], f2, fvb)
            wn, wm = orbo.search_by_bow_keyframes(ka, da, f1, fva, kb, db, f2, fvb, ratio, ori)
            assert nm == wn and np.array_equal(m12, wm), (levelsup, a, b, ratio, ori)
            total += wn
    assert total >= 10


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
@pytest.mark.parametrize("a,b", ORDERS)
def test_search_for_triangulation_on_differing_node_lists(scene, levelsup, a, b):
    (ka, da), (kb, db) = scene["feats"][a], scene["feats"][b]
    fva, fvb = scene["fvs"][levelsup][a], scene["fvs"][levelsup][b]
    F = BC.F12 if (a, b) == (0, 1) else BC.F12.T.copy()
    none_a, none_b = np.zeros(len(ka), np.uint8), np.zeros(len(kb), np.uint8)
    mono_a, mono_b = np.full(len(ka), -1, np.float32), np.full(len(kb), -1, np.float32)
    total = 0
    st_a, st_b = BC.u_right(ka, 5 + a), BC.u_right(kb, 5 + b)
    inside = (BC.W / 2.0, BC.H / 2.0)  # an epipole in the image: mono-mono pairs around it go, stereo ones stay
    for ua, ub, ep, only_stereo in ((mono_a, mono_b, BC.EPIPOLE, False), (st_a, st_b, BC.EPIPOLE, False),
                                    (st_a, st_b, inside, False), (st_a, st_b, inside, True)):
        for ori in (True, False):
            nm, pairs, m12 = V.FMatcher(scene["fe"], 0.6, ori).SearchForTriangulation(
                ka, scene["dev"][a], none_a, ua, fva, kb, scene["dev"][b], none_b, ub, fvb, F, ep, only_stereo)
            wn, wm = orbo.search_for_triangulation(ka, da, none_a, ua, fva, kb, db, none_b, ub, fvb, scene["sf"],
                                                   scene["sig2"], F, ep, only_stereo, False, ori)
            assert nm == wn and np.array_equal(m12, wm), (levelsup, a, b, ep, only_stereo, ori)
            assert len(pairs) == nm and np.array_equal(pairs[:, 1], m12[pairs[:, 0]])
            total += wn
    assert total >= 10
