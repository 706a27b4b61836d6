"""The edges of the rotation histogram that every matcher shares (vslam_md::rot_bin and vslam_md::three_maxima in
vi_slam_amd/csrc/vslam_matchdev.h): the two 0.1-ratio cuts of ComputeThreeMaxima (fmatcher.cpp:2813-2854), its strict `>`
on ties, the `rot < 0 -> rot + 360` branch and the `bin == HISTO_LENGTH -> 0` wrap.

Frames of at most 16 keypoints, all at octave 0 on a lattice coarser than any window, frame 2 = frame 1 apart from the
angles; query i has exactly one candidate, keypoint i, at Hamming distance 0, every other descriptor is > 100 bits away.
So every query is matched, match i falls into the bin of angle1[i] - angle2[i], and what survives shows which bins
ComputeThreeMaxima kept.  Each case states the histogram it means to produce; that is asserted against the reference
arithmetic alone (projection_bounds_ref._rot_bin) before anything runs.

About the wrap: with factor = 1 / HISTO_LENGTH = 1/30 (fmatcher.cpp:1001) a rotation in [0, 360) lands in bins 0..12, so a
rotation in [354, 360) is bin 12 and does NOT wrap -- `near_360` pins that (bin 12 of size 1 is dropped beside bin 0 of
size 11; wrapped into bin 0 it would survive).  Bin 30 itself needs a rotation in [885, 915), i.e. an angle outside
[0, 360): `wrap_30`.

CPU half: the host replay (vslamh_search_init), which runs the header's text, against tests/undistort_ref.py.
GPU half: SearchForInitialization, SearchByProjection(CurrentFrame, LastFrame) on the parallel and on the forced
sequential path, and SearchByBoW, each against the oracle as in the neighbouring tests of those entry points.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import projection_bounds_ref as PR
import undistort_ref as U
import vi_slam_amd as V
from oracle import orbo

W, H = 1241, 376
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
WINDOW = 20  # lattice pitch 70: windows of +-20 (init) and +-15 (projection, th 15 at octave 0) never overlap

# name -> (check_ori, [(angle1, angle2, how many matches)], intended histogram {bin: size}, bins that survive)
CASES = {
    # (float)1 < 0.1f * 10 is false (0.1f * 10 rounds to 1.0f): the second bin is kept
    "10_and_1": (True, [(20, 20, 10), (80, 20, 1)], {0: 10, 2: 1}, {0, 2}),
    # (float)1 < 0.1f * 11: the second and the third bin are dropped
    "11_and_1": (True, [(20, 20, 11), (80, 20, 1)], {0: 11, 2: 1}, {0}),
    # the `else if`: the second bin stays ((float)2 < 0.1f * 20 is false), the third goes
    "20_2_1": (True, [(20, 20, 13), (80, 20, 2), (140, 20, 1)], {0: 13, 2: 2, 4: 1}, {0, 2}),
    # four bins of equal size: the strict `>` keeps the three with the lowest index
    "four_equal": (True, [(20, 20, 4), (50, 20, 4), (80, 20, 4), (110, 20, 4)], {0: 4, 1: 4, 2: 4, 3: 4}, {0, 1, 2}),
    "near_360": (True, [(20, 20, 11), (358, 1, 1)], {0: 11, 12: 1}, {0}),
    "wrap_30": (True, [(110, 20, 11), (890, 0, 1)], {3: 11, 0: 1}, {3}),
    # 10 - 40 = -30 -> 330 -> bin 11
    "negative": (True, [(10, 40, 11), (30, 20, 1)], {11: 11, 0: 1}, {11}),
    "one_bin": (True, [(110, 20, 12)], {3: 12}, {3}),
    "ori_off": (False, [(20, 20, 4), (50, 20, 4), (80, 20, 4), (110, 20, 4)], {0: 4, 1: 4, 2: 4, 3: 4}, {0, 1, 2, 3}),
}


def _frames(name):
    """-> (check_ori, k1, k2, desc, bin of every pair, surviving bins)"""
    ori, groups, hist, keep = CASES[name]
    a1 = np.concatenate([np.full(c, a, np.float32) for a, _, c in groups])
    a2 = np.concatenate([np.full(c, b, np.float32) for _, b, c in groups])
    n = len(a1)
    assert n <= 16
    k1 = np.zeros(n, V.KP_DTYPE)
    k1["x"] = 60 + 70 * ((np.arange(n) * 7) % 16)  # one row of 16 lattice nodes, the bins interleaved along it
    k1["y"] = 180
    k1["size"], k1["response"], k1["octave"], k1["class_id"] = 31, 50, 0, -1
    k2 = k1.copy()
    k1["angle"], k2["angle"] = a1, a2
    desc = np.random.default_rng(5).integers(0, 256, (64, 32), dtype=np.uint8)[:n]
    d = U.hamming(desc, desc)
    assert np.all(d[~np.eye(n, dtype=bool)] > 100)  # exactly one candidate under TH_LOW = 50 / TH_HIGH = 100
    bins = np.array([PR._rot_bin(a, b) for a, b in zip(a1, a2)])
    assert dict(collections.Counter(bins.tolist())) == hist, name  # the histogram the case means to produce
    assert set(i for i in U._three_maxima([hist.get(b, 0) for b in range(30)]) if i >= 0) == (keep if ori else {0, 1, 2})
    return ori, k1, k2, desc, bins, keep


def _expect(name):
    ori, k1, k2, desc, bins, keep = _frames(name)
    want = np.where(np.isin(bins, sorted(keep)), np.arange(len(k1)), -1).astype(np.int32)
    return ori, k1, k2, desc, want


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_replay(name):
    ori, k1, k2, desc, want = _expect(name)
    bounds = (0.0, float(W), 0.0, float(H))
    rn, rm, rp = U.search_for_initialization(k1, desc, k2, desc, bounds, window=WINDOW, nnratio=0.9, check_ori=ori)
    assert np.array_equal(rm, want) and rn == int((want >= 0).sum())
    HL = C.CDLL(V.HOST_LIB_PATH)
    dm = np.minimum(U.hamming(desc, desc), 255).astype(np.uint8)
    pm = np.stack([k1["x"], k1["y"]], 1).astype(np.float32).copy()
    m = np.zeros(len(k1), np.int32)
    nm = HL.vslamh_search_init(_p(k1), len(k1), _p(k2), len(k2), _p(dm), W, H, _p(pm), _p(m), WINDOW, C.c_float(0.9), int(ori))
    assert nm == rn and np.array_equal(m, rm) and np.array_equal(pm, rp)


@pytest.fixture(scope="module")
def fe():
    f = V.FExtractor(1000, 1.2, 8, 20, 7, W, H, max_batch=1)
    yield f
    f.set_tuning(sbp_sequential=0)
    f.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matchers(fe, name):
    ori, k1, k2, desc, want = _expect(name)
    n = len(k1)
    nwant = int((want >= 0).sum())
    dk2, dd = _dev(k2), _dev(desc)
    m = V.FMatcher(fe, 0.9, ori)

    # SearchForInitialization
    prev = np.stack([k1["x"], k1["y"]], 1)
    nm, m12, pm = m.SearchForInitialization(k1, dd.data_ptr(), k2, dd.data_ptr(), prev, WINDOW)
    wn, wm, wp = orbo.search_for_initialization(k1, desc, k2, desc, W, H, window=WINDOW, nnratio=0.9, check_ori=ori)
    assert nm == wn and np.array_equal(m12, wm) and np.array_equal(pm, wp)
    assert np.array_equal(wm, want)

    # SearchByProjection(CurrentFrame = frame 2, LastFrame = frame 1): both poses the identity, the MapPoint of last-frame
    # keypoint i ten metres in front of it, so it projects onto current keypoint i
    T = np.hstack([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)])
    cam = (FX, FY, CX, CY, BF, BF / FX)
    z = np.float32(10.0)
    X = np.stack([(k1["x"] - CX) / FX * z, (k1["y"] - CY) / FY * z, np.full(n, z)], 1).astype(np.float32)
    flags = np.full(n, 3, np.uint8)
    sn, sm, sd = orbo.search_by_projection_frame(T, T, cam, 15, k1, flags, X, desc, k2, desc, np.full(n, -1, np.float32),
                                                 fe.GetScaleFactors(), W, H, mono=False, check_ori=ori)
    assert sd == (False, False) and np.array_equal(sm, want)
    for seq in (0, 1):
        fe.set_tuning(sbp_sequential=seq)
        gn, gm, gd = m.SearchByProjection(T, T, cam, 15, k1, flags, X, desc, dk2.data_ptr(), dd.data_ptr(), n, None, False,
                                          (W, H))
        assert gd == sd and gn == sn and np.array_equal(gm, sm), seq

    # SearchByBoW: one vocabulary node holds every feature of both frames
    fv = dict(fv_nodes=np.array([7], np.int32), fv_off=np.array([0, n], np.int32), fv_feat=np.arange(n, dtype=np.int32))
    ones = np.ones(n, np.uint8)
    bn, bm = m.SearchByBoW(k1, dd.data_ptr(), ones, fv, k2, dd.data_ptr(), fv)
    on, om = orbo.search_by_bow(k1, desc, ones, fv, k2, desc, fv, 0.9, ori)
    assert bn == on and np.array_equal(bm, om)
    assert np.array_equal(om, want) and on == nwant
