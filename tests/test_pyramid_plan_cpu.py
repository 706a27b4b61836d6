"""Host plan of the fused pyramid (vslam::build_pyramid_group) in its two LDS layouts, evaluated on the CPU through
vslamh_pyramid_fused_shape: the ping-pong layout keeps a tile within the 20 KB one k_fast_bands workgroup holds, its two
regions never overlap while both are live, every tile's store ranges partition every level exactly once, and the plan's
CPU emulation (same indexing as k_pyramid_group) gives the oracle's pyramid byte for byte.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import vi_slam_amd as V
from vi_slam_amd import synth
from oracle import orbo
from pyramid_tiles_cases import CASES

LDS_BUDGET = 20 * 1024  # one k_fast_bands workgroup: 8 of them fill the 160 KB of a CU

KITTI, HUT, FULLHD = (1241, 376), (752, 480), (1920, 1080)
# the small frames of tests/test_gpu_pyramid_tiles.py
SMALL = [(96, 64), (96, 70), (160, 144), (300, 144), (520, 144), (437, 151), (144, 144), (300, 140), (64, 48)]


def _host():
    H = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(V.__file__)), "libvslam_host.so"))
    vp, i = C.c_void_p, C.c_int
    H.vslamh_pyramid_fused_shape.argtypes = [vp, i, i, C.c_size_t, i, C.c_float, i, i, i, i, vp, vp, vp, vp, vp, i, vp]
    return H


def _plan(w, h, batch, rows, pingpong, nlevels=8, scale=1.2, img=None):
    """-> (groups, lds_bytes_max, tiles_total, (rows, pingpong, lds limit), records[n, 16], levels >= 1 packed)"""
    if img is None:
        img = np.zeros((h, w), np.uint8)
    e = orbo.Extractor(500, scale=scale, nlevels=nlevels)
    e.pyramid_only(img)
    sizes = [e.level(l).shape for l in range(nlevels)]
    out = np.zeros(sum(a * b for a, b in sizes[1:]) + 16, np.uint8)
    lds, nt, nrec = C.c_int(), C.c_int(), C.c_int()
    shape = (C.c_int32 * 3)()
    recs = np.zeros((1 << 16, 16), np.int32)
    ng = _host().vslamh_pyramid_fused_shape(img.ctypes.data, w, h, img.strides[0], 500, scale, nlevels, batch, rows, pingpong,
                                            out.ctypes.data, C.byref(lds), C.byref(nt), shape, recs.ctypes.data, len(recs),
                                            C.byref(nrec))
    assert ng >= 0, "plan or emulation failed: %d" % ng
    assert nrec.value <= len(recs)
    return ng, lds.value, nt.value, tuple(shape), recs[:nrec.value], out, sizes, e


def _check_plan(w, h, batch, rows, pingpong, nlevels=8, scale=1.2):
    ng, lds, nt, shape, recs, _, sizes, _ = _plan(w, h, batch, rows, pingpong, nlevels, scale)
    assert shape[1] == (1 if pingpong else 0)
    assert ng == 1 + max(0, (nlevels - 1 - 3 + 3) // 4)
    if pingpong:
        assert 0 < lds <= LDS_BUDGET, (w, h, lds)
        assert recs[:, 15].max() <= LDS_BUDGET
    covered = [np.zeros(((sizes[l][1] + 3) // 4, sizes[l][0]), np.int32) for l in range(nlevels)]  # [quad, row] store counts
    for g in range(ng):
        G = recs[recs[:, 0] == g]
        nl = int(G[0, 3])
        l0 = 0 if g == 0 else 3 + 4 * (g - 1)
        for t in np.unique(G[:, 1]):
            T = G[G[:, 1] == t]
            assert list(T[:, 2]) == list(range(nl + 1))
            size = T[:, 13].astype(np.int64) * T[:, 7]
            lo, hi = T[:, 12].astype(np.int64), T[:, 12] + size
            rt = [(int(T[j, 14]), int(T[j, 14]) + 8 * int(T[j, 7])) for j in range(1, nl + 1)]
            assert max(int(hi.max()), max(b for _, b in rt)) <= int(T[0, 15]) <= (LDS_BUDGET if pingpong else 64 * 1024)
            for j in range(1, nl + 1):
                assert size[j] > 0
                # while level j is computed, level j-1 (read) and level j (written) are live; so are all row tables
                assert hi[j] <= lo[j - 1] or hi[j - 1] <= lo[j], ("regions overlap", w, h, g, t, j)
                for a, b in rt:
                    assert hi[j] <= a or b <= lo[j], ("tile over a row table", w, h, g, t, j)
                    assert hi[j - 1] <= a or b <= lo[j - 1]
                if pingpong and j >= 2:
                    assert lo[j] == lo[j - 2], "level j goes over level j-2"
                # stores stay inside what the tile computes
                c0q, ncq, r0, nr, sq0, sq1, sr0, sr1 = int(T[j, 4]) // 4, int(T[j, 5]) // 4, *[int(v) for v in T[j, 6:12]]
                # every tile owns something on every level: the planner makes no more tile rows / columns than the deepest
                # level of a group has rows / quads, so k_pyramid_group's "tile that owns nothing" exit is never taken
                assert sq1 > sq0 and sr1 > sr0, ("a tile owns nothing", w, h, g, t, j)
                assert c0q <= sq0 and sq1 <= c0q + ncq and r0 <= sr0 and sr1 <= r0 + nr
                covered[l0 + j][sq0:sq1, sr0:sr1] += 1
    for l in range(1, nlevels):
        assert np.all(covered[l] == 1), ("level %d is not partitioned exactly once" % l, w, h)
    return lds, nt


@pytest.mark.parametrize("wh", [KITTI, HUT, FULLHD])
def test_default_batch_shape_fits_one_fast_hole(wh):
    """the shape a context of 32 images gets by default, if it is the ping-pong one, and the ping-pong shape forced"""
    w, h = wh
    _check_plan(w, h, 32, -1, 1)
    _, _, _, shape, recs, _, _, _ = _plan(w, h, 32, -1, -1)
    if shape[1]:
        assert shape[2] == LDS_BUDGET and recs[:, 15].max() <= LDS_BUDGET


@pytest.mark.parametrize("wh", [KITTI, HUT, FULLHD])
@pytest.mark.parametrize("rows", [16, 28, 32, 40, 48, 64])
def test_pingpong_plans_of_every_tile_height(wh, rows):
    _check_plan(wh[0], wh[1], 32, rows, 1)


@pytest.mark.parametrize("wh", [KITTI, HUT, FULLHD])
def test_resident_layout_is_the_plan_it_was(wh):
    """every level resident (pyr_pingpong = 0): the tiles follow each other in LDS; 48 / 40-row tiles as before"""
    w, h = wh
    lds, _ = _check_plan(w, h, 32, -1, 0)
    assert LDS_BUDGET < lds <= 64 * 1024
    _, _, _, shape, recs, _, _, _ = _plan(w, h, 32, -1, 0)
    assert shape == (40 if w * h > 1000000 else 48, 0, 64 * 1024)
    for g in np.unique(recs[:, 0]):
        T = recs[(recs[:, 0] == g) & (recs[:, 1] == 0)]
        assert list(T[:, 12]) == list(np.concatenate([[0], np.cumsum(T[:-1, 13] * T[:-1, 7])]))
    assert _plan(w, h, 1, -1, -1)[3][:2] == (16, 0)  # contexts of one or two images keep their shape


@pytest.mark.parametrize("wh", SMALL)
@pytest.mark.parametrize("pingpong", [0, 1])
@pytest.mark.parametrize("lv", [(8, 1.2), (4, 1.5)])
def test_small_frames(wh, pingpong, lv):
    _check_plan(wh[0], wh[1], 9, -1, pingpong, lv[0], lv[1])
    _check_plan(wh[0], wh[1], 9, 8, pingpong, lv[0], lv[1])  # several tile rows on a small frame


@pytest.mark.parametrize("wh", [KITTI, (437, 101)])
@pytest.mark.parametrize("pingpong", [0, 1])
def test_emulated_plan_equals_the_oracle(wh, pingpong):
    """the emulation marks what a level's tile overwrites as not computed, so a tap into a dead level fails the plan"""
    w, h = wh
    img = synth.make_frame(w, h, seed=w + pingpong)
    _, _, _, _, _, out, sizes, e = _plan(w, h, 32, -1, pingpong, img=img)
    o = 0
    for l in range(1, 8):
        hh, ww = sizes[l]
        assert np.array_equal(out[o:o + hh * ww].reshape(hh, ww), e.level(l)), l
        o += hh * ww


@pytest.mark.parametrize("pingpong", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_r%d_b%d_l%d_s%.1f" % c)
def test_every_gpu_case_gets_a_fused_plan(case, pingpong):
    """vslam_fe_create falls back to one launch per level when a group has no plan: the GPU test's cases must not"""
    w, h, rows, n, nlevels, scale = case
    _check_plan(w, h, n, rows, pingpong, nlevels, scale)
