"""CPU: the yardstick of the grid Harris / Shi-Tomasi detector, tests/harris_ref.py, pinned on its own: its port of the
oracle's grid suppression against the oracle's FAST grids, its filter taps against integer Sobel sums, its border
rules, its tie order, the association of its box sums, and how much FMA contraction would change.  Then the golden
file it produced."""
import importlib.util
import os

import numpy as np
import pytest

import harris_cases as HC
import harris_ref as hr
from oracle import orbo

GOLD = HC.GOLD


@pytest.fixture(scope="module")
def crops():
    return HC.crops()


# (min_level, max_level, hborder, vborder, threshold, arc, score)
FAST_CONFIGS = [(0, 1, 0, 0, 10.0, 10, 1), (0, 3, 0, 0, 10.0, 10, 1), (1, 3, 8, 5, 20.0, 9, 2), (0, 2, 16, 16, 7.5, 11, 1),
                (0, 3, 40, 3, 10.5, 9, 0)]


@pytest.mark.parametrize("cfg", FAST_CONFIGS)
@pytest.mark.parametrize("tie", [0, 1])
def test_ported_grid_nms_equals_the_oracles_fast_grids(crops, cfg, tie):
    lv0, lv1, hbo, vbo, thr, arc, kind = cfg
    for img in crops.values():
        h, w = img.shape
        want = orbo.fg_detect(img, (32, 32), lv0, lv1, (hbo, vbo), thr, arc, kind, tie)
        nc, nr = (w + 31) // 32, (h + 31) // 32
        pos, sc, lv = np.zeros((nc * nr, 2), np.float32), np.zeros(nc * nr, np.float32), np.full(nc * nr, -1, np.int32)
        cur = img
        for l in range(lv1):
            if l:
                cur = orbo.fg_halfsample(cur)
            if l < lv0:
                continue
            resp = orbo.fg_response(cur, max(3, hbo - 1), max(3, vbo - 1), thr, arc, kind)  # fast_gpu.cpp:72-73
            hr.grid_nms(l, lv0, resp, max(3, hbo), max(3, vbo), 32, 32, nc, nr, pos, sc, lv, tie)
        assert np.array_equal(sc.view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(lv, want[2]) and np.array_equal(pos, want[0])
        assert (sc > 0).sum() > 3


def test_halfsample_equals_the_oracle(crops):
    for img in crops.values():
        assert np.array_equal(hr.halfsample(img), orbo.fg_halfsample(img))
        assert np.array_equal(hr.halfsample(hr.halfsample(img)), orbo.fg_halfsample(orbo.fg_halfsample(img)))


def test_unscaled_derivatives_are_integer_sobel_sums_over_four(crops):
    """Independent of harris_ref's own taps: 4 Dx = the 3x3 Sobel gx sum, 4 Dy = the gy sum, in int64; y points down."""
    for img in crops.values():
        dx, dy = hr.derivatives(img, hr.BORDER_ZERO, scale=False)
        P = np.pad(img.astype(np.int64), 1)
        h, w = img.shape

        def S(dy_, dx_):
            return P[1 + dy_:1 + dy_ + h, 1 + dx_:1 + dx_ + w]
        gx = (S(-1, 1) + 2 * S(0, 1) + S(1, 1)) - (S(-1, -1) + 2 * S(0, -1) + S(1, -1))
        gy = (S(1, -1) + 2 * S(1, 0) + S(1, 1)) - (S(-1, -1) + 2 * S(-1, 0) + S(-1, 1))
        assert np.array_equal(dx.astype(np.float64) * 4, gx.astype(np.float64))
        assert np.array_equal(dy.astype(np.float64) * 4, gy.astype(np.float64))
        assert np.abs(gx).max() > 100 and np.abs(gy).max() > 100
        sx, sy = hr.derivatives(img, hr.BORDER_ZERO)
        assert np.array_equal(sx, dx * (np.float32(1) / np.float32(255))) and sx.dtype == np.float32 and sy.dtype == np.float32


def test_each_border_type_pads_a_ramp_as_documented():
    img = (np.arange(6)[None, :] + 10 * np.arange(1, 6)[:, None]).astype(np.uint8)  # rows 10.., 20.., .. 50..; 6 wide
    rows = {hr.BORDER_ZERO: [0, 10, 11, 12, 13, 14, 15, 0], hr.BORDER_SKIP: [0, 10, 11, 12, 13, 14, 15, 0],
            hr.BORDER_REPLICATE: [10, 10, 11, 12, 13, 14, 15, 15], hr.BORDER_REFLECT: [10, 10, 11, 12, 13, 14, 15, 15],
            hr.BORDER_WRAP: [15, 10, 11, 12, 13, 14, 15, 10], hr.BORDER_REFLECT_101: [11, 10, 11, 12, 13, 14, 15, 14]}
    cols = {hr.BORDER_ZERO: [0, 10, 20, 30, 40, 50, 0], hr.BORDER_SKIP: [0, 10, 20, 30, 40, 50, 0],
            hr.BORDER_REPLICATE: [10, 10, 20, 30, 40, 50, 50], hr.BORDER_REFLECT: [10, 10, 20, 30, 40, 50, 50],
            hr.BORDER_WRAP: [50, 10, 20, 30, 40, 50, 10], hr.BORDER_REFLECT_101: [20, 10, 20, 30, 40, 50, 40]}
    corner = {hr.BORDER_ZERO: 0, hr.BORDER_SKIP: 0, hr.BORDER_REPLICATE: 10, hr.BORDER_REFLECT: 10, hr.BORDER_WRAP: 55,
              hr.BORDER_REFLECT_101: 21}
    for b in range(6):
        P = hr.pad(img, b)
        assert P.shape == (7, 8) and P.dtype == np.float32
        assert P[1].tolist() == rows[b] and P[:, 1].tolist() == cols[b] and P[0, 0] == corner[b]
        assert np.array_equal(P[1:6, 1:7], img.astype(np.float32))
    # the response region: m = 2 for BORDER_SKIP, else 1; 0.0f elsewhere
    big = HC.squares([(5, 5)], 16)
    for b in range(6):
        r = hr.response(big, b, True, 0.04)
        m = 2 if b == hr.BORDER_SKIP else 1
        inside = np.zeros((16, 16), bool)
        inside[m:16 - m, m:16 - m] = True
        assert np.all(r[~inside] == 0) and np.any(r[inside] != 0)
    with pytest.raises(ValueError):
        hr.pad(img, 6)


@pytest.mark.parametrize("use_harris", [True, False])
def test_translated_squares_tie_and_the_tie_rule_decides(use_harris):
    differ = 0
    for pts in HC.TIE_CASES:
        img = HC.squares(pts)
        r = hr.response(img, hr.BORDER_SKIP, use_harris, 0.04)
        v = hr.nms3x3(r)[32:64, 32:64]
        top = v.max()
        assert top > 0 and (v.view(np.uint32) == top.view(np.uint32)).sum() >= 2  # bit-equal maxima in the centre cell
        a = hr.detect(img, filter_border=hr.BORDER_SKIP, use_harris=use_harris, tie_rule=0)
        b = hr.detect(img, filter_border=hr.BORDER_SKIP, use_harris=use_harris, tie_rule=1)
        assert np.array_equal(a[1], b[1]) and a[1][4] == top  # same scores either way; only the position may differ
        differ += int(not np.array_equal(a[0], b[0]))
    assert differ >= 1


def test_mirrored_corners_of_a_square_are_not_equal_under_harris():
    """The box sums add in raster order, so the four corners of one square, mirror images of each other, do not get the
    same response: a box sum added in another order would be caught by a bit-for-bit comparison."""
    r = hr.response(HC.squares([(40, 40)]), hr.BORDER_SKIP, True, 0.04)
    y, x = np.unravel_index(np.argmax(r), r.shape)
    peak = r[y, x]
    mirrors = [r[y, 84 - x], r[84 - y, x], r[84 - y, 84 - x]]  # the square spans 40..44: mirror about 42
    assert all(0 < mv < peak for mv in mirrors)
    assert all(abs(float(mv) - float(peak)) < 1e-4 * float(peak) for mv in mirrors)  # equal but for rounding


@pytest.mark.parametrize("use_harris", [True, False])
def test_fma_contraction_would_change_the_response(crops, use_harris):
    img = crops["hut"]
    plain = hr.response(img, hr.BORDER_SKIP, use_harris, 0.04)
    fused = hr.response(img, hr.BORDER_SKIP, use_harris, 0.04, fused=True)
    inside = plain[2:-2, 2:-2].view(np.uint32) != fused[2:-2, 2:-2].view(np.uint32)
    assert inside.mean() > 0.05
    assert np.allclose(plain, fused, rtol=0, atol=1e-5 * float(np.abs(plain).max()))


def test_responses_are_often_negative_and_the_threshold_is_a_float_product(crops):
    for img in crops.values():
        for use_harris in (True, False):
            r = hr.response(img, hr.BORDER_SKIP, use_harris, 0.04)
            neg = (r[2:-2, 2:-2] < 0).mean()  # Shi-Tomasi is twice the smaller eigenvalue: never below 0 but for rounding
            assert 0.1 < neg < 0.4 if use_harris else neg < 0.01
            pos, sc, lv, keep, n = hr.detect(img, use_harris=use_harris, quality_level=0.1)
            assert np.all(sc >= 0) and np.array_equal(lv == -1, sc == 0)
            assert n == int((sc > sc.max() * np.float32(0.1)).sum()) and 0 < n <= int((sc > 0).sum())
            assert hr.detect(img, use_harris=use_harris, quality_level=0.0)[4] == int((sc > 0).sum())


def test_golden_file_regenerates_identically():
    spec = importlib.util.spec_from_file_location("make_harrisgrid_golden", os.path.join(GOLD, "make_harrisgrid_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(os.path.join(GOLD, "harrisgrid.npz"))
    made = gen.make()
    assert sorted(z.files) == sorted(made) and len(gen.CONFIGS) >= 12 and len(made) == 2 * 4 * len(gen.CONFIGS)
    for key, arr in made.items():
        assert z[key].dtype == arr.dtype and np.array_equal(z[key].view(np.uint8), arr.view(np.uint8)), key
    assert os.path.getsize(os.path.join(GOLD, "harrisgrid.npz")) < 200 * 1024


def test_library_exports_the_header_and_create_rejects_bad_parameters_without_a_cpu_fallback():
    """include/vslam_harrisgrid.h: the validity rules of vslam_fg_create plus quality_level >= 0 and the six border
    types; without a device the constructor fails."""
    import ctypes as C
    import re

    import torch
    import vi_slam_amd as V
    from vi_slam_amd import harrisgrid
    src = open(os.path.join(os.path.dirname(GOLD), "..", "include", "vslam_harrisgrid.h")).read()
    declared = sorted(set(re.findall(r"\b(vslam_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(["vslam_hg_create", "vslam_hg_destroy", "vslam_hg_grid", "vslam_hg_detect", "vslam_hg_detect_batch",
                               "vslam_hg_level_copy", "vslam_hg_response_copy"])
    L = C.CDLL(V.LIB_PATH)
    assert all(hasattr(L, name) for name in declared)
    assert C.sizeof(harrisgrid._HgParams) == 60
    for bad in (dict(cell_size_width=48), dict(filter_border_type=6), dict(filter_border_type=-1), dict(max_level=0),
                dict(max_level=9), dict(max_level=3, image_width=130), dict(max_batch=0), dict(max_batch=65),
                dict(quality_level=-0.1), dict(tie_rule=2)):
        kw = dict(image_width=128, image_height=64)
        kw.update(bad)
        with pytest.raises(V.VslamError) as ei:
            harrisgrid.HarrisGPU(**kw)
        assert ei.value.code == V.ERR_INVALID
    if torch.cuda.device_count() == 0:
        with pytest.raises(V.VslamError):
            harrisgrid.HarrisGPU(128, 64)
