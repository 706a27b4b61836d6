"""GPU (-m gpu): the grid Harris / Shi-Tomasi detector (vilib::HarrisGPU) through the C ABI of include/vslam_harrisgrid.h,
bit for bit against the numpy restatement tests/harris_ref.py (itself pinned by tests/test_harrisgrid_cpu.py) and the
committed golden grids."""
import os

import numpy as np
import pytest

import harris_cases as HC
import harris_ref as hr
import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth
from vi_slam_amd import harrisgrid as HG
from vi_slam_amd.harrisgrid import HarrisGPU

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """(pos, score, level, keep, n_keep), floats compared as words"""
    assert np.array_equal(_u32(got[1]), _u32(want[1])), "score"
    assert np.array_equal(got[2], want[2]), "level"
    assert np.array_equal(_u32(got[0]), _u32(want[0])), "pos"
    assert np.array_equal(got[3], want[3]), "keep"
    assert int(got[4]) == int(want[4]), "n_keep"


def _ref(img, cfg):
    return hr.detect(img, (cfg.get("cell_size_width", 32), cfg.get("cell_size_height", 32)), cfg.get("min_level", 0),
                     cfg.get("max_level", 1), (cfg.get("horizontal_border", 0), cfg.get("vertical_border", 0)),
                     cfg.get("filter_border_type", hr.BORDER_SKIP), cfg.get("use_harris", True), cfg.get("harris_k", 0.04),
                     cfg.get("quality_level", 0.1), cfg.get("tie_rule", 0))


def test_the_mirror_names_the_border_types_in_the_references_order():
    assert (HG.BORDER_SKIP, HG.BORDER_ZERO, HG.BORDER_REPLICATE, HG.BORDER_REFLECT, HG.BORDER_WRAP, HG.BORDER_REFLECT_101) == (
        hr.BORDER_SKIP, hr.BORDER_ZERO, hr.BORDER_REPLICATE, hr.BORDER_REFLECT, hr.BORDER_WRAP, hr.BORDER_REFLECT_101)


SWEEP = [dict(use_harris=uh, filter_border_type=b, max_level=2) for uh in (True, False) for b in range(6)] + [
    dict(),                                                   # test_harris.cpp:143-154: one level, 32x32, SKIP, k 0.04, q 0.1
    dict(use_harris=False),
    dict(max_level=2), dict(max_level=3), dict(max_level=3, use_harris=False, filter_border_type=hr.BORDER_WRAP),
    dict(min_level=1, max_level=3), dict(min_level=1, max_level=3, use_harris=False, filter_border_type=hr.BORDER_REFLECT_101),
    dict(max_level=3, cell_size_width=64, cell_size_height=64),
    dict(max_level=3, cell_size_width=64, cell_size_height=64, filter_border_type=hr.BORDER_REPLICATE, use_harris=False),
    dict(max_level=2, cell_size_width=64, cell_size_height=32), dict(max_level=2, cell_size_width=64, cell_size_height=32, tie_rule=1),
    dict(max_level=3, horizontal_border=8, vertical_border=5), dict(max_level=2, horizontal_border=16, vertical_border=16),
    dict(max_level=2, horizontal_border=200, vertical_border=3),
    dict(max_level=2, horizontal_border=16, vertical_border=16, filter_border_type=hr.BORDER_ZERO, use_harris=False),
    dict(max_level=3, tie_rule=1), dict(max_level=3, tie_rule=1, use_harris=False, filter_border_type=hr.BORDER_REFLECT),
    dict(max_level=2, quality_level=0.0), dict(max_level=2, quality_level=0.9), dict(max_level=2, quality_level=0.9, use_harris=False),
    dict(max_level=2, quality_level=0.0, use_harris=False, filter_border_type=hr.BORDER_ZERO),
    dict(max_level=2, harris_k=0.15), dict(max_level=3, harris_k=0.15, filter_border_type=hr.BORDER_REFLECT_101, tie_rule=1),
]


@pytest.mark.parametrize("cfg", SWEEP, ids=lambda c: "-".join("%s=%s" % (k[:6], v) for k, v in c.items()) or "default")
def test_grid_and_keep_equal_the_restatement_on_reference_image_crops(cfg):
    for img in HC.crops().values():
        h, w = img.shape
        d = HarrisGPU(w, h, **cfg)
        try:
            got = d.detect(img)
            want = _ref(img, cfg)
            _same(got, want)
            raw = d.detect(img, raw=True)  # the callback overload: the grid alone
            assert all(np.array_equal(a, b) for a, b in zip(raw, got[:3]))
            pts = d.getPoints(*got)
            assert len(pts) == want[4] and all(p[2] > 0 for p in pts)
            if cfg.get("horizontal_border", 0) < 100:
                assert (got[1] > 0).sum() > 10
        finally:
            d.close()


@pytest.mark.parametrize("use_harris", [True, False])
def test_pyramid_levels_and_response_images(use_harris):
    """vilib::Frame's half-sampled pyramid and DetectorBaseGPU::copyResponseTo, zeros outside the computed region included."""
    img = HC.crops()["hut"]
    h, w = img.shape
    for b in range(6):
        d = HarrisGPU(w, h, max_level=3, filter_border_type=b, use_harris=use_harris, harris_k=0.04, horizontal_border=6)
        try:
            d.detect(img)
            cur = img
            for l in range(3):
                if l:
                    cur = orbo.fg_halfsample(cur)
                assert np.array_equal(d.level(0, l), cur)
                want = hr.response(cur, b, use_harris, 0.04)
                got = d.response(0, l)
                assert got.shape == want.shape and np.array_equal(_u32(got), _u32(want)), (b, l)
                m = 2 if b == hr.BORDER_SKIP else 1
                assert np.all(_u32(got[:m]) == 0) and np.all(_u32(got[:, :m]) == 0) and np.all(_u32(got[-m:]) == 0) and np.all(_u32(got[:, -m:]) == 0)
                assert np.any(got[m] != 0) and np.any(got[:, -m - 1] != 0)
        finally:
            d.close()


def _blocks():
    """256 x 256 in 32-pixel blocks of random grey: level 5 is the 8 x 8 image of the blocks, so that the restatement's
    response has non-zero values on every level up to there"""
    grey = np.random.default_rng(24).integers(0, 256, (8, 8)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(grey, np.ones((32, 32), np.uint8)))


@pytest.mark.parametrize("border", [hr.BORDER_SKIP, hr.BORDER_REFLECT_101])
@pytest.mark.parametrize("cell", [32, 64])
def test_six_levels_down_to_one_and_two_pixel_cells(cell, border):
    """Levels 4 and 5 of 32 x 32 cells and level 5 of 64 x 64 cells have 2- and 1-pixel cells: the window is staged byte by
    byte there, dword by dword above; the border rule is applied to either."""
    img = _blocks()
    d = HarrisGPU(256, 256, cell, cell, 0, 6, filter_border_type=border)
    try:
        _same(d.detect(img), hr.detect(img, (cell, cell), 0, 6, filter_border=border))
        cur = img
        for l in range(1, 6):
            cur = hr.halfsample(cur)
            if l < 3:
                continue
            want = hr.response(cur, border, True, 0.04)
            assert np.any(want != 0), l
            assert np.array_equal(_u32(d.response(0, l)), _u32(want)), l
    finally:
        d.close()


def test_golden_grids():
    crops = HC.crops()
    z = np.load(os.path.join(HC.GOLD, "harrisgrid.npz"))
    n = 0
    for key in z.files:
        if not key.endswith("_score"):
            continue
        stem = key[:-6]
        name, cfg = stem.split("__")
        lv0, lv1, hb, vb, bt, uh, k1000, q100, tie, cw, ch = [int(v) for v in cfg.split("_")]
        img = crops[name]
        d = HarrisGPU(img.shape[1], img.shape[0], cw, ch, lv0, lv1, hb, vb, bt, bool(uh), k1000 / 1000.0, q100 / 100.0, tie)
        try:
            keep = z[stem + "_keep"]
            _same(d.detect(img), (z[stem + "_pos"], z[key], z[stem + "_level"], keep, int(keep.sum())))
        finally:
            d.close()
        n += 1
    assert n >= 24


@pytest.mark.parametrize("border", [hr.BORDER_SKIP, hr.BORDER_REFLECT_101])
def test_kitti_size_batch_host_and_device_inputs(border):
    """Height 376 is no multiple of 32: with BORDER_REFLECT_101 response row h - 2 depends on the rule below the image."""
    import torch
    W, H, B = 1240, 376, 6
    frames = [np.ascontiguousarray(synth.make_frame(1241, 376, step=s)[:, :W]) for s in range(B)]
    want = [hr.detect(f, (32, 32), 0, 3, (0, 0), border, True, 0.04, 0.1, 0) for f in frames]
    d = HarrisGPU(W, H, max_level=3, filter_border_type=border, max_batch=B)
    try:
        pos, sc, lv, keep, nk = d.detect_batch(frames)
        for s in range(B):
            _same((pos[s], sc[s], lv[s], keep[s], nk[s]), want[s])
        assert len(set(float(sc[s].max()) for s in range(B))) > 1  # the threshold is per image
        _same(d.detect(frames[2]), want[2])
        dev = torch.zeros((B, H, 1280), dtype=torch.uint8, device="cuda")
        for s in range(B):
            dev[s, :, :W] = torch.from_numpy(frames[s]).cuda()
        torch.cuda.synchronize()
        got = d.detect_batch(dev_ptrs=[dev[s].data_ptr() for s in range(B)], pitch=1280)
        for a, b in zip(got, (pos, sc, lv, keep, nk)):
            assert np.array_equal(a, b)
        assert (sc[0] > 0).mean() > 0.8
        r = d.response(3, 0)
        assert np.array_equal(_u32(r), _u32(hr.response(frames[3], border, True, 0.04)))
    finally:
        d.close()


@pytest.mark.parametrize("use_harris", [True, False])
@pytest.mark.parametrize("tie", [0, 1])
def test_equal_maxima_follow_the_tie_rule_on_the_device(use_harris, tie):
    d = HarrisGPU(96, 96, use_harris=use_harris, tie_rule=tie)
    try:
        for pts in HC.TIE_CASES:
            img = HC.squares(pts)
            got = d.detect(img)
            _same(got, hr.detect(img, use_harris=use_harris, tie_rule=tie))
            assert got[1][4] > 0 and got[4] >= 1
    finally:
        d.close()


def test_flat_and_binary_images():
    d = HarrisGPU(128, 64, max_level=2)
    try:
        for v in (0, 128, 255):
            pos, sc, lv, keep, nk = d.detect(np.full((64, 128), v, np.uint8))
            assert np.all(sc == 0) and np.all(lv == -1) and np.all(pos == 0) and not keep.any() and nk == 0
        rng = np.random.default_rng(0)
        noise = (rng.integers(0, 2, (64, 128)) * 255).astype(np.uint8)
        _same(d.detect(noise), hr.detect(noise, max_level=2))
    finally:
        d.close()
    for b in (hr.BORDER_WRAP, hr.BORDER_REFLECT_101):
        d = HarrisGPU(128, 64, max_level=2, filter_border_type=b, use_harris=False)
        try:
            _same(d.detect(noise), hr.detect(noise, max_level=2, filter_border=b, use_harris=False))
        finally:
            d.close()


def test_bad_parameters_raise():
    for bad in (dict(cell_size_width=48), dict(filter_border_type=6), dict(max_level=0), dict(max_level=9),
                dict(max_level=3, image_width=130), dict(quality_level=-0.1)):
        kw = dict(image_width=128, image_height=64)
        kw.update(bad)
        with pytest.raises(V.VslamError) as ei:
            HarrisGPU(**kw)
        assert ei.value.code == V.ERR_INVALID
