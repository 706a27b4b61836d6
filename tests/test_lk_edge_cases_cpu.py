"""CPU: the synthetic cases of tests/lk_edge_cases.py do on the YARDSTICK (tests/lk_ref.py) what they are named for.
tests/test_gpu_featuretracker_edges.py compares the device with the yardstick on them; that comparison says something about a
branch only if the case takes the yardstick down it.  The yardstick is instrumented from outside (lk_edge_cases.Census wraps
its functions); its arithmetic is not touched.  Every count below is an "at least one" condition.

The census row that no case reaches is `ft_floor_int` saturation (a position of +-inf or beyond 2^31 that is not NaN).  An
exactly singular Gram matrix H has adj(H) = c * v * v^T with H v = 0, and v is orthogonal to the right-hand side Jres (Jres is a
sum of the Jacobian's rows, each of which is orthogonal to v).  The terms inf * v_k * Jres_k of an update row therefore have
mixed signs or a zero factor, and the row is NaN, never +-inf: test_exactly_singular_hessians_give_nan_updates_never_inf.  A
non-NaN runaway position needs a determinant that merely ROUNDS to zero on a regular H (for the 2-parameter form: a patch-32
template with |det| < 2^-25 * H0 * H2, e.g. full-contrast diagonal stripes), which no detector selects; it stays uncovered."""
import collections

import numpy as np
import pytest

import lk_cases as LC
import lk_edge_cases as EC
import lk_ref as lk

F = np.float32
EXITS = ("left edge (u == half-1)", "right edge (u == w-half)", "top edge (v == half-1)", "bottom edge (v == h-half)")
STARTS = ("u == half", "u == w-half-1", "v == half", "v == h-half-1")
FIT_CLASSES = [what % ax for ax in "xy" for what in ("last fit %s_tl == 0", "first miss %s_tl == -1", "last fit %s_tl + ps + 1 == size - 1",
                                                      "first miss %s_tl + ps + 1 == size")]


@pytest.fixture(scope="module")
def census():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = EC.census(name)
        return cache[name]
    return get


def _buffers(T, pred):
    """buffer ids whose inverse Hessian on some level satisfies pred(row of 10 floats)"""
    return {b for b in range(T.invh.shape[0]) for li in range(T.invh.shape[1]) if pred(T.invh[b, li])}


def _arith_nan0(row):
    return np.isnan(row[0]) and row[:1].view(np.uint32)[0] != lk.NAN_WORD


def _live(T):
    return {t.buffer_id for t in T.book.tracks}


def _exits(n, kind):
    return n["leave-the-level exit, " + kind]


# ------------------------------------------------------------------------------------------------- the hand-derivable facts
def _inv2(H):
    """the 2-parameter closed form in plain float32, written out here and not taken from lk_ref"""
    with np.errstate(all="ignore"):
        inv = F(1.0) / (F(H[0]) * F(H[2]) - F(H[1]) * F(H[1]))
        return np.array([F(H[2]) * inv, F(-1.0) * F(H[1]) * inv, F(H[0]) * inv], F)


def test_degenerate_inverses_by_hand():
    z = _inv2((0, 0, 0))
    assert np.isnan(z).all()                                     # 0 * inf
    h = _inv2((0, 0, 7.5))
    assert h[0] == np.inf and np.isnan(h[1]) and np.isnan(h[2])  # c * inf, -0 * inf, 0 * inf: a horizontal edge
    v = _inv2((7.5, 0, 0))
    assert np.isnan(v[0]) and np.isnan(v[1]) and v[2] == np.inf  # a vertical edge: the level is skipped
    for H in ((0, 0, 0), (0, 0, 7.5), (7.5, 0, 0), (3, 1, 2)):
        got, n = lk.invert(np.array(list(H) + [0] * 7, F), False, False)
        want = _inv2(H)
        assert n == 3 and np.array_equal(np.isnan(got[:3]), np.isnan(want))
        assert np.array_equal(got[:3][~np.isnan(want)], want[~np.isnan(want)])
    # the arithmetic NaN is not the marker word of a patch that does not fit
    assert z[:1].view(np.uint32)[0] != lk.NAN_WORD and np.isnan(lk.nan_marker())


@pytest.mark.parametrize("offset,gain", EC.AFFINE)
def test_exactly_singular_hessians_give_nan_updates_never_inf(offset, gain):
    """templates whose Gram matrix is exactly singular in every closed form (constant; a step along x, along y; a ramp; a
    diagonal step): with any right-hand side that comes from such a Jacobian the update rows are NaN wherever they are not finite"""
    rng = np.random.default_rng(5)
    ps = 8
    yy, xx = np.mgrid[0:ps + 2, 0:ps + 2]
    singular = 0
    for patch in (np.full((ps + 2, ps + 2), 200), 100 + 60 * (xx > 4), 100 + 60 * (yy > 5), 20 + 7 * xx, 20 + 7 * xx + 3 * yy, 100 + 60 * (xx + yy > 9)):
        patch = patch.astype(np.int32)
        inv, n = lk.invert(lk.hessian(patch, ps, offset, gain), offset, gain)
        if np.isfinite(inv[:n]).all():
            continue
        singular += 1
        img = np.clip(patch + rng.integers(-3, 4, patch.shape), 0, 255).astype(np.uint8)
        big = np.pad(img, 4, mode="edge")
        opt = lk.Options(affine_est_offset=offset, affine_est_gain=gain)
        (x, y), _, conv, go = lk.perform_lk(big, ps, patch.ravel(), inv, (F(9.25), F(9.5)), (F(0), F(0)), opt)
        assert not conv and not go and (np.isnan(x) or np.isnan(y)), (offset, gain)
    assert singular >= 4


# --------------------------------------------------------------------------------------------------------------- the cases
def test_shapes_and_frame_counts():
    shapes = set()
    for name in EC.cases():
        seq = EC.frames(name)
        assert 2 <= len(seq) <= 5 and all(f.dtype == np.uint8 and f.shape == seq[0].shape for f in seq), name
        shapes.add(seq[0].shape)
    assert shapes == {EC.LAND, EC.PORT, EC.WIDE}
    assert EC.PORT[0] > EC.PORT[1] and EC.WIDE[1] % 16 == 0 and EC.WIDE[1] % 32 != 0
    assert all(h % 16 == 0 and w % 16 == 0 for h, w in shapes)  # five levels


def test_flat_coarse(census):
    n, T, last = census("flat_coarse")
    assert n["inverse nan0, 2 parameters"] >= 1 and n["inf or NaN inverse used while tracking"] == 0
    nan = _buffers(T, _arith_nan0)
    coarse = {b for b in nan if _arith_nan0(T.invh[b, 0]) or _arith_nan0(T.invh[b, 1])}  # level 4 or 3
    assert coarse and coarse <= _live(T)                            # skipped on the coarse level, converged on finer ones
    assert last["life"].max() == len(EC.frames("flat_coarse")) - 1


@pytest.mark.parametrize("offset,gain", EC.AFFINE)
def test_edge_h(census, offset, gain):
    name = "edge_h_%d%d" % (offset, gain)
    n, T, last = census(name)
    p = lk.n_params(offset, gain)
    assert n["inverse inf0, %d parameters" % p] >= 1 and n["inf or NaN inverse used while tracking"] >= 1
    assert n["isnan(x) exit of the iteration loop"] >= 1
    inf0 = _buffers(T, lambda r: np.isinf(r[0]))
    assert inf0 and not (inf0 & _live(T))                          # the track is dropped
    assert last["counts"][1, 0] <= last["counts"][0, 1] - len(inf0)
    if p == 2:
        for b in inf0:
            rows = [r for r in T.invh[b] if np.isinf(r[0])]
            assert all(r[0] == np.inf and np.isnan(r[1]) and np.isnan(r[2]) for r in rows)


@pytest.mark.parametrize("offset,gain", EC.AFFINE)
def test_edge_v(census, offset, gain):
    name = "edge_v_%d%d" % (offset, gain)
    n, T, last = census(name)
    assert n["inverse nan0, %d parameters" % lk.n_params(offset, gain)] >= 1
    assert n["inf or NaN inverse used while tracking"] == 0 and n["isnan(x) exit of the iteration loop"] == 0  # the level is skipped
    nan = _buffers(T, _arith_nan0)
    assert nan and (nan & _live(T))                                # and the track survives through finer levels


@pytest.mark.parametrize("name,p", [("saturated", 3), ("saturated_11", 4)])
def test_saturated(census, name, p):
    n, T, last = census(name)
    assert n["inverse nan0, %d parameters" % p] >= 1 and n["inverse singular (1/det = inf)"] >= 1
    assert EC.frames(name)[0].max() == 255
    nan = _buffers(T, _arith_nan0)
    assert nan and nan <= _live(T)
    # the level under the NaN is exactly constant: H is singular through the gain column alone
    pyr = lk.pyramid(EC.frames(name)[0], 5)
    assert any(len(np.unique(pyr[l])) == 1 for l in (2, 3, 4))


def test_drift_exits_and_starts(census):
    total = sum((census(k)[0] for k in EC.cases() if k.startswith("drift_")), start=collections.Counter())
    for case, kind in (("drift_left", EXITS[0]), ("drift_right", EXITS[1]), ("drift_top", EXITS[2]), ("drift_bottom", EXITS[3])):
        assert _exits(census(case)[0], kind) >= 1, case
    for k in STARTS:
        assert total["started at %s and converged" % k] >= 1, k
    assert _exits(census("drift_patch32")[0], EXITS[0] + ", patch 32") + _exits(census("drift_patch32")[0], EXITS[2] + ", patch 32") >= 1
    for ps in (8, 16, 32):
        assert sum(_exits(total, "%s, patch %d" % (k, ps)) for k in EXITS) >= 1, ps


def test_patch_fit_boundaries(census):
    total = sum((census(k)[0] for k in EC.FIT), start=collections.Counter())
    for ps in (8, 16, 32):
        for what in FIT_CLASSES:
            assert total["patch %d: %s" % (ps, what)] >= 1, (ps, what)


def test_thresholds(census):
    for name, sizes in (("static_zero_threshold", (8, 16)), ("static_zero_threshold_32", (32,))):
        n, T, last = census(name)
        for ps in sizes:
            assert n["iteration exhaustion, patch %d" % ps] >= 1, (name, ps)
        runs = sum(v for k, v in n.items() if k.startswith("level runs"))
        # every track that has a template on some level runs one level, and exhausts it
        assert last["counts"][0, 1] // 2 < runs == sum(v for k, v in n.items() if k.startswith("iteration exhaustion")) <= last["counts"][0, 1]
        assert last["counts"][1, 0] == 0                            # and every track dies
    n, T, last = census("inf_threshold")
    conv = sum(v for k, v in n.items() if k.startswith("converged, patch"))
    assert conv == n["converged at iteration one"] > 100
    assert not any(k.startswith("iteration exhaustion") for k in n)


def test_faded_converges_in_the_last_iteration(census, monkeypatch):
    n, T, last = census("faded")
    assert n["converged at the last iteration"] >= 1
    assert n["iteration exhaustion, patch 16"] >= 1 and n["inverse"] == n["inverse finite, 2 parameters"]  # on regular Hessians
    monkeypatch.setattr(lk, "MAX_ITER", lk.MAX_ITER - 1)  # one iteration fewer loses that track
    c = EC.cases()["faded"]
    fewer = LC.run_case(c["det"], c["opts"], EC.frames("faded"), c["border"])[1]
    assert fewer["counts"][1, 0] < last["counts"][1, 0]


def test_last_template_and_gain(census):
    n, T, last = census("drift_last_template")
    assert n["inverse"] > 3 * last["counts"][0, 1]                 # templates are renewed in every frame
    assert not np.array_equal(np.array([T.template_px[t.buffer_id] for t in T.book.tracks], F), last["first_pos"].view(F))
    for name in ("gain_dimmed_01", "gain_dimmed_11"):
        n, T, last = census(name)
        alpha = np.array([T.ab[t.buffer_id][0] for t in T.book.tracks], F)
        assert last["counts"][-1, 0] > 20 and (np.abs(alpha) > 0.05).sum() > 10, name  # 1 + alpha is far from 1


@pytest.mark.parametrize("name", EC.LEVELS)
def test_level_ranges(census, name):
    n, T, last = census(name)
    opt = T.opt
    levels = range(opt.klt_min_level, opt.klt_max_level + 1)
    assert T.invh.shape[1] == len(levels) < 5
    used = {opt.klt_patch_sizes[l] for l in levels}
    assert {int(k.split()[-1]) for k in n if k.startswith("level runs")} == used
    assert sum(v for k, v in n.items() if k.endswith(": fits") or k.endswith(": does not fit")) == last["counts"][0, 1] * len(levels)
    assert last["counts"][-1, 0] > 20
    if name == "levels_0_2_deep":
        assert opt.pyramid_levels > opt.klt_max_level + 1 and max(opt.klt_patch_sizes) > max(used)


def test_bundle():
    with EC.Census() as cen:
        B, per_call, counts = EC.bundle_uncached()
    per_cam = []
    for cam in range(len(EC.BUNDLE["cameras"])):  # the same cameras alone, for the per-camera conditions
        with EC.Census() as one:
            LC.run_case(EC.BUNDLE["det"], EC.BUNDLE["opts"], [call[cam] for call in EC.bundle_images()], EC.BUNDLE["border"])
        per_cam.append(one.n)
    assert 2 <= len(per_cam) <= 3
    assert _exits(per_cam[0], EXITS[3]) >= 1                      # camera 0 leaves through its last row ...
    assert per_cam[1]["isnan(x) exit of the iteration loop"] >= 1  # ... above camera 1's first, whose tracks die of NaN
    assert sum(cen.n.values()) == sum(sum(n.values()) for n in per_cam)
    assert all(t > 0 for call in counts[1:] for t, _ in call)
