"""The gate tables of tests/matcher_gate_cases.py on the CPU: for every row the hand-written expectation, the oracle
(oracle/orb_oracle.cpp) and the numpy restatement over integer bounds (tests/projection_bounds_ref.py) agree; the exit the
restatement records is the row's gate, i.e. the inputs bite where they say; every `on` row has an `inside` and an
`outside` sibling and does not behave like both of them; and the rows built to land on a literal carry exactly that float.

One-sided gates, where no value exists beyond the boundary, are listed in ONE_SIDED with the reason."""
import numpy as np
import pytest

import matcher_gate_cases as G
import projection_bounds_ref as R

F32 = np.float32
TABLES = sorted(G.BUILDERS)
RUNS = [(name, k) for name in TABLES for k in range(len(G.table(name).runs))]
# `on` rows without a sibling on both sides
ONE_SIDED = {
    "dist-256": "256 is the greatest Hamming distance of 256-bit descriptors: nothing lies beyond bestDist's initial value",
}

_res = {}


def results(name, k):
    """(oracle result, numpy result, numpy stats) of one run, computed once"""
    if (name, k) not in _res:
        t = G.table(name)
        run = t.runs[k]
        stats = {}
        _res[(name, k)] = (G.reference(t, run, "orbo"), G.reference(t, run, "numpy", stats), stats)
    return _res[(name, k)]


@pytest.mark.parametrize("name", TABLES)
def test_tables_stay_small_and_rows_are_well_formed(name):
    t = G.table(name)
    assert 0 < len(t.rows) <= G.MAX_ROWS and len(t.kps) <= G.MAX_KPS
    for r in t.rows:
        assert r["side"] in ("inside", "on", "outside", "non-finite"), r
        assert r["line"] and r["gate"], r
        for e in (r["exit"].values() if isinstance(r["exit"], dict) else [r["exit"]]):
            assert e is None or e in R.EXITS + R.TRI_EXITS, r


@pytest.mark.parametrize("name", [n for n in TABLES if n != "triangulation"])
def test_no_row_sees_another_rows_keypoints(name):
    """every keypoint within the largest window of a row's projection is one of the row's own"""
    t = G.table(name)
    a = G.inputs(t)
    for i, r in enumerate(t.rows):
        if "pos" in r:
            with np.errstate(all="ignore"):
                u, v = G.project(abs(r["pos"][0]) if r["pos"][2] < 0 else r["pos"][0], G.FX, G.CX, abs(r["pos"][2])), \
                    G.project(abs(r["pos"][1]) if r["pos"][2] < 0 else r["pos"][1], G.FY, G.CY, abs(r["pos"][2]))
        else:
            u, v = r["proj_x"], r["proj_y"]
        if not (np.isfinite(u) and np.isfinite(v)):
            continue
        th = float(t.runs[-1].get("th", getattr(t, "th", 0)))
        sf = G.tables()["scale"]  # the widest window the row can have: its own level's where the row sets the level
        rad = th * 4.0 * float(sf[r["level"]]) if name == "mappoints" else th * float(sf[-1])
        near = np.nonzero((np.abs(a["kps"]["x"] - u) < rad) & (np.abs(a["kps"]["y"] - v) < rad))[0]
        assert set(near) <= set(r["own"]), (i, r["gate"], near, r["own"])


@pytest.mark.parametrize("name,k", RUNS)
def test_expectation_oracle_and_restatement_agree(name, k):
    t = G.table(name)
    run = t.runs[k]
    o, n, _ = results(name, k)
    assert G.same(o, n), (name, run["name"])
    got = G.per_row(t, o)
    want = t.expected(run)
    bad = [(i, t.rows[i]["gate"], t.rows[i]["side"], t.rows[i]["group"], int(got[i]), w)
           for i, w in enumerate(want) if w is not None and got[i] != w]
    assert not bad, (name, run["name"], bad)
    if run is t.runs[0]:
        assert sum(w is not None for w in want) >= 0.8 * len(want)


@pytest.mark.parametrize("name,k", RUNS)
def test_recorded_exit_is_the_rows_gate(name, k):
    t = G.table(name)
    run = t.runs[k]
    stats = results(name, k)[2]
    want = t.exits(run)
    bad = [(i, t.rows[i]["gate"], t.rows[i]["side"], stats["exit"].get(i), w) for i, w in enumerate(want)
           if w is not None and stats["exit"].get(i) != w]
    assert not bad, (name, run["name"], bad)
    # every exit of the form is taken by some row of its table (first run; the later runs move rows between exits)
    if k == 0:
        taken = set(stats["exit"].values())
        assert "accepted" in taken and len(taken) >= 5, taken


@pytest.mark.parametrize("name,k", RUNS)
def test_every_on_row_has_siblings_and_differs_from_one(name, k):
    t = G.table(name)
    run = t.runs[k]
    out = t.outcome(G.per_row(t, results(name, k)[0]))
    want = t.expected(run)
    assert -2 not in out  # nobody matched another row's keypoint
    if not t.sided(run):  # the rows name their sides for the table's plain runs (Table.sided)
        return
    groups = {}
    for i, r in enumerate(t.rows):
        groups.setdefault(r["group"], []).append(i)
    n_on = 0
    for g, rows in groups.items():
        ons = [i for i in rows if t.rows[i]["side"] == "on" and want[i] is not None]
        if not ons or g in ONE_SIDED:
            continue
        sides = {s: [i for i in rows if t.rows[i]["side"] == s and want[i] is not None] for s in ("inside", "outside")}
        assert sides["inside"] and sides["outside"], (name, g)
        for i in ons:
            n_on += 1
            assert any(out[j] != out[i] for j in sides["inside"] + sides["outside"]), (name, run["name"], g, i)
    if k == 0:
        assert n_on >= 5


@pytest.mark.parametrize("name", [n for n in TABLES if n not in ("triangulation", "mappoints")])
def test_bound_rows_project_onto_the_bound_and_one_float_beside_it(name):
    t = G.table(name)
    seen = 0
    for r in t.rows:
        if "proj" not in r:
            continue
        axis, want, bound = r["proj"]
        f, c = (G.FX, G.CX) if axis == 0 else (G.FY, G.CY)
        got = G.project(r["pos"][axis], f, c)
        assert got == want
        lower = bound == 0
        inward = np.inf if lower else -np.inf
        beside = {"on": F32(bound), "inside": np.nextafter(F32(bound), F32(inward)),
                  "outside": np.nextafter(F32(bound), F32(-inward))}[r["side"]]
        if lower and r["side"] != "on":  # around 0 one step of the projection is one float of cx, not of 0
            beside = F32(bound) + (np.nextafter(c, F32(np.inf)) - c) * (1 if r["side"] == "inside" else -1)
        assert got == beside, (name, r["group"], r["side"], got, beside)
        seen += 1
    assert seen == 12


def test_chi_square_rows_carry_the_literals_float():
    t = G.table("fuse")
    stats = results("fuse", 0)[2]
    seen = []
    for i, r in enumerate(t.rows):
        if "chi2" not in r:
            continue
        got = stats["chi2"][(i, r["own"][0])]
        assert got.dtype == np.float32 and got == r["chi2"], (i, got, r["chi2"])
        seen.append((r["group"], r["side"], float(got)))
    lit = {"chi2-7.8": 7.8, "chi2-5.99": 5.99}
    for g, side, v in seen:
        f = F32(lit[g])
        assert v == float({"inside": np.nextafter(f, F32(0)), "on": f, "outside": np.nextafter(f, F32(9))}[side])
    assert len(seen) == 6
    # what makes the literal's type matter: 7.8f lies above 7.8, 5.99f below 5.99
    assert float(F32(7.8)) > 7.8 and float(F32(5.99)) < 5.99 < float(np.nextafter(F32(5.99), F32(9)))


def test_view_cos_rows_carry_the_literals_float():
    t = G.table("mappoints")
    vals = sorted({float(r["view_cos"]) for r in t.rows if r["group"].startswith("viewcos")})
    f = F32(0.998)
    assert vals == [float(np.nextafter(f, F32(0))), float(f), float(np.nextafter(f, F32(1)))]
    assert vals[0] < 0.998 < vals[1]
    a = G.inputs(t)
    assert a["mps"]["view_cos"].dtype == np.float32


def test_epipolar_and_epipole_rows_carry_the_literals_float():
    t = G.table("triangulation")
    stats = results("triangulation", 0)[2]
    sig2, sf = G.tables()["sigma2"], G.tables()["scale"]
    assert sig2[0] == 1 and sf[0] == 1
    n = 0
    for i, r in enumerate(t.rows):
        if "dsqr" in r:
            got = stats["dsqr"][(i, r["own"][0])]
            assert got.dtype == np.float32 and got == r["dsqr"]
            if r["side"] == "on":
                assert got == F32(3.84) and float(got) < 3.84
            if r["side"] == "outside":
                assert float(got) > 3.84
            n += 1
        if "epi" in r and (i, r["own"][0]) in stats.get("epi", {}):
            got = stats["epi"][(i, r["own"][0])]
            assert got == r["epi"]
            assert (got == 100) == (r["side"] == "on") and (got < 100) == (r["side"] == "outside")
            n += 1
    assert n == 6


def test_window_and_ratio_rows_sit_on_their_edge():
    for name in TABLES:
        for r in G.table(name).rows:
            if r["gate"] == "window":
                d = {"inside": -1, "on": 0, "outside": 1}[r["side"]]
                assert np.sign(float(r["dx"]) - float(r["radius"])) == d, (name, r["side"])
            if "ratio" in r:
                side, ratio = r["ratio"]
                got = F32(F32(r["max_distance"]) / F32(r["d3"]))
                assert {"inside": got < ratio, "on": got == ratio, "outside": got > ratio}[side], (name, side, got)
    assert np.ceil(F32(R.orbo.logf(float(F32(1.2)))) / F32(G.LSF)) == 1  # ratio == 1.2f is still level 1


def test_frame_runs_take_the_direction_they_name():
    t = G.table("frame")
    for run in t.runs:
        fwd, bwd = R.projection_direction(G.POSE, G.frame_tlw(run), G.MB, run["mono"], not run["gemm_float"])
        assert {"none": (False, False), "fwd": (True, False), "bwd": (False, True)}[run["kind"]] == (fwd, bwd), run
    # tlc.z == mb is not forward; one float above is; and mono overrides both
    names = {r["name"]: r for r in t.runs}
    assert names["on"]["tlw_z"] == G.MB and names["fwd"]["tlw_z"] == np.nextafter(G.MB, F32(1))
    assert names["mono"]["tlw_z"] == names["fwd"]["tlw_z"] and names["mono-bwd"]["tlw_z"] == names["bwd"]["tlw_z"]


def test_zero_depth_of_either_sign_arrives_as_plus_zero():
    """Rcw * p + tcw accumulates from +0.0, so a point at z = -0.0 is zc = +0.0 at the depth gate, in both gemm forms"""
    for name in ("frame", "fuse", "sim3dir"):
        rows = [r for r in G.table(name).rows if "zc" in r]
        assert sorted(np.signbit(r["zc"]) for r in rows) == [False, True]
        for r in rows:
            for dbl in (True, False):
                z = R._gemm_row(G.POSE[2, :3], r["pos"], G.POSE[2, 3], dbl)
                assert z == 0 and not np.signbit(z), (name, r["zc"], z)
