"""GPU (-m gpu): the gate tables of tests/matcher_gate_cases.py through the device matchers -- k_sbp_rank, k_sbp_resolve,
k_sbpm_resolve, the replay kernels, k_fuse_rank and k_stri_queries -- array_equal to the oracle on every row, for both gemm
forms, under the sequential and short-prefix tunings, and SearchBySim3's directions through both of their entry points.
tests/test_matcher_gates_cpu.py vouches for the tables: what each row expects, and that it leaves at the gate it names."""
import numpy as np
import pytest

import matcher_gate_cases as G
import vi_slam_amd as V

pytestmark = pytest.mark.gpu

TABLES = sorted(G.BUILDERS)
_want = {}


def want(name, k):
    if (name, k) not in _want:
        t = G.table(name)
        _want[(name, k)] = G.reference(t, t.runs[k], "orbo")
    return _want[(name, k)]


@pytest.fixture(scope="module")
def ctx():
    """one 640 x 480 context; per table the keypoints, descriptors and right coordinates as device tensors"""
    import torch
    fe = V.FExtractor(1000, 1.2, 8, 20, 7, G.W, G.H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), G.tables()["scale"])
    assert np.array_equal(fe.GetInverseScaleSigmaSquares(), G.tables()["inv_sigma2"])
    assert np.array_equal(fe.GetScaleSigmaSquares(), G.tables()["sigma2"])
    dev = {}
    for name in TABLES:
        a = G.inputs(G.table(name))
        n = len(a["kps"])
        d = dict(kps=torch.from_numpy(a["kps"].view(np.uint8).reshape(n, -1).copy()).cuda(),
                 desc=torch.from_numpy(np.ascontiguousarray(a["desc"])).cuda(),
                 u_right=torch.from_numpy(a["u_right"].copy()).cuda(), occupied=torch.from_numpy(a["occupied"].copy()).cuda(),
                 desc_q=torch.from_numpy(np.ascontiguousarray(a["desc_q"])).cuda(), n=n)
        dev[name] = d
    torch.cuda.synchronize()
    yield dict(fe=fe, dev=dev)
    fe.set_tuning(sbp_sequential=0, sbp_topm=8)
    fe.close()


def device(ctx, name, run):
    """one run of a table on the device, in the shape matcher_gate_cases.reference returns it"""
    t = G.table(name)
    a, d, fe = G.inputs(t), ctx["dev"][name], ctx["fe"]
    kp, dp, n = d["kps"].data_ptr(), d["desc"].data_ptr(), d["n"]
    size = (G.W, G.H)
    gf = run.get("gemm_float", False)
    I3, z3 = G.POSE[:, :3], G.POSE[:, 3]
    if name == "frame":
        m = V.FMatcher(fe, 0.9, True)
        return m.SearchByProjection(G.POSE, G.frame_tlw(run), G.CAM + (float(G.BF), float(G.MB)), t.th, a["q_kps"], a["flags"],
                                    a["x3dw"], a["desc_q"], kp, dp, n, a["u_right"], run["mono"], size, a["occupied"], gf)
    if name == "keyframe":
        m = V.FMatcher(fe, 0.9, True)
        return m.SearchByProjectionKeyFrame(G.POSE, G.OW, G.CAM, t.th, run["orb_dist"], G.LSF, a["q_kps"], a["flags"],
                                            a["x3dw"], a["mn"], a["mx"], a["desc_q"], kp, dp, n, a["occupied"], size, gf)
    if name == "mappoints":
        m = V.FMatcher(fe, t.nnratio, True)
        return m.SearchByProjectionMapPoints(a["mps"], a["desc_q"], kp, dp, n, a["u_right"], float(run["th"]), a["occupied"],
                                             size)
    p = a.get("pts")
    if name == "sim3proj":
        m = V.FMatcher(fe, 0.9, True)
        return m.SearchByProjectionSim3(G.POSE, G.OW, G.CAM, t.th, run["ratio"], G.LSF, p["valid"].astype(np.uint8), p["pos"],
                                        p["normal"], p["min_distance"], p["max_distance"], a["desc_q"], kp, dp, n,
                                        a["occupied"], size, run["variant"], gf)
    if name in ("fuse", "fuse_sim3"):
        m = V.FMatcher(fe, 0.6, True)
        return m.FuseSearch(p, a["desc_q"], kp, dp, n, a["u_right"], I3, z3, G.OW, G.CAM + (float(G.BF),), t.th, G.LSF, size,
                            name == "fuse_sim3", gf)
    if name == "sim3dir":
        m = V.FMatcher(fe, 0.75, True)
        b, e = m.FuseSearch(p, a["desc_q"], kp, dp, n, None, I3, z3, z3, G.CAM + (0.0,), t.th, G.LSF, size, 2, gf, I3, z3)
        return (np.where((b >= 0) & (e <= 100), b, -1),)
    if name == "triangulation":
        m = V.FMatcher(fe, 0.6, True)
        nm, pairs, m12 = m.SearchForTriangulation(a["kps1"], ctx["dev"][name]["desc_q"].data_ptr(), a["mp1"], a["ur1"], a["fv1"],
                                                  a["kps"], dp, a["occupied"], a["u_right"], a["fv2"], t.F12, t.ep,
                                                  run["only_stereo"], run["coarse"])
        assert len(pairs) == nm and np.array_equal(pairs[:, 1], m12[pairs[:, 0]])
        return nm, m12
    raise KeyError(name)


def differing_rows(t, got, ref):
    g, w = G.per_row(t, got), G.per_row(t, ref)
    return [(i, t.rows[i]["gate"], t.rows[i]["side"], t.rows[i]["group"], int(g[i]), int(w[i])) for i in np.nonzero(g != w)[0]]


@pytest.mark.parametrize("name", TABLES)
def test_every_row_of_every_run_equals_the_oracle(ctx, name):
    """both gemm_float settings are among each table's runs (the local-map and triangulation forms take no pose)"""
    t = G.table(name)
    for k, run in enumerate(t.runs):
        got, ref = device(ctx, name, run), want(name, k)
        assert not differing_rows(t, got, ref), (name, run["name"])
        assert G.same(got, ref), (name, run["name"])
    if name not in ("mappoints", "triangulation"):
        assert {bool(r["gemm_float"]) for r in t.runs} == {False, True}


@pytest.mark.parametrize("tune", [dict(sbp_sequential=1), dict(sbp_topm=1), dict(sbp_topm=2)])
@pytest.mark.parametrize("name", ["frame", "mappoints", "keyframe", "sim3proj"])
def test_sequential_and_short_prefix_paths(ctx, name, tune):
    """k_sbp_replay / k_sbpm_replay and their full re-scans decide the same rows"""
    fe = ctx["fe"]
    t = G.table(name)
    fe.set_tuning(**tune)
    try:
        for k, run in enumerate(t.runs):
            got, ref = device(ctx, name, run), want(name, k)
            assert not differing_rows(t, got, ref), (name, run["name"], tune)
            assert G.same(got, ref), (name, run["name"], tune)
    finally:
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)


def sim3_pair(t, ref1):
    """SearchBySim3's two KeyFrames from the sim3dir table: KeyFrame 1 owns the table's MapPoints, one keypoint per row at
    the row's projection with the row's descriptor; KeyFrame 2 owns the table's keypoints, and the keypoint that direction 1
    gives a row carries that row's MapPoint, so that direction 2 looks for the row from the other side"""
    a = G.inputs(t)
    p = a["pts"]
    k1 = np.zeros(len(p), G.orbo.KP_DTYPE)
    with np.errstate(all="ignore"):
        k1["x"] = np.nan_to_num(np.clip(G.FX * p["pos"][:, 0] / p["pos"][:, 2] + G.CX, 1, G.W - 2), nan=1.0)
        k1["y"] = np.nan_to_num(np.clip(G.FY * p["pos"][:, 1] / p["pos"][:, 2] + G.CY, 1, G.H - 2), nan=1.0)
    k1["octave"], k1["size"] = 1, 31.0
    pts2 = np.zeros(len(a["kps"]), G.orbo.FUSE_POINT_DTYPE)
    for i, j in enumerate(ref1):
        if j >= 0:
            pts2[j] = p[i]
            k1["octave"][i] = a["kps"]["octave"][j]  # inside the level window the row's MapPoint predicts
    return k1, pts2


def test_sim3_directions_through_search_by_sim3(ctx):
    import torch
    t = G.table("sim3dir")
    a, d, fe = G.inputs(t), ctx["dev"]["sim3dir"], ctx["fe"]
    I3, z3 = G.POSE[:, :3], G.POSE[:, 3]
    p, n2 = a["pts"], d["n"]
    for k, run in enumerate(t.runs):
        gf = run["gemm_float"]
        ref1 = want("sim3dir", k)[0]
        k1, pts2 = sim3_pair(t, ref1)
        dk1 = torch.from_numpy(k1.view(np.uint8).reshape(len(k1), -1).copy()).cuda()
        m = V.FMatcher(fe, 0.75, True)
        nf, m12, (sR21, t21, sR12) = m.SearchBySim3(p, a["desc_q"], dk1.data_ptr(), d["desc_q"].data_ptr(), len(p), I3, z3, pts2,
                                                    a["desc"], d["kps"].data_ptr(), d["desc"].data_ptr(), n2, I3, z3, 1.0, I3,
                                                    z3, t.th, G.CAM, G.LSF, (G.W, G.H), gf)
        wn, wm = G.orbo.search_by_sim3(p["valid"], p["pos"], p["min_distance"], p["max_distance"], a["desc_q"], k1, I3, z3,
                                       pts2["valid"], pts2["pos"], pts2["min_distance"], pts2["max_distance"], a["desc"],
                                       a["kps"], I3, z3, sR12, z3, sR21, t21, G.CAM, t.th, G.LSF, G.tables()["scale"], G.W,
                                       G.H, not gf)
        assert nf == wn and np.array_equal(m12, wm), run["name"]
        # the pairs that survive the agreement check are direction 1's, and most of its matches survive
        assert np.all((m12 == ref1) | (m12 == -1)) and wn >= 20, (wn, ref1)


def test_frame_table_device_resident(ctx):
    """the batch form: last-frame side, right coordinates and occupancy all in device memory, two jobs in one call"""
    import torch
    t = G.table("frame")
    a, d, fe = G.inputs(t), ctx["dev"]["frame"], ctx["fe"]
    nq = len(t.rows)
    qk = torch.from_numpy(a["q_kps"].view(np.uint8).reshape(nq, -1).copy()).cuda()
    fl = torch.from_numpy(a["flags"].copy()).cuda()
    X = torch.from_numpy(np.ascontiguousarray(a["x3dw"])).cuda()
    nl = torch.tensor([nq], dtype=torch.int32, device="cuda")
    nc = torch.tensor([d["n"]], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ks = [k for k, r in enumerate(t.runs) if r["name"] in ("on", "fwd-f")]
    jobs = []
    for k in ks:
        run = t.runs[k]
        fwd, bwd = G.R.projection_direction(G.POSE, G.frame_tlw(run), G.MB, run["mono"], not run["gemm_float"])
        jobs.append(dict(Tcw=G.POSE, cam=G.CAM + (float(G.BF),), th=t.th, forward=fwd, backward=bwd, img=(G.W, G.H),
                         gemm_float=run["gemm_float"], last_kps=qk.data_ptr(), n_last=nl.data_ptr(), last_flags=fl.data_ptr(),
                         last_x3dw=X.data_ptr(), mp_desc=d["desc_q"].data_ptr(), cur_kps=d["kps"].data_ptr(),
                         cur_desc=d["desc"].data_ptr(), n_cur=nc.data_ptr(), cur_u_right=d["u_right"].data_ptr(),
                         cur_occupied=d["occupied"].data_ptr()))
    m = V.FMatcher(fe, 0.9, True)
    m.search_by_projection_dev_async(jobs)
    out = m.search_by_projection_dev_wait([d["n"]] * len(jobs))
    for (nm, mc), k in zip(out, ks):
        ref = want("frame", k)
        assert nm == ref[0] and np.array_equal(mc, ref[1]), t.runs[k]["name"]
