"""GPU (-m gpu): the search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame / a two-fisheye rig on the
device -- vslam_fuse_search_rig[_async/_wait], k_fuse_rank_rig -- equal, integer for integer, to tests/fuse_rig_ref.py
(fmatcher.cpp:1918-2119 with NLeft != -1, :2121-2243) over tests/fuse_rig_cases.py: blocking and async, from host and from device
points; a 6-job call against six 1-job calls; a blocking rig matcher between _async and _wait; the refusals."""
import numpy as np
import pytest

import frustum_cases as HC
import fuse_rig_cases as FC
import vi_slam_amd as V

pytestmark = pytest.mark.gpu
SERVED = [n for n in sorted(FC.cases()) if FC.cases()[n]["refuse"] is None]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def ctx():
    """one context with the left KB8 camera set; every keypoint / descriptor array of the cases goes to HBM once"""
    import torch
    g = FC.golden()
    fe = V.FExtractor(HC.HUT_NF, 1.2, 8, 20, 7, HC.HUT_W, HC.HUT_H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), g["sf"])
    fe.set_kb8_camera(V.kb8_camera(*FC.CAM1))
    c = dict(fe=fe, dev={}, rig=V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"]))
    yield c
    torch.cuda.synchronize()
    fe.close()


def dev_of(ctx, a, dtype):
    """the device copy of a case array, made once per array"""
    import torch
    key = (id(a), len(a))
    if key not in ctx["dev"]:
        ctx["dev"][key] = (_dev(np.ascontiguousarray(a, dtype)), a)  # the array is kept: its id stays its own
        torch.cuda.synchronize()
    return ctx["dev"][key][0].data_ptr()


def jobs_of(ctx, c, only=None):
    out = []
    for j in (c["jobs"] if only is None else [c["jobs"][only]]):
        n = len(j["kps"])
        out.append(V.fuse_rig_job(*j["pose"], dev_of(ctx, j["kps"], V.KP_DTYPE) if n else 0,
                                  dev_of(ctx, j["desc"], np.uint8) if n else 0, n, j["camera"], j["idx_offset"], j["valid"], j["sim3"]))
    return out


def run(ctx, c, mode="blocking", only=None):
    fe = ctx["fe"]
    jobs = jobs_of(ctx, c, only)
    a = (ctx["rig"], jobs, c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG, c["gf"])
    if mode == "blocking":
        return fe.fuse_search_rig(*a)
    if mode == "device" and len(c["pts"]):
        import torch
        p, d = _dev(np.ascontiguousarray(c["pts"], V.FUSE_POINT_DTYPE)), _dev(np.ascontiguousarray(c["desc"], np.uint8))
        torch.cuda.synchronize()
        fe.fuse_search_rig_async(ctx["rig"], jobs, p.data_ptr(), d.data_ptr(), c["th"], FC.LSF, FC.IMG, c["gf"], n_points=len(c["pts"]))
        return fe.fuse_search_rig_wait()  # p, d live until here
    fe.fuse_search_rig_async(*a)
    return fe.fuse_search_rig_wait()


def assert_same(got, want, what):
    bad = np.argwhere((got[0] != want[0]) | (got[1] != want[1]))
    assert got[0].shape == want[0].shape and len(bad) == 0, (what, bad[:6], [(got[0][tuple(b)], want[0][tuple(b)]) for b in bad[:6]])


@pytest.mark.parametrize("name", SERVED)
def test_every_case(ctx, name):
    c = FC.cases()[name]
    want = FC.reference(name)
    for mode in ("blocking", "async", "device"):
        assert_same(run(ctx, c, mode), want, (name, mode))


def test_six_jobs_equal_six_single_jobs(ctx):
    c = FC.cases()["scene"]
    all_i, all_d = run(ctx, c)
    for j in range(6):
        bi, bd = run(ctx, c, only=j)
        assert np.array_equal(bi[0], all_i[j]) and np.array_equal(bd[0], all_d[j]), j
    assert (all_i >= 0).sum() > 1000


def test_refusals_enqueue_nothing(ctx):
    fe = ctx["fe"]
    for name, code in (("jobs17", V.ERR_INVALID), ("kf4097", V.ERR_UNSUPPORTED)):
        c = FC.cases()[name]
        with pytest.raises(V.VslamError) as ei:
            run(ctx, c)
        assert ei.value.code == code, name
        bi, bd = fe.last_fuse_rig_outputs  # the outputs of a refused call, all n_jobs * n_points of them: -1 / 256
        assert len(bi) == len(c["jobs"]) * len(c["pts"]) > 0
        assert (bi == -1).all() and (bd == 256).all(), name
        with pytest.raises(V.VslamError):
            fe.fuse_search_rig_wait()  # nothing was enqueued
    n = V.LOCAL_POINTS_MAX + 1
    c = FC.cases()["np1"]
    with pytest.raises(V.VslamError) as ei:
        fe.fuse_search_rig(ctx["rig"], jobs_of(ctx, dict(c, jobs=[dict(c["jobs"][0], valid=None)])), np.zeros(n, V.FUSE_POINT_DTYPE),
                           np.zeros((n, 32), np.uint8), c["th"], FC.LSF, FC.IMG)
    assert ei.value.code == V.ERR_UNSUPPORTED
    assert (fe.last_fuse_rig_outputs[0] == -1).all() and (fe.last_fuse_rig_outputs[1] == 256).all()
    # camera 1 without a rig; a sim3 job on the right camera
    with pytest.raises(V.VslamError) as ei:
        fe.fuse_search_rig(None, jobs_of(ctx, c), c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG)
    assert ei.value.code == V.ERR_INVALID
    bad = dict(c, jobs=[dict(c["jobs"][1], sim3=True)])
    with pytest.raises(V.VslamError) as ei:
        run(ctx, bad)
    assert ei.value.code == V.ERR_INVALID
    # descriptor rows that are not 16-byte aligned (the kernel reads them 16 bytes at a time)
    j = c["jobs"][0]
    off = V.fuse_rig_job(*j["pose"], dev_of(ctx, j["kps"], V.KP_DTYPE), dev_of(ctx, j["desc"], np.uint8) + 8, len(j["kps"]) - 1)
    with pytest.raises(V.VslamError) as ei:
        fe.fuse_search_rig(None, [off], c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG)
    assert ei.value.code == V.ERR_INVALID
    # a left-only call needs no rig
    mono = FC.cases()["mono"]
    got = fe.fuse_search_rig(None, jobs_of(ctx, mono), mono["pts"], mono["desc"], mono["th"], FC.LSF, FC.IMG)
    assert_same(got, FC.reference("mono"), "mono without a rig")
    # without a KB8 camera the entry refuses
    fe.set_kb8_camera(None)
    try:
        with pytest.raises(V.VslamError) as ei:
            run(ctx, c)
        assert ei.value.code == V.ERR_INVALID
    finally:
        fe.set_kb8_camera(V.kb8_camera(*FC.CAM1))
    assert_same(run(ctx, c), FC.reference("np1"), "after the refusals")


def test_pinhole_fuse_still_refuses_with_a_kb8_camera(ctx):
    fe, c = ctx["fe"], FC.cases()["np16"]
    j = c["jobs"][0]
    m = V.FMatcher(fe)
    with pytest.raises(V.VslamError) as ei:
        m.FuseSearch(c["pts"], c["desc"], dev_of(ctx, j["kps"], V.KP_DTYPE), dev_of(ctx, j["desc"], np.uint8), len(j["kps"]), None,
                     *j["pose"], FC.CAM1[:4] + (0.0,), c["th"], FC.LSF, FC.IMG)
    assert ei.value.code == V.ERR_UNSUPPORTED


def test_async_with_a_blocking_rig_matcher_in_between_and_one_in_flight(ctx):
    """a blocking vslam_search_by_projection_mappoints_rig between _async and _wait fills the shared staging block of the
    blocking matchers: both results are intact; a second _async is refused"""
    fe, c = ctx["fe"], FC.cases()["scene"]
    want = FC.reference("scene")
    g = FC.golden()
    alone = _mappoints_rig(ctx, g)
    assert alone[0] > 50
    jobs = jobs_of(ctx, c)
    a = (ctx["rig"], jobs, c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG, c["gf"])
    fe.fuse_search_rig_async(*a)
    with pytest.raises(V.VslamError) as ei:  # one search per context
        fe.fuse_search_rig_async(*a)
    assert ei.value.code == V.ERR_INVALID
    between = _mappoints_rig(ctx, g)
    got = fe.fuse_search_rig_wait()
    assert_same(got, want, "with a blocking matcher in between")
    assert between[0] == alone[0] and np.array_equal(between[1], alone[1])
    with pytest.raises(V.VslamError):
        fe.fuse_search_rig_wait()  # nothing enqueued any more
    assert_same(run(ctx, c, "async"), want, "afterwards")


def _mappoints_rig(ctx, g):
    """SearchByProjection(F, vpMapPoints) of a rig from hand-made records: one MapPoint on every eighth keypoint of each side"""
    fe = ctx["fe"]
    nl, nr = len(g["kl"]), len(g["kr"])
    sel_l, sel_r = np.arange(0, nl, 8), np.arange(0, nr, 8)
    n = len(sel_l) + len(sel_r)
    tl, tr = np.zeros(n, V.MP_TRACK_DTYPE), np.zeros(n, V.MP_TRACK_DTYPE)
    tl["level"], tr["level"] = -1, -1
    for k, i in enumerate(sel_l):
        tl[k] = (g["kl"]["x"][i], g["kl"]["y"][i], 0.0, 1.0, g["kl"]["octave"][i], 3)
    for k, i in enumerate(sel_r):
        tr[len(sel_l) + k] = (g["kr"]["x"][i], g["kr"]["y"][i], 0.0, 1.0, g["kr"]["octave"][i], 3)
    desc = np.concatenate([g["dl"][sel_l], g["dr"][sel_r]])
    frame = V.rig_frame(dev_of(ctx, g["kl"], V.KP_DTYPE), dev_of(ctx, g["dl"], np.uint8), nl, dev_of(ctx, g["kr"], V.KP_DTYPE),
                        dev_of(ctx, g["dr"], np.uint8), nr, np.full(nl, -1, np.int32), np.full(nr, -1, np.int32))
    return fe.search_by_projection_mappoints_rig(tl, tr, desc, frame, 1.0, 0.8, FC.IMG)


def test_profile_getter(ctx):
    fe, c = ctx["fe"], FC.cases()["np17"]
    fe.set_profiling(True)
    try:
        run(ctx, c)
        run(ctx, c, "async")
        ms, n = fe.get_fuse_rig_profile()
    finally:
        fe.set_profiling(False)
    assert n == 2 and ms > 0
