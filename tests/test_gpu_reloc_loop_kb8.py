"""GPU (-m gpu): the relocalisation and the loop-closing SearchByProjection for fisheye cameras on the device --
vslam_search_by_projection_keyframe_kb8 (k_sbp_rank_kb8 mode 2) and vslam_search_by_projection_sim3_kb8[_async/_wait] (k_s3k_gate,
k_s3k_compact, k_sbp_rank_kb8 mode 3, k_sbp_resolve / k_sbp_replay, k_s3k_finish) -- equal, integer for integer, to
tests/reloc_loop_kb8_ref.py (fmatcher.cpp:2689-2811, :750-863) over tests/reloc_loop_kb8_cases.py.  A: default tuning, the
sequential wave (sbp_sequential = 1) and a sorted prefix of one entry (sbp_topm = 1).  B: blocking and async, from host and from
device points; a 6-job call against six 1-job calls; a blocking rig matcher between _async and _wait; the refusals."""
import numpy as np
import pytest

import frustum_cases as HC
import reloc_loop_kb8_cases as RC
import vi_slam_amd as V

pytestmark = pytest.mark.gpu
B_SERVED = [n for n in sorted(RC.b_cases()) if RC.b_cases()[n]["refuse"] is None]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def ctx():
    """one context with the KB8 camera of the B cases set; every keypoint / descriptor array of the cases goes to HBM once"""
    import torch
    g = RC.golden()
    fe = V.FExtractor(HC.HUT_NF, 1.2, 8, 20, 7, HC.HUT_W, HC.HUT_H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), g["sf"])
    fe.set_kb8_camera(V.kb8_camera(*RC.CAM1))
    c = dict(fe=fe, dev={})
    yield c
    torch.cuda.synchronize()
    fe.close()


def dev_of(ctx, a, dtype):
    import torch
    key = (id(a), len(a))
    if key not in ctx["dev"]:
        ctx["dev"][key] = (_dev(np.ascontiguousarray(a, dtype)), a)  # the array is kept: its id stays its own
        torch.cuda.synchronize()
    return ctx["dev"][key][0].data_ptr()


# ------------------------------------------------------------------------------------------------ A
def run_a(ctx, c, tuning=None, proj_cam=None):
    fe = ctx["fe"]
    m = V.FMatcher(fe, checkOri=c["check_ori"])
    fe.set_kb8_camera(V.kb8_camera(*c["cam"]))
    if tuning:
        fe.set_tuning(**tuning)
    try:
        n = len(c["cur_kps"])
        return m.SearchByProjectionKeyFrameKB8(c["T"], c["Ow"], proj_cam or c["cam"][:4], c["th"], c["orb_dist"], RC.LSF,
                                               c["kf_kps"], c["flags"], c["x3dw"], c["mn"], c["mx"], c["desc"],
                                               dev_of(ctx, c["cur_kps"], V.KP_DTYPE), dev_of(ctx, c["cur_desc"], np.uint8), n,
                                               c["occupied"], RC.IMG, c["gf"])
    finally:
        if tuning:
            fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        fe.set_kb8_camera(V.kb8_camera(*RC.CAM1))


@pytest.mark.parametrize("tuning", [None, dict(sbp_sequential=1), dict(sbp_topm=1)], ids=["default", "sequential", "topm1"])
@pytest.mark.parametrize("name", sorted(RC.a_cases()))
def test_a_every_case(ctx, name, tuning):
    nm, m = run_a(ctx, RC.a_cases()[name], tuning)
    want = RC.reference_a(name)
    assert nm == want[0] and np.array_equal(m, want[1]), (name, tuning, nm, want[0], np.nonzero(m != want[1])[0][:6])


def test_a_refusals(ctx):
    fe, c = ctx["fe"], RC.a_cases()["a_scene"]
    want = RC.reference_a("a_scene")
    fe.set_kb8_camera(None)  # without a KB8 camera the entry refuses
    try:
        m = V.FMatcher(fe)
        with pytest.raises(V.VslamError) as ei:
            m.SearchByProjectionKeyFrameKB8(c["T"], c["Ow"], c["cam"][:4], c["th"], c["orb_dist"], RC.LSF, c["kf_kps"], c["flags"],
                                            c["x3dw"], c["mn"], c["mx"], c["desc"], dev_of(ctx, c["cur_kps"], V.KP_DTYPE),
                                            dev_of(ctx, c["cur_desc"], np.uint8), len(c["cur_kps"]), c["occupied"], RC.IMG)
        assert ei.value.code == V.ERR_INVALID
    finally:
        fe.set_kb8_camera(V.kb8_camera(*RC.CAM1))
    big = 4097  # more KeyFrame entries than the ordering key indexes
    with pytest.raises(V.VslamError) as ei:
        run_a(ctx, dict(c, kf_kps=np.zeros(big, V.KP_DTYPE), flags=np.zeros(big, np.uint8), x3dw=np.zeros((big, 3), np.float32),
                        mn=np.zeros(big, np.float32), mx=np.zeros(big, np.float32), desc=np.zeros((big, 32), np.uint8)))
    assert ei.value.code == V.ERR_UNSUPPORTED
    with pytest.raises(V.VslamError) as ei:  # intrinsics that are not the camera's
        run_a(ctx, c, proj_cam=(c["cam"][0] + 1.0,) + tuple(c["cam"][1:4]))
    assert ei.value.code == V.ERR_INVALID
    nm, m = run_a(ctx, c)  # the context serves the next call
    assert nm == want[0] and np.array_equal(m, want[1])


def test_the_pinhole_entries_still_refuse_with_a_kb8_camera(ctx):
    fe, c = ctx["fe"], RC.a_cases()["a_scene"]
    m = V.FMatcher(fe)
    kp, de, n = dev_of(ctx, c["cur_kps"], V.KP_DTYPE), dev_of(ctx, c["cur_desc"], np.uint8), len(c["cur_kps"])
    with pytest.raises(V.VslamError) as ei:
        m.SearchByProjectionKeyFrame(c["T"], c["Ow"], c["cam"][:4], c["th"], c["orb_dist"], RC.LSF, c["kf_kps"], c["flags"], c["x3dw"],
                                     c["mn"], c["mx"], c["desc"], kp, de, n, c["occupied"], RC.IMG)
    assert ei.value.code == V.ERR_UNSUPPORTED
    b = RC.b_cases()["b_one"]
    j = b["jobs"][0]
    T = np.hstack([j["pose"][0], j["pose"][1].reshape(3, 1)])
    with pytest.raises(V.VslamError) as ei:
        m.SearchByProjectionSim3(T, j["pose"][2], RC.CAM1[:4], b["th"], b["ratio"], RC.LSF, b["pts"]["valid"].astype(np.uint8),
                                 b["pts"]["pos"], b["pts"]["normal"], b["pts"]["min_distance"], b["pts"]["max_distance"], b["desc"],
                                 dev_of(ctx, j["kps"], V.KP_DTYPE), dev_of(ctx, j["desc"], np.uint8), len(j["kps"]), None, RC.IMG)
    assert ei.value.code == V.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ B
def jobs_of(ctx, c, only=None):
    out = []
    for j in (c["jobs"] if only is None else [c["jobs"][only]]):
        n = len(j["kps"])
        out.append(V.sim3_kb8_job(*j["pose"], dev_of(ctx, j["kps"], V.KP_DTYPE) if n else 0,
                                  dev_of(ctx, j["desc"], np.uint8) if n else 0, n, j.get("matched"), j.get("valid")))
    return out


def run_b(ctx, c, mode="blocking", only=None):
    fe = ctx["fe"]
    jobs = jobs_of(ctx, c, only)
    a = (jobs, c["pts"], c["desc"], c["th"], c["ratio"], RC.LSF, RC.IMG, c["gf"])
    if mode == "blocking":
        return fe.search_by_projection_sim3_kb8(*a)
    if mode == "device" and len(c["pts"]):
        import torch
        p, d = _dev(np.ascontiguousarray(c["pts"], V.FUSE_POINT_DTYPE)), _dev(np.ascontiguousarray(c["desc"], np.uint8))
        torch.cuda.synchronize()
        fe.search_by_projection_sim3_kb8_async(jobs, p.data_ptr(), d.data_ptr(), c["th"], c["ratio"], RC.LSF, RC.IMG, c["gf"],
                                               n_points=len(c["pts"]))
        return fe.search_by_projection_sim3_kb8_wait()  # p, d live until here
    fe.search_by_projection_sim3_kb8_async(*a)
    return fe.search_by_projection_sim3_kb8_wait()


def assert_same_b(got, want, what, jobs=None):
    m, nm, ng = got
    for k, j in enumerate(range(len(m)) if jobs is None else jobs):
        assert nm[k] == want[1][j] and ng[k] == want[2][j], (what, j, nm[k], want[1][j], ng[k], want[2][j])
        bad = np.nonzero(m[k] != want[0][j])[0]
        assert len(bad) == 0, (what, j, bad[:6], m[k][bad[:6]], want[0][j][bad[:6]])


@pytest.mark.parametrize("name", B_SERVED)
def test_b_every_case(ctx, name):
    c = RC.b_cases()[name]
    want = RC.reference_b(name)
    for mode in ("blocking", "async", "device"):
        assert_same_b(run_b(ctx, c, mode), want, (name, mode))


def test_b_the_sequential_wave_and_a_prefix_of_one(ctx):
    fe = ctx["fe"]
    for tuning in (dict(sbp_sequential=1), dict(sbp_topm=1)):
        fe.set_tuning(**tuning)
        try:
            for name in ("b_hand", "b_scene"):
                assert_same_b(run_b(ctx, RC.b_cases()[name]), RC.reference_b(name), (name, tuning))
        finally:
            fe.set_tuning(sbp_sequential=0, sbp_topm=8)


def test_b_six_jobs_equal_six_single_jobs(ctx):
    c = RC.b_cases()["b_six"]
    m, nm, ng = run_b(ctx, c)
    for j in range(6):
        m1, nm1, ng1 = run_b(ctx, c, only=j)
        assert np.array_equal(m1[0], m[j]) and nm1[0] == nm[j] and ng1[0] == ng[j], j
    assert nm.sum() > 100


def test_b_a_refused_job_leaves_the_others_delivered(ctx):
    fe, c = ctx["fe"], RC.b_cases()["b_4097"]
    want = RC.reference_b("b_4097")
    for mode in ("blocking", "async"):
        with pytest.raises(V.VslamError) as ei:
            run_b(ctx, c, mode)
        assert ei.value.code == V.ERR_UNSUPPORTED
        m, nm, ng = fe.last_sim3_kb8_outputs
        assert nm[1] == -1 and ng[1] == 4097 and (m[1] == -1).all()
        assert_same_b(([m[0]], nm[:1], ng[:1]), want, ("b_4097", mode), jobs=[0])
    assert_same_b(run_b(ctx, RC.b_cases()["b_one"]), RC.reference_b("b_one"), "after the refused job")


def test_b_refusals_enqueue_nothing(ctx):
    fe = ctx["fe"]
    c = RC.b_cases()["b_one"]
    j = c["jobs"][0]
    g = RC.golden()

    def refused(code, jobs, pts=c["pts"], desc=c["desc"]):
        with pytest.raises(V.VslamError) as ei:
            fe.search_by_projection_sim3_kb8(jobs, pts, desc, c["th"], c["ratio"], RC.LSF, RC.IMG)
        assert ei.value.code == code
        m, nm, ng = fe.last_sim3_kb8_outputs  # the outputs of a refused call: -1 throughout
        assert all((a == -1).all() for a in m) and (nm == -1).all() and (ng == -1).all()
        with pytest.raises(V.VslamError):
            fe.search_by_projection_sim3_kb8_wait()  # nothing was enqueued

    refused(V.ERR_INVALID, jobs_of(ctx, dict(c, jobs=[j] * 17)))
    reps = 4097 // len(g["kl"]) + 1
    big = dict(j, kps=np.tile(g["kl"], reps)[:4097], desc=np.tile(g["dl"], (reps, 1))[:4097], matched=None)
    refused(V.ERR_UNSUPPORTED, jobs_of(ctx, dict(c, jobs=[big])))
    n = V.LOCAL_POINTS_MAX + 1
    refused(V.ERR_UNSUPPORTED, jobs_of(ctx, dict(c, jobs=[dict(j, valid=None)])), np.zeros(n, V.FUSE_POINT_DTYPE),
            np.zeros((n, 32), np.uint8))
    off = V.sim3_kb8_job(*j["pose"], dev_of(ctx, j["kps"], V.KP_DTYPE), dev_of(ctx, j["desc"], np.uint8) + 8, len(j["kps"]) - 1)
    refused(V.ERR_INVALID, [off])  # descriptor rows that are not 16-byte aligned
    fe.set_kb8_camera(None)
    try:
        refused(V.ERR_INVALID, jobs_of(ctx, c))  # without a KB8 camera
    finally:
        fe.set_kb8_camera(V.kb8_camera(*RC.CAM1))
    assert_same_b(run_b(ctx, c), RC.reference_b("b_one"), "after the refusals")


def test_b_async_with_a_blocking_rig_matcher_in_between_and_one_in_flight(ctx):
    """a blocking vslam_search_by_projection_mappoints_rig between _async and _wait fills the staging block of the blocking
    matchers: both results are intact; a second _async is refused"""
    fe, c = ctx["fe"], RC.b_cases()["b_scene"]
    want = RC.reference_b("b_scene")
    g = RC.golden()
    alone = _mappoints_rig(ctx, g)
    assert alone[0] > 50
    a = (jobs_of(ctx, c), c["pts"], c["desc"], c["th"], c["ratio"], RC.LSF, RC.IMG, c["gf"])
    fe.search_by_projection_sim3_kb8_async(*a)
    with pytest.raises(V.VslamError) as ei:  # one search per context
        fe.search_by_projection_sim3_kb8_async(*a)
    assert ei.value.code == V.ERR_INVALID
    between = _mappoints_rig(ctx, g)
    assert_same_b(fe.search_by_projection_sim3_kb8_wait(), want, "with a blocking matcher in between")
    assert between[0] == alone[0] and np.array_equal(between[1], alone[1])
    with pytest.raises(V.VslamError):
        fe.search_by_projection_sim3_kb8_wait()  # nothing enqueued any more
    assert_same_b(run_b(ctx, c, "async"), want, "afterwards")


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
    return fe.search_by_projection_mappoints_rig(tl, tr, desc, frame, 1.0, 0.8, RC.IMG)


def test_b_profile_getter(ctx):
    fe, c = ctx["fe"], RC.b_cases()["b_one"]
    fe.set_profiling(True)
    try:
        run_b(ctx, c)
        run_b(ctx, c, "async")
        gate, rank, resolve, n = fe.get_sim3_kb8_profile()
    finally:
        fe.set_profiling(False)
    assert n == 2 and gate > 0 and rank > 0 and resolve > 0
