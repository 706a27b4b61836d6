"""GPU (-m gpu): SearchByBoW(KeyFrame, Frame) for a two-fisheye rig on the device -- vslam_search_by_bow_rig[_async/_wait],
vslam_search_by_bow_keyframes_rig, Vocabulary.transform_rig -- equal, integer for integer, to tests/bow_rig_ref.py
(fmatcher.cpp:546-748 with F.Nleft != -1) over tests/bow_rig_cases.py.  The largest shape is 913 x 980 features."""
import os

import numpy as np
import pytest

import bow_rig_cases as BC
import bow_rig_ref as BR
import frustum_cases as FC
import vi_slam_amd as V
from oracle import orbo

pytestmark = pytest.mark.gpu


class Dev:
    """host arrays in HBM, uploaded once per array"""

    def __init__(self):
        self.t = {}

    def ptr(self, a, dtype):
        import torch
        a = np.ascontiguousarray(a, dtype)
        if a.size == 0:
            return 0
        key = (a.dtype.str, a.shape, a.tobytes())
        if key not in self.t:
            self.t[key] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
        return self.t[key].data_ptr()


@pytest.fixture(scope="module")
def ctx():
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=2)
    yield dict(fe=fe, dev=Dev())
    fe.close()


def job_of(ctx, k):
    d, nl = ctx["dev"], k["n_left"]
    return dict(kps=k["kps"], flags=k["flags"], fv=k["fv"], n_left=nl, n_right=len(k["kps"]) - nl,
                dev_desc_left=d.ptr(k["desc"][:nl], np.uint8), dev_desc_right=d.ptr(k["desc"][nl:], np.uint8))


def frame_of(ctx, f):
    d, nl = ctx["dev"], f["n_left"]
    return V.rig_frame(d.ptr(f["kps"][:nl], V.KP_DTYPE), d.ptr(f["desc"][:nl], np.uint8), nl, d.ptr(f["kps"][nl:], V.KP_DTYPE),
                       d.ptr(f["desc"][nl:], np.uint8), len(f["kps"]) - nl, None, None)


def run(ctx, c, blocking=True):
    m = V.FMatcher(ctx["fe"], c["ratio"], c["ori"])
    a = ([job_of(ctx, c["kf"])], frame_of(ctx, c["f"]), c["f"]["fv"])
    if blocking:
        return m.SearchByBoWRig(*a)[0]
    m.SearchByBoWRig_async(*a)
    return m.SearchByBoWRig_wait()[0]


def same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("blocking", [True, False])
@pytest.mark.parametrize("name", sorted(BC.cases()))
def test_every_case(ctx, name, blocking):
    c = BC.cases()[name]
    wn, wm = BC.reference(c)
    nm, m = run(ctx, c, blocking)
    bad = np.nonzero(m != wm)[0]
    assert len(m) == len(wm) and len(bad) == 0 and nm == wn, (name, nm, wn, bad[:8], m[bad[:8]], wm[bad[:8]])


def test_batch_of_five_equals_five_single_calls(ctx):
    jobs, f, ratio, ori = BC.batch()
    m = V.FMatcher(ctx["fe"], ratio, ori)
    fr = frame_of(ctx, f)
    got = m.SearchByBoWRig([job_of(ctx, k) for k in jobs], fr, f["fv"])
    m.SearchByBoWRig_async([job_of(ctx, k) for k in jobs], fr, f["fv"])
    got_async = m.SearchByBoWRig_wait()
    assert len(got) == len(got_async) == 5
    for j, k in enumerate(jobs):
        want = BC.reference(dict(kf=k, f=f, ratio=ratio, ori=ori))
        single = m.SearchByBoWRig([job_of(ctx, k)], fr, f["fv"])[0]
        assert same(got[j], want) and same(got_async[j], want) and same(single, want), j
    assert got[0][0] > 100 and got[1][0] > 30 and got[2][0] == 0 and (got[2][1] == -1).all()


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
def test_without_a_right_side_it_is_the_pinhole_entry(ctx, levelsup):
    """n_right == 0 on both sides against V.FMatcher.SearchByBoW of the same build"""
    kf, f = BC.keyframe(), BC.frame()
    kfv, ffv = BC.fv_of(kf["desc"], levelsup), BC.fv_of(f["desc"], levelsup)
    d = ctx["dev"]
    for ratio in BC.RATIOS:
        for ori in (True, False):
            m = V.FMatcher(ctx["fe"], ratio, ori)
            want = m.SearchByBoW(kf["kps"], d.ptr(kf["desc"], np.uint8), kf["flags"], kfv, f["kps"], d.ptr(f["desc"], np.uint8), ffv)
            job = dict(kps=kf["kps"], flags=kf["flags"], fv=kfv, n_left=len(kf["kps"]), n_right=0,
                       dev_desc_left=d.ptr(kf["desc"], np.uint8), dev_desc_right=0)
            fr = V.rig_frame(d.ptr(f["kps"], V.KP_DTYPE), d.ptr(f["desc"], np.uint8), len(f["kps"]), 0, 0, 0, None, None)
            got = m.SearchByBoWRig([job], fr, ffv)[0]
            assert same(got, want) and want[0] > 100, (ratio, ori)
            assert same(got, orbo.search_by_bow(kf["kps"], kf["desc"], kf["flags"], kfv, f["kps"], f["desc"], ffv, ratio, ori))


def test_more_than_2048_under_one_node_is_unsupported(ctx):
    c = BC.overflow()
    m = V.FMatcher(ctx["fe"], c["ratio"], c["ori"])
    a = ([job_of(ctx, c["kf"])], frame_of(ctx, c["f"]), c["f"]["fv"])
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig(*a)
    assert ei.value.code == V.ERR_UNSUPPORTED
    tab, nm = m.last_bow_rig_outputs  # what the blocking entry point left in its outputs
    assert tab.shape == (1, 2049) and (tab == -1).all() and nm[0] == 0
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig_async(*a)
    assert ei.value.code == V.ERR_UNSUPPORTED
    with pytest.raises(V.VslamError):
        m.SearchByBoWRig_wait()  # nothing was enqueued
    # one feature fewer under the node: served, and equal to the restatement
    f = dict(c["f"])
    f["fv"] = dict(f["fv"], fv_off=np.array([0, 2048], np.int32), fv_feat=f["fv"]["fv_feat"][:2048])
    c2 = dict(c, f=f)
    assert same(run(ctx, c2), BC.reference(c2))


def test_limits_and_bad_indices(ctx):
    c = BC.hand_made()["both_written"]
    m = V.FMatcher(ctx["fe"], 0.7, True)
    job, fr = job_of(ctx, c["kf"]), frame_of(ctx, c["f"])
    big = V.rig_frame(fr.dev_kps_left, fr.dev_desc_left, 4097, fr.dev_kps_right, fr.dev_desc_right, 1, None, None)
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig([job], big, c["f"]["fv"])
    assert ei.value.code == V.ERR_UNSUPPORTED
    bad = dict(c["f"]["fv"], fv_feat=np.array([0, 1, 3], np.int32))
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig([job], fr, bad)
    assert ei.value.code == V.ERR_INVALID
    bad = dict(c["kf"]["fv"], fv_feat=np.array([0, -1], np.int32))
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig([dict(job, fv=bad)], fr, c["f"]["fv"])
    assert ei.value.code == V.ERR_INVALID
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig([job] * 17, fr, c["f"]["fv"])
    assert ei.value.code == V.ERR_INVALID
    # empty inputs are ordinary
    none = V.rig_frame(0, 0, 0, 0, 0, 0, None, None)
    empty_fv = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
    nm, tab = m.SearchByBoWRig([job], none, empty_fv)[0]
    assert nm == 0 and len(tab) == 0
    nm, tab = m.SearchByBoWRig([job], fr, empty_fv)[0]
    assert nm == 0 and (tab == -1).all() and len(tab) == len(c["f"]["kps"])


def test_blocking_matcher_between_async_and_wait(ctx):
    """a blocking SearchByProjection(F, vpMapPoints) -- it fills the shared staging block at once -- while a rig BoW search is in
    flight: both results are intact; a second _async is refused"""
    g = np.load(os.path.join(FC.GOLDEN, "tracking_hut_320x240.npz"))
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    fe, d = ctx["fe"], ctx["dev"]
    sf = np.asarray(orbo.Extractor(FC.HUT_NF).tables()["scale"], np.float32)
    want_p = orbo.search_by_projection_mappoints(g["mps"], p["dL"], g["kC"], g["dC"], np.full(len(g["kC"]), -1, np.float32), sf,
                                                 FC.HUT_W, FC.HUT_H, 3.0, 0.8, g["occ"])
    c = BC.realistic()["real_lu2_r7_ori"]
    m = V.FMatcher(fe, c["ratio"], c["ori"])
    a = ([job_of(ctx, c["kf"])], frame_of(ctx, c["f"]), c["f"]["fv"])
    m.SearchByBoWRig_async(*a)
    with pytest.raises(V.VslamError) as ei:
        m.SearchByBoWRig_async(*a)
    assert ei.value.code == V.ERR_INVALID
    got_p = V.FMatcher(fe, 0.8, True).SearchByProjectionMapPoints(g["mps"], p["dL"], d.ptr(g["kC"], V.KP_DTYPE),
                                                                  d.ptr(g["dC"], np.uint8), len(g["kC"]), None, 3.0, g["occ"],
                                                                  (FC.HUT_W, FC.HUT_H))
    got = m.SearchByBoWRig_wait()[0]
    assert same(got, BC.reference(c))
    assert got_p[0] == want_p[0] > 20 and np.array_equal(got_p[1], want_p[1])
    with pytest.raises(V.VslamError):
        m.SearchByBoWRig_wait()  # nothing enqueued any more


def test_profile_getter(ctx):
    import ctypes as C
    fe, c = ctx["fe"], BC.realistic()["real_lu2_r7_ori"]
    fe.set_profiling(True)
    try:
        run(ctx, c)
        run(ctx, c, blocking=False)
        a, b, n = C.c_double(0), C.c_double(0), C.c_long(0)
        assert V.lib().vslam_fe_get_bow_rig_profile(fe._h, C.byref(a), C.byref(b), C.byref(n)) == V.VSLAM_OK
    finally:
        fe.set_profiling(False)
    assert n.value == 2 and a.value > 0 and b.value > 0


@pytest.mark.parametrize("levelsup", (0, 2))
def test_keyframe_keyframe_rig_equals_restatement(ctx, levelsup):
    kf = BC.keyframe()
    nl = kf["n_left"]
    sub = np.concatenate([np.arange(100, 400), nl + np.arange(50, 300)])
    k2 = dict(kps=kf["kps"][sub], desc=np.ascontiguousarray(kf["desc"][sub]), n_left=300)
    k2["desc"][::3, 5] ^= 0x5A
    f1 = kf["flags"]
    f2 = (np.random.default_rng(8).random(len(sub)) < 0.9).astype(np.uint8)
    fv1, fv2 = BC.fv_of(kf["desc"], levelsup), BC.fv_of(k2["desc"], levelsup)
    d = ctx["dev"]
    for ratio, ori in ((0.8, True), (0.6, False)):
        want = BR.search_by_bow_keyframes_rig(kf["kps"], kf["desc"], f1, nl, fv1, k2["kps"], k2["desc"], f2, 300, fv2, ratio, ori)
        got = V.FMatcher(ctx["fe"], ratio, ori).SearchByBoWKeyFramesRig(
            kf["kps"], d.ptr(kf["desc"][:nl], np.uint8), f1, nl, fv1, k2["kps"], d.ptr(k2["desc"][:300], np.uint8), f2, 300, fv2)
        assert same(got, want) and want[0] > 30
        assert len(got[1]) == len(kf["kps"]) and (got[1][nl:] == -1).all()


@pytest.mark.parametrize("levelsup", (0, 2))
def test_transform_rig_over_two_slots_equals_the_oracle(ctx, levelsup):
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    fe = ctx["fe"]
    (kl, dl, _), (kr, dr, _) = fe.compute_batch([p["L"], p["R"]])
    assert np.array_equal(dl, p["dL"]) and np.array_equal(dr, p["dR"])
    voc = BC.vocabulary()
    dv = V.Vocabulary(voc)
    try:
        got = dv.transform_rig(fe, 0, fe, 1, levelsup)
    finally:
        dv.close()
    want = orbo.bow_transform(voc, np.concatenate([dl, dr]), levelsup)
    for k in ("word", "weight", "nid", "bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat"):
        assert np.array_equal(got[k], want[k]), k
    assert got["n_left"] == len(kl) and got["n_right"] == len(kr) and (got["fv_feat"] >= len(kl)).any()
