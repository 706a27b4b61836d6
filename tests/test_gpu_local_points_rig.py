"""GPU (-m gpu): SearchByProjection(F, vpMapPoints) and Tracking::SearchLocalPoints for a two-fisheye rig on the device --
vslam_search_by_projection_mappoints_rig, vslam_search_local_points_rig[_async/_wait] -- equal, integer for integer, to
tests/local_points_rig_ref.py (fmatcher.cpp:321-491 with Nleft != -1) over tests/local_points_rig_cases.py, by the prefix walk and
by the full re-scan walk (sbp_sequential = 1); records bit for bit against tests/kb8_ref.py and vslam_frame_in_frustum_rig."""
import ctypes as C

import numpy as np
import pytest

import frustum_cases as FC
import kb8_cases as KC
import local_points_rig_cases as LC
import local_points_rig_ref as RR
import vi_slam_amd as V
from test_gpu_kb8 import same_records, vparams

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()
    return t


@pytest.fixture(scope="module")
def ctx():
    """one context; both cameras' golden keypoints and descriptors in HBM"""
    import torch
    g = LC.golden()
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), g["sf"])
    dev = {k: _dev(g[k]) for k in ("kl", "dl", "kr", "dr")}
    torch.cuda.synchronize()
    yield dict(fe=fe, g=g, dev=dev)
    fe.close()


def frame_of(ctx, c):
    """vslam_rig_frame of a case: the golden's device arrays, or none of a side the case leaves out"""
    d = ctx["dev"]
    nl, nr = len(c["kl"]), len(c["kr"])
    return V.rig_frame(d["kl"].data_ptr() if nl else 0, d["dl"].data_ptr() if nl else 0, nl,
                       d["kr"].data_ptr() if nr else 0, d["dr"].data_ptr() if nr else 0, nr, c["l2r"], c["r2l"], c["occ"])


@pytest.fixture(scope="module")
def refs():
    """the reference over every case, once"""
    sf = LC.golden()["sf"]
    return {name: RR.search_by_projection_rig(c["tl"], c["tr"], c["desc"], c["kl"], c["dl"], c["kr"], c["dr"], c["l2r"], c["r2l"],
                                              sf, LC.BOUNDS, c["th"], c["nnratio"], c["occ"])
            for name, c in LC.cases().items()}


def fallbacks(fe):
    n = C.c_int(0)
    assert V.lib().vslam_dbg_search_init_fallbacks(fe._h, C.byref(n)) == V.VSLAM_OK
    return n.value


# ------------------------------------------------------------------------------------------------ 1. the matcher alone
@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_matcher_alone(ctx, refs, name, seq):
    fe, c = ctx["fe"], LC.cases()[name]
    fe.set_tuning(sbp_sequential=seq)
    try:
        nm, m = fe.search_by_projection_mappoints_rig(c["tl"], c["tr"], c["desc"], frame_of(ctx, c), c["th"], c["nnratio"])
    finally:
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)
    wn, wm, _ = refs[name]
    bad = np.nonzero(m != wm)[0]
    assert len(bad) == 0 and nm == wn, (name, seq, nm, wn, bad[:8], m[bad[:8]], wm[bad[:8]])


@pytest.mark.parametrize("topm", [1, 2, 8])
def test_prefix_runs_out(ctx, refs, topm):
    """occupiers take the best candidates of a window, then lookers find their whole sorted prefix taken: the window is
    re-scanned in full, and the result is still the reference's"""
    fe = ctx["fe"]
    for name in ("prefix_overflow", "scene_occupied"):
        c = LC.cases()[name]
        fe.set_tuning(sbp_topm=topm)
        try:
            fallbacks(fe)
            nm, m = fe.search_by_projection_mappoints_rig(c["tl"], c["tr"], c["desc"], frame_of(ctx, c), c["th"], c["nnratio"])
            nfb = fallbacks(fe)
        finally:
            fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        wn, wm, _ = refs[name]
        assert nm == wn and np.array_equal(m, wm), (name, topm)
        if name == "prefix_overflow":
            assert nfb >= 1, topm


# ------------------------------------------------------------------------------------------------ 2. the whole chain
@pytest.fixture(scope="module")
def chain_ref():
    """far -> th -> (nmatches, match in the caller's indices, nToMatch, kept, left records, right records)"""
    s = LC.scene()
    out = {}
    for far in (True, False):
        P, (tl, tr, dl, dr, nv), (fl, fr) = LC.scene_records(far)
        for th in (1.0, 3.0):
            nm, m, _ = RR.search_by_projection_rig(fl, fr, s["desc"], s["kl"], s["dl"], s["kr"], s["dr"], s["l2r"], s["r2l"],
                                                   s["sf"], LC.BOUNDS, th, 0.8, None)
            out[far, th] = (P, nm, m, nv, len(RR.kept_indices(fl, fr)), tl, tr)
    return out


def crig(s):
    return V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), s["rig"]["Tlr"], s["rig"]["Trl"])


def scene_frame(ctx, occ=None):
    s = LC.scene()
    return frame_of(ctx, dict(kl=s["kl"], kr=s["kr"], l2r=s["l2r"], r2l=s["r2l"], occ=occ))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("far,th,seq", [(True, 3.0, 0), (False, 1.0, 0), (True, 1.0, 1)])
def test_search_local_points_rig(ctx, chain_ref, where, far, th, seq):
    fe, s = ctx["fe"], LC.scene()
    P, wn, wm, wntm, wkept, wtl, wtr = chain_ref[far, th]
    frame = scene_frame(ctx)
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    fe.set_tuning(sbp_sequential=seq)
    try:
        if where == "host":
            got = fe.search_local_points_rig(vparams(P), crig(s), s["pts"], s["desc"], frame, th, 0.8, want_track=True)
        else:
            import torch
            dpts, ddesc = _dev(np.ascontiguousarray(s["pts"], V.MAP_POINT_DTYPE)), _dev(s["desc"])
            torch.cuda.synchronize()
            got = fe.search_local_points_rig(vparams(P), crig(s), dpts.data_ptr(), ddesc.data_ptr(), frame, th, 0.8,
                                             n_mp=len(s["pts"]), want_track=True)
        rl, rr, _, _, rnv = fe.frame_in_frustum_rig(vparams(P), crig(s), s["pts"])
    finally:
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        fe.set_kb8_camera(None)
    nm, m, ntm, kept, tl, tr = got
    assert (nm, ntm, kept) == (wn, wntm, wkept)
    assert np.array_equal(m, wm)
    assert same_records(tl, wtl) and same_records(tr, wtr)
    assert tl.tobytes() == rl.tobytes() and tr.tobytes() == rr.tobytes() and rnv == ntm


def test_async_with_other_work_and_one_in_flight(ctx, chain_ref):
    fe, s = ctx["fe"], LC.scene()
    P, wn, wm, wntm, wkept, _, _ = chain_ref[True, 3.0]
    frame = scene_frame(ctx)
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        fe.search_local_points_rig_async(vparams(P), crig(s), s["pts"], s["desc"], frame, 3.0, 0.8)
        with pytest.raises(V.VslamError) as ei:  # one search per context
            fe.search_local_points_rig_async(vparams(P), crig(s), s["pts"], s["desc"], frame, 3.0, 0.8)
        assert ei.value.code == V.ERR_INVALID
        with pytest.raises(V.VslamError) as ei:  # nor the single-camera one, nor the frustum stage alone: they share the block
            fe.search_local_points_async(vparams(P), s["pts"], s["desc"], ctx["dev"]["kl"].data_ptr(),
                                         ctx["dev"]["dl"].data_ptr(), len(s["kl"]))
        assert ei.value.code == V.ERR_INVALID
        with pytest.raises(V.VslamError) as ei:
            fe.frame_in_frustum_rig(vparams(P), crig(s), s["pts"])
        assert ei.value.code == V.ERR_INVALID
        uv = fe.kb8_project(s["pts"]["pos"][:64])  # unrelated work on the same stream
        m0 = np.zeros(4, np.int32)
        i0 = C.c_int(0)
        assert V.lib().vslam_search_local_points_wait(fe._h, m0.ctypes.data_as(C.c_void_p), C.byref(i0), C.byref(i0),
                                                      C.byref(i0), None) == V.ERR_INVALID  # the other form's wait
        nm, m, ntm, kept = fe.search_local_points_rig_wait()
    finally:
        fe.set_kb8_camera(None)
    assert uv.shape == (64, 2)
    assert (nm, ntm, kept) == (wn, wntm, wkept) and np.array_equal(m, wm)
    with pytest.raises(V.VslamError):
        fe.search_local_points_rig_wait()  # nothing enqueued any more


def test_occupied_through_the_chain(ctx):
    fe, s = ctx["fe"], LC.scene()
    P, _, (fl, fr) = LC.scene_records(True)
    occ = LC.cases()["scene_occupied"]["occ"]
    wn, wm, _ = RR.search_by_projection_rig(fl, fr, s["desc"], s["kl"], s["dl"], s["kr"], s["dr"], s["l2r"], s["r2l"], s["sf"],
                                            LC.BOUNDS, 3.0, 0.8, occ)
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        nm, m, _, _ = fe.search_local_points_rig(vparams(P), crig(s), s["pts"], s["desc"], scene_frame(ctx, occ), 3.0, 0.8)
    finally:
        fe.set_kb8_camera(None)
    assert nm == wn and np.array_equal(m, wm)


# ------------------------------------------------------------------------------------------------ 3. error paths
def test_error_paths(ctx):
    fe, s = ctx["fe"], LC.scene()
    P = s["P"]
    frame = scene_frame(ctx)
    args = (crig(s), s["pts"][:300], s["desc"][:300], frame, 3.0, 0.8)
    with pytest.raises(V.VslamError) as ei:  # a pinhole context
        fe.search_local_points_rig(vparams(P), *args)
    assert ei.value.code == V.ERR_INVALID
    c = LC.cases()["own_cross"]
    bad = c["l2r"].copy()
    bad[3] = len(c["kr"])
    worse = c["r2l"].copy()
    worse[0] = -2
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        Q = dict(P)
        Q["fx"] = np.nextafter(F32(P["fx"]), F32(1e9))
        with pytest.raises(V.VslamError) as ei:  # foreign intrinsics
            fe.search_local_points_rig(vparams(Q), *args)
        assert ei.value.code == V.ERR_INVALID
        for l2r, r2l in ((bad, c["r2l"]), (c["l2r"], worse)):
            f = frame_of(ctx, dict(c, l2r=l2r, r2l=r2l))
            with pytest.raises(V.VslamError) as ei:
                fe.search_local_points_rig(vparams(P), crig(s), s["pts"][:300], s["desc"][:300], f, 3.0, 0.8)
            assert ei.value.code == V.ERR_INVALID
            with pytest.raises(V.VslamError) as ei:
                fe.search_by_projection_mappoints_rig(c["tl"], c["tr"], c["desc"], f)
            assert ei.value.code == V.ERR_INVALID
        with pytest.raises(V.VslamError) as ei:
            fe.search_local_points_rig(vparams(P), crig(s), s["pts"][:300], s["desc"][:300], frame, 3.0, 0.3)
        assert ei.value.code == V.ERR_UNSUPPORTED
        # more than 4096 points handed on: refused with the counts delivered and no match
        pts, desc, i = LC.over_capacity_points(4097)
        with pytest.raises(V.VslamError) as ei:
            fe.search_local_points_rig(vparams(P), crig(s), pts, desc, frame, 3.0, 0.8)
        e = ei.value
        assert e.code == V.ERR_UNSUPPORTED and e.n_to_match == 4097 and e.n_matched_against == 4097
        assert (e.match_cur == -1).all() and len(e.match_cur) == len(s["kl"]) + len(s["kr"])
        nm, m, ntm, kept = fe.search_local_points_rig(vparams(P), crig(s), pts[:4096], desc[:4096], frame, 3.0, 0.8)
        _, _, (fl, fr) = LC.scene_records(True)
        wn, wm, _ = RR.search_by_projection_rig(np.repeat(fl[i:i + 1], 4096), np.repeat(fr[i:i + 1], 4096), desc[:4096], s["kl"],
                                                s["dl"], s["kr"], s["dr"], s["l2r"], s["r2l"], s["sf"], LC.BOUNDS, 3.0, 0.8, None)
        assert ntm == kept == 4096 and nm == wn and np.array_equal(m, wm)  # exactly full is served
    finally:
        fe.set_kb8_camera(None)
    with pytest.raises(V.VslamError) as ei:  # the matcher alone takes at most 4096 records
        z = np.zeros(4097, V.MP_TRACK_DTYPE)
        fe.search_by_projection_mappoints_rig(z, z, np.zeros((4097, 32), np.uint8), frame)
    assert ei.value.code == V.ERR_UNSUPPORTED
    # empty inputs are ordinary
    e = np.zeros(0, V.MP_TRACK_DTYPE)
    nm, m = fe.search_by_projection_mappoints_rig(e, e, np.zeros((0, 32), np.uint8), frame)
    assert nm == 0 and (m == -1).all() and len(m) == len(s["kl"]) + len(s["kr"])
    none = V.rig_frame(0, 0, 0, 0, 0, 0, np.zeros(0, np.int32), np.zeros(0, np.int32))
    nm, m = fe.search_by_projection_mappoints_rig(c["tl"], c["tr"], c["desc"], none)
    assert nm == 0 and len(m) == 0


# ------------------------------------------------------------------------------------------------ 4. nothing left behind
def test_nothing_left_behind(ctx, chain_ref):
    """the single-camera search and the frustum stage give, after a rig search, what they gave before it"""
    fe, s = ctx["fe"], LC.scene()
    P = s["P"]
    kp, dp, n = ctx["dev"]["kl"].data_ptr(), ctx["dev"]["dl"].data_ptr(), len(s["kl"])
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        def others():
            a = fe.search_local_points(vparams(P), s["pts"], s["desc"], kp, dp, n, None, None, 3.0, 0.8, want_track=True)
            b = fe.frame_in_frustum_rig(vparams(P), crig(s), s["pts"])
            return a, b
        a0, b0 = others()
        assert a0[0] >= 100
        got = fe.search_local_points_rig(vparams(P), crig(s), s["pts"], s["desc"], scene_frame(ctx), 3.0, 0.8)
        assert got[0] == chain_ref[True, 3.0][1]
        a1, b1 = others()
    finally:
        fe.set_kb8_camera(None)
    assert a0[0] == a1[0] and np.array_equal(a0[1], a1[1]) and a0[2:4] == a1[2:4] and a0[4].tobytes() == a1[4].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(b0[:4], b1[:4])) and b0[4] == b1[4]
