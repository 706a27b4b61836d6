"""GPU (-m gpu): SearchByProjection(CurrentFrame, LastFrame) for a two-fisheye rig on the device --
vslam_search_by_projection_frame_rig[_async/_wait] -- equal, integer for integer, to tests/frame_projection_rig_ref.py
(fmatcher.cpp:2494-2684 with Nleft != -1) over tests/frame_projection_rig_cases.py, by the parallel resolution and by the
sequential wave that re-scans every window (sbp_sequential = 1), and at sorted prefixes of 1, 2 and 8 entries."""
import ctypes as C
import gc

import numpy as np
import pytest

import frame_projection_rig_cases as FP
import frustum_cases as FC
import kb8_cases as KC
import vi_slam_amd as V

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def ctx():
    """one context with the left KB8 camera set; both cameras' golden keypoints and descriptors in HBM"""
    import torch
    g = FP.golden()
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), g["sf"])
    dev = {k: _dev(np.ascontiguousarray(g[k], V.KP_DTYPE if k[0] == "k" else np.uint8)) for k in ("kl", "dl", "kr", "dr")}
    torch.cuda.synchronize()
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    yield dict(fe=fe, g=g, dev=dev)
    fe.close()


def frame_of(ctx, c):
    d = ctx["dev"]
    nl, nr = len(c["kl"]), len(c["kr"])
    return V.rig_frame(d["kl"].data_ptr() if nl else 0, d["dl"].data_ptr() if nl else 0, nl,
                       d["kr"].data_ptr() if nr else 0, d["dr"].data_ptr() if nr else 0, nr, None, None, c["occ"])


def params_of(c, cam=KC.LOCAL_CAM):
    return V.proj_params(c["Tcw"], cam[:4], c["th"], FP.IMG, c["forward"], c["backward"], c["ori"], c["gf"])


def crig(c):
    g = FP.golden()
    return V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), g["rig"]["Tlr"], c["Trl"])


def run(ctx, c, blocking=True):
    fe = ctx["fe"]
    a = (params_of(c), crig(c), c["last_kps"], c["flags"], c["x3dw"], c["desc"], frame_of(ctx, c))
    if blocking:
        return fe.search_by_projection_frame_rig(*a)
    fe.search_by_projection_frame_rig_async(*a)
    return fe.search_by_projection_frame_rig_wait()


def fallbacks(fe):
    n = C.c_int(0)
    assert V.lib().vslam_dbg_search_init_fallbacks(fe._h, C.byref(n)) == V.VSLAM_OK
    return n.value


def live():
    v = [C.c_ulonglong() for _ in range(4)]
    assert V.lib().vslam_dbg_live_memory(*[C.byref(x) for x in v]) == V.VSLAM_OK
    return tuple(x.value for x in v)


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("name", sorted(FP.cases()))
def test_every_case(ctx, name, seq):
    fe, c = ctx["fe"], FP.cases()[name]
    wn, wm, _ = FP.reference(c)
    fe.set_tuning(sbp_sequential=seq)
    try:
        nm, m = run(ctx, c)
    finally:
        fe.set_tuning(sbp_sequential=0, sbp_topm=8)
    bad = np.nonzero(m != wm)[0]
    assert len(m) == len(wm) and len(bad) == 0 and nm == wn, (name, seq, nm, wn, bad[:8], m[bad[:8]], wm[bad[:8]])


@pytest.mark.parametrize("topm", [1, 2, 8])
def test_prefix_runs_out(ctx, topm):
    """more occupied candidates in a window than the sorted prefix holds: the call is handed to the sequential wave, which
    re-scans the window, and the result is still the reference's"""
    fe = ctx["fe"]
    for name in FP.PREFIX_CASES:
        c = FP.cases()[name]
        wn, wm, _ = FP.reference(c)
        fe.set_tuning(sbp_topm=topm)
        try:
            fallbacks(fe)
            nm, m = run(ctx, c)
            nfb = fallbacks(fe)
        finally:
            fe.set_tuning(sbp_sequential=0, sbp_topm=8)
        assert nm == wn and np.array_equal(m, wm), (name, topm)
        if name == "prefix_overflow":
            assert nfb >= 1, topm


def test_async_with_other_work_and_one_in_flight(ctx):
    fe, c = ctx["fe"], FP.cases()["scene"]
    wn, wm, _ = FP.reference(c)
    a = (params_of(c), crig(c), c["last_kps"], c["flags"], c["x3dw"], c["desc"], frame_of(ctx, c))
    fe.search_by_projection_frame_rig_async(*a)
    with pytest.raises(V.VslamError) as ei:  # one search per context
        fe.search_by_projection_frame_rig_async(*a)
    assert ei.value.code == V.ERR_INVALID
    uv = fe.kb8_project(c["x3dw"][:64])  # unrelated work on the same stream, which waits for it
    small = FP.cases()["overwrite"]  # a blocking matcher of the same family in between: it has a staging block of its own
    with pytest.raises(V.VslamError) as ei:
        fe.search_by_projection_frame_rig(params_of(small), crig(small), small["last_kps"], small["flags"], small["x3dw"],
                                          small["desc"], frame_of(ctx, small))
    assert ei.value.code == V.ERR_INVALID
    nm, m = fe.search_by_projection_frame_rig_wait()
    assert uv.shape == (64, 2)
    assert nm == wn and np.array_equal(m, wm)
    with pytest.raises(V.VslamError):
        fe.search_by_projection_frame_rig_wait()  # nothing enqueued any more
    nm, m = run(ctx, c, blocking=False)
    assert nm == wn and np.array_equal(m, wm)


def test_profile_getter(ctx):
    fe, c = ctx["fe"], FP.cases()["scene"]
    fe.set_profiling(True)
    try:
        run(ctx, c)
        run(ctx, c)
        rank_ms, resolve_ms, n = fe.get_frame_rig_profile()
    finally:
        fe.set_profiling(False)
    assert n == 2 and rank_ms > 0 and resolve_ms > 0


def test_error_paths(ctx):
    fe, c = ctx["fe"], FP.cases()["overwrite"]
    a = (crig(c), c["last_kps"], c["flags"], c["x3dw"], c["desc"], frame_of(ctx, c))
    one_bit = list(KC.LOCAL_CAM[:4])
    one_bit[2] = float(np.nextafter(np.float32(one_bit[2]), np.float32(1e9)))
    with pytest.raises(V.VslamError) as ei:  # intrinsics differing in one bit
        fe.search_by_projection_frame_rig(params_of(c, one_bit), *a)
    assert ei.value.code == V.ERR_INVALID
    # counts over the limits: nothing is enqueued
    d = ctx["dev"]
    big = V.rig_frame(d["kl"].data_ptr(), d["dl"].data_ptr(), 4097, d["kr"].data_ptr(), d["dr"].data_ptr(), 10, None, None)
    with pytest.raises(V.VslamError) as ei:
        fe.search_by_projection_frame_rig(params_of(c), *a[:5], big)
    assert ei.value.code == V.ERR_UNSUPPORTED
    big = V.rig_frame(d["kl"].data_ptr(), d["dl"].data_ptr(), 10, d["kr"].data_ptr(), d["dr"].data_ptr(), 4097, None, None)
    with pytest.raises(V.VslamError) as ei:
        fe.search_by_projection_frame_rig(params_of(c), *a[:5], big)
    assert ei.value.code == V.ERR_UNSUPPORTED
    n = 4097
    with pytest.raises(V.VslamError) as ei:
        fe.search_by_projection_frame_rig(params_of(c), crig(c), np.zeros(n, V.KP_DTYPE), np.zeros(n, np.uint8),
                                          np.zeros((n, 3), np.float32), np.zeros((n, 32), np.uint8), frame_of(ctx, c))
    assert ei.value.code == V.ERR_UNSUPPORTED
    with pytest.raises(V.VslamError):
        fe.search_by_projection_frame_rig_wait()  # nothing was enqueued by any of them
    # the pinhole entry keeps refusing while a KB8 camera is set
    m, nm = np.zeros(len(c["kl"]), np.int32), C.c_int(0)
    P = params_of(c)
    kp = np.ascontiguousarray(c["last_kps"], V.KP_DTYPE)
    rc = V.lib().vslam_search_by_projection_frame(fe._h, C.byref(P), kp.ctypes.data_as(C.c_void_p), len(kp),
                                                  c["flags"].ctypes.data_as(C.c_void_p), c["x3dw"].ctypes.data_as(C.c_void_p),
                                                  c["desc"].ctypes.data_as(C.c_void_p), C.c_void_p(d["kl"].data_ptr()),
                                                  C.c_void_p(d["dl"].data_ptr()), len(c["kl"]), None, None,
                                                  m.ctypes.data_as(C.c_void_p), C.byref(nm))
    assert rc == V.ERR_UNSUPPORTED
    # no KB8 camera; and a distorted pinhole camera, beside which none can be set
    fe.set_kb8_camera(None)
    try:
        with pytest.raises(V.VslamError) as ei:
            fe.search_by_projection_frame_rig(params_of(c), *a)
        assert ei.value.code == V.ERR_INVALID
        fe.set_camera(*KC.LOCAL_CAM[:4], dist=(-0.28, 0.07, 0.0002, 0.00002))
        try:
            with pytest.raises(V.VslamError) as ei:
                fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
            assert ei.value.code == V.ERR_INVALID
            with pytest.raises(V.VslamError) as ei:
                fe.search_by_projection_frame_rig(params_of(c), *a)
            assert ei.value.code == V.ERR_INVALID
        finally:
            fe.set_camera(None)
    finally:
        fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    wn, wm, _ = FP.reference(c)
    nm, m = run(ctx, c)
    assert nm == wn and np.array_equal(m, wm)


def test_nothing_left_behind():
    """a context of its own: created, searched with repeatedly (both walks, growing and shrinking inputs), destroyed -- the
    library's count of live device and pinned memory ends where it began"""
    import torch
    gc.collect()
    before = live()
    g = FP.golden()
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
    dev = {k: _dev(np.ascontiguousarray(g[k], V.KP_DTYPE if k[0] == "k" else np.uint8)) for k in ("kl", "dl", "kr", "dr")}
    torch.cuda.synchronize()
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    own = dict(fe=fe, g=g, dev=dev)
    grown = None
    for rep in range(3):
        for name in ("overwrite", "scene", "left_invz"):
            c = FP.cases()[name]
            wn, wm, _ = FP.reference(c)
            fe.set_tuning(sbp_sequential=rep % 2)
            nm, m = run(own, c, blocking=rep != 1)
            assert nm == wn and np.array_equal(m, wm)
        if grown is None:
            grown = live()
        else:
            assert live() == grown  # the staging block grows once
    fe.close()
    del own, fe
    gc.collect()
    assert live() == before
