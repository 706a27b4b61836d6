"""GPU (-m gpu): the fisheye camera (KannalaBrandt8) on the device -- vslam_kb8_project / _unproject,
vslam_kb8_unproject_slot_async, vslam_frame_in_frustum and vslam_search_local_points with a KB8 camera set,
vslam_frame_in_frustum_rig -- bit for bit (floats as uint32) against tests/kb8_ref.py, and the switch back to pinhole."""
import ctypes as C

import numpy as np
import pytest

import frustum_cases as FC
import frustum_ref as FR
import kb8_cases as KC
import kb8_ref as KR
import vi_slam_amd as V
from conftest import kp_equal
from oracle import orbo

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same(a, b):
    """bit for bit; two NaNs count as equal"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def same_records(got, want):
    return all(np.array_equal(got[f].view(U32), want[f].view(U32)) for f in want.dtype.names)


def vparams(P):
    return V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                            (P["img_w"], P["img_h"]), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])


@pytest.fixture(scope="module")
def ctx():
    """one context: the hut frame extracted into slot 0 (its keypoints are the golden's)"""
    s = KC.local_scene()
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
    k, d, _ = fe.compute_batch([s["C"]])[0]
    assert kp_equal(k, s["kC"]) and np.array_equal(d, s["dC"])
    kp, dp, _ = fe.slot_dev_ptrs(0)
    yield dict(fe=fe, s=s, kp=kp, dp=dp, n=len(k))
    fe.close()


@pytest.fixture(scope="module")
def cam_refs():
    """the reference over the whole case lists, once; the tests slice it"""
    xyz = KC.project_points()
    out = {}
    for name in ("tum", "zero", "strong_fine"):
        cam, px = KC.camera(name), KC.unproject_pixels(name)
        out[name] = (xyz, KR.project(cam, xyz), px, KR.unproject(cam, px)[0])
    return out


@pytest.fixture(scope="module")
def frustum_refs():
    P, cam, pts = KC.frustum_scene()
    Pr, camr, rig, ptsr = KC.rig_scene()
    assert np.array_equal(pts["pos"], ptsr["pos"])
    return dict(P=P, pts=pts, rig=rig, mono=KR.frame_in_frustum(P, cam, pts, FR.bounds_of(P), FC.NLEVELS)[:3],
                rig_out=KR.frame_in_frustum_rig(P, cam, rig, pts, FR.bounds_of(P), FC.NLEVELS))


# ------------------------------------------------------------------------------------------------ 1. project / unproject
@pytest.mark.parametrize("name,n", [("tum", 1), ("tum", 63), ("tum", 64), ("tum", 65), ("tum", 4099), ("zero", 4099),
                                    ("strong_fine", 4099)])
def test_project_unproject(ctx, cam_refs, name, n):
    fe = ctx["fe"]
    xyz, uv, px, rays = cam_refs[name]
    fe.set_kb8_camera(V.kb8_camera(*KC.CAMERAS[name]))
    try:
        guv = fe.kb8_project(xyz[:n])
        gr = fe.kb8_unproject(px[:n])
    finally:
        fe.set_kb8_camera(None)
    assert guv.shape == (n, 2) and same(guv, uv[:n]), (name, n)
    assert gr.shape == (n, 3) and same(gr, rays[:n]), (name, n)


def test_unproject_slot(ctx):
    import torch
    fe, s = ctx["fe"], ctx["s"]
    n, cap = ctx["n"], fe.cap
    want, _, _ = KR.unproject(s["cam"], np.stack([s["kC"]["x"], s["kC"]["y"]], 1))
    dev = torch.full((3 * cap,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        fe.kb8_unproject_slot_async(0, dev.data_ptr())
        torch.cuda.synchronize()  # the launch went to the context's own stream: wait for the whole device
    finally:
        fe.set_kb8_camera(None)
    got = dev.cpu().numpy()
    assert same(got[:3 * n].reshape(n, 3), want)
    assert n < cap and (got[3 * n:] == -7.0).all()  # entries beyond the slot's count are untouched
    with pytest.raises(V.VslamError) as ei:         # without a camera there is nothing to unproject with
        fe.kb8_unproject_slot_async(0, dev.data_ptr())
    assert ei.value.code == V.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. frustum records
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_frustum_kb8_and_rig(ctx, frustum_refs, n):
    fe = ctx["fe"]
    P, pts, rig = frustum_refs["P"], frustum_refs["pts"][:n], frustum_refs["rig"]
    wt, wd, _ = frustum_refs["mono"]
    wl, wr, wdl, wdr, _ = frustum_refs["rig_out"]
    fe.set_kb8_camera(V.kb8_camera(*KC.CAMERAS["tum"]))
    try:
        gt, gd, gn = fe.frame_in_frustum(vparams(P), pts)
        crig = V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), rig["Tlr"], rig["Trl"])
        tl, tr, dl, dr, nv = fe.frame_in_frustum_rig(vparams(P), crig, pts)
    finally:
        fe.set_kb8_camera(None)
    assert same_records(gt, wt[:n]) and np.array_equal(bits(gd), bits(wd[:n])) and gn == int((wt[:n]["flags"] & 1).sum())
    assert same_records(tl, wl[:n]) and same_records(tr, wr[:n])
    assert np.array_equal(bits(dl), bits(wdl[:n])) and np.array_equal(bits(dr), bits(wdr[:n]))
    assert nv == int((((wl[:n]["flags"] | wr[:n]["flags"]) & 1) != 0).sum())


# ------------------------------------------------------------------------------------------------ 3. SearchLocalPoints
@pytest.fixture(scope="module")
def local_ref():
    s = KC.local_scene()
    P = s["P"]
    track, depth, ntm, _, _ = KR.frame_in_frustum(P, s["cam"], s["pts"], FR.bounds_of(P), FC.NLEVELS)
    t = FR.far_filtered(P, track, depth)
    mvu = np.full(len(s["kC"]), -1, F32)
    nm, m = orbo.search_by_projection_mappoints(t, s["desc"], s["kC"], s["dC"], mvu, s["sf"], P["img_w"], P["img_h"], 3.0, 0.8,
                                                None)
    kept = int((t["flags"] & 1).sum())
    assert nm >= 100 and kept < ntm and 650 <= len(s["pts"]) <= 750  # matches to get wrong; the far test drops some points
    return nm, m, ntm, kept, track


@pytest.mark.parametrize("where", ["host", "device"])
def test_search_local_points_kb8(ctx, local_ref, where):
    fe, s = ctx["fe"], ctx["s"]
    P = vparams(s["P"])
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    try:
        if where == "host":
            got = fe.search_local_points(P, s["pts"], s["desc"], ctx["kp"], ctx["dp"], ctx["n"], None, None, 3.0, 0.8,
                                         want_track=True)
        else:
            import torch
            dpts = torch.from_numpy(np.ascontiguousarray(s["pts"]).view(np.uint8).copy()).cuda()
            ddesc = torch.from_numpy(np.ascontiguousarray(s["desc"])).cuda()
            torch.cuda.synchronize()
            got = fe.search_local_points(P, dpts.data_ptr(), ddesc.data_ptr(), ctx["kp"], ctx["dp"], ctx["n"], None, None, 3.0,
                                         0.8, n_mp=len(s["pts"]), want_track=True)
    finally:
        fe.set_kb8_camera(None)
    nm, m, ntm, kept, track = got
    wnm, wm, wntm, wkept, wtrack = local_ref
    assert (nm, ntm, kept) == (wnm, wntm, wkept)
    assert np.array_equal(m, wm) and same_records(track, wtrack)


# ------------------------------------------------------------------------------------------------ 4. switch, error paths
def test_switch_back_to_pinhole_leaves_nothing_behind(ctx, frustum_refs):
    fe = ctx["fe"]
    P, pts = FC.rotation_case()
    want = FR.frame_in_frustum(P, pts, FR.bounds_of(P), FC.NLEVELS)
    Pk, kpts = frustum_refs["P"], frustum_refs["pts"][:300]
    fe.set_kb8_camera(V.kb8_camera(*KC.CAMERAS["tum"]))
    try:
        gt, _, _ = fe.frame_in_frustum(vparams(Pk), kpts)
        assert same_records(gt, frustum_refs["mono"][0][:300])
        with pytest.raises(V.VslamError) as ei:  # the pinhole scene's intrinsics are not the camera's
            fe.frame_in_frustum(vparams(P), pts)
        assert ei.value.code == V.ERR_INVALID
    finally:
        fe.set_kb8_camera(None)
    gt, gd, gn = fe.frame_in_frustum(vparams(P), pts)
    assert same_records(gt, want[0]) and np.array_equal(bits(gd), bits(want[1])) and gn == want[2]


def _projecting_calls(fe):
    """every entry point that projects with intrinsics of its own, called with an empty problem: -> name -> return code"""
    L, h, i0 = V.lib(), fe._h, C.c_int(0)
    pp = V._ProjParams()
    pp.img_w = pp.img_h = 8
    fp = V._FuseParams()
    fp.img_w = fp.img_h = 8
    tp, job, ow = V._TriParams(), V._SbpJob(), (C.c_float * 3)()
    N = None
    out = {}
    out["frame"] = L.vslam_search_by_projection_frame(h, C.byref(pp), N, 0, N, N, N, N, N, 0, N, N, N, C.byref(i0))
    out["keyframe"] = L.vslam_search_by_projection_keyframe(h, C.byref(pp), ow, 0.18, 100, N, 0, N, N, N, N, N, N, N, 0, N, N,
                                                            C.byref(i0))
    out["sim3"] = L.vslam_search_by_projection_sim3(h, C.byref(pp), ow, 0.18, 1.0, 0, N, N, N, N, N, N, 0, N, N, 0, N, N,
                                                    C.byref(i0))
    out["fuse"] = L.vslam_fuse_search(h, C.byref(fp), N, N, 0, N, N, 0, N, N, N)
    out["triangulation"] = L.vslam_search_for_triangulation(h, C.byref(tp), N, N, N, N, 0, N, N, N, 0, N, N, N, N, 0, N, N, N,
                                                            0, N, C.byref(i0))
    return out, job


def test_error_paths(ctx, frustum_refs):
    fe = ctx["fe"]
    L = V.lib()
    codes, job = _projecting_calls(fe)
    assert set(codes.values()) == {V.VSLAM_OK}, codes  # pinhole: empty problems succeed
    fe.set_kb8_camera(V.kb8_camera(*KC.CAMERAS["tum"]))
    try:
        codes, job = _projecting_calls(fe)
        assert set(codes.values()) == {V.ERR_UNSUPPORTED}, codes
        assert L.vslam_search_by_projection_dev_async(fe._h, 1, C.byref(job)) == V.ERR_UNSUPPORTED
        with pytest.raises(V.VslamError) as ei:  # a distorted pinhole camera beside the fisheye
            fe.set_camera(190.0, 190.0, 255.0, 255.0, [0.1, 0.0, 0.0, 0.0])
        assert ei.value.code == V.ERR_INVALID
        fe.set_camera(190.0, 190.0, 255.0, 255.0, [0.0, 0.01, 0.0, 0.0])  # k1 == 0: no distortion as the reference reads it
        fe.set_camera(None)
        P = frustum_refs["P"].copy()
        P["cx"] = np.nextafter(F32(P["cx"]), F32(1e9))
        with pytest.raises(V.VslamError) as ei:
            fe.frame_in_frustum(vparams(P), frustum_refs["pts"][:4])
        assert ei.value.code == V.ERR_INVALID
        s = ctx["s"]
        with pytest.raises(V.VslamError) as ei:  # the local scene's intrinsics are another camera's
            fe.search_local_points(vparams(s["P"]), s["pts"], s["desc"], ctx["kp"], ctx["dp"], ctx["n"])
        assert ei.value.code == V.ERR_INVALID
    finally:
        fe.set_kb8_camera(None)
    fe.set_camera(190.0, 190.0, 255.0, 255.0, [0.1, 0.0, 0.0, 0.0])
    try:
        with pytest.raises(V.VslamError) as ei:
            fe.set_kb8_camera(V.kb8_camera(*KC.CAMERAS["tum"]))
        assert ei.value.code == V.ERR_INVALID
    finally:
        fe.set_camera(None)
    with pytest.raises(V.VslamError):
        fe.kb8_project(np.zeros((1, 3), F32))  # no KB8 camera
    with pytest.raises(V.VslamError):
        fe.set_kb8_camera(V.kb8_camera(0.0, 190.0, 255.0, 255.0, KC.K_TUM))
