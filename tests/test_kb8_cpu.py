"""CPU: the fisheye camera (KannalaBrandt8).  The shared arithmetic of vi_slam_amd/csrc/vslam_kb8.h (host build in
libvslam_host.so) against the numpy restatement tests/kb8_ref.py and the platform libm, bit for bit; the conditions the cases
must meet, asserted on the restatement alone; the decisions of the entry points around a KB8 camera; the export table."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import frustum_cases as FC
import frustum_ref as FR
import kb8_cases as KC
import kb8_ref as KR
import vi_slam_amd as V

F32, U32 = np.float32, np.uint32
FN = {"atanf": 0, "tanf": 1, "sinf": 2, "cosf": 3, "atan2f": 4}
vp = C.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same(a, b):
    """bit for bit; two NaNs count as equal (glibc returns x + x or x - x for them, payloads are not part of the contract)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def HL():
    L = C.CDLL(V.HOST_LIB_PATH)
    fp, cp = C.POINTER(V._FrustumParams), C.POINTER(V._Kb8Camera)
    L.vslamh_libm_twin.argtypes = [C.c_int, vp, vp, C.c_int, vp]
    L.vslamh_libm_platform.argtypes = [C.c_int, vp, vp, C.c_int, vp]
    for name in ("atanf", "tanf", "sinf", "cosf"):
        getattr(L, "vslamh_" + name).argtypes = [C.c_float]
        getattr(L, "vslamh_" + name).restype = C.c_float
    L.vslamh_atan2f.argtypes = [C.c_float, C.c_float]
    L.vslamh_atan2f.restype = C.c_float
    L.vslamh_kb8_project.argtypes = [cp, vp, C.c_int, vp]
    L.vslamh_kb8_unproject.argtypes = [cp, vp, C.c_int, vp, vp]
    L.vslamh_in_frustum_kb8.argtypes = [fp, cp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.vslamh_in_frustum_kb8_rig.argtypes = [fp, cp, C.POINTER(V._Kb8Rig), vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.vslamh_kb8_exclusive.argtypes = [C.c_int, C.c_float]
    L.vslamh_kb8_frustum_check.argtypes = [fp, cp]
    L.vslamh_kb8_projecting_entry.argtypes = [C.c_int]
    return L


@pytest.fixture(scope="module")
def inputs():
    """edge list + fixed-seed sample per function, computed once: fn -> tuple of float32 arrays"""
    out = {}
    for fn in FN:
        e, s = KC.libm_edges(fn), KC.libm_sample(fn)
        out[fn] = tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(e, s))
        assert len(out[fn][0]) >= 2_000_000
    return out


def run_batch(HL, which, fn, args):
    out = np.zeros_like(args[0])
    f = HL.vslamh_libm_twin if which == "twin" else HL.vslamh_libm_platform
    assert f(FN[fn], _p(args[0]), _p(args[1]) if len(args) > 1 else None, len(out), _p(out)) == 0
    return out


def domain(fn, args):
    """where the restatement speaks: tanf below 3*pi/4, sinf / cosf below 120 (NaN beyond, by design)"""
    ix = bits(args[0]) & U32(0x7fffffff)
    if fn == "tanf":
        return (ix < 0x4016cbe4) | (ix > 0x7f800000)
    if fn in ("sinf", "cosf"):
        return (ix < 0x42f00000) | (ix > 0x7f800000)
    return np.ones(len(ix), bool)


# ------------------------------------------------------------------------------------------------ 1. libm
@pytest.mark.parametrize("fn", list(FN))
def test_twin_equals_reference(HL, inputs, fn):
    args = inputs[fn]
    bad = np.nonzero(~same(run_batch(HL, "twin", fn, args), getattr(KR, fn)(*args)))[0]
    assert len(bad) == 0, (fn, len(bad), [tuple(a[i] for a in args) for i in bad[:5]])


@pytest.mark.parametrize("fn", list(FN))
def test_twin_equals_platform_libm(HL, inputs, fn):
    gnu = C.CDLL(None).gnu_get_libc_version
    gnu.restype = C.c_char_p
    ver = gnu().decode()
    if ver != "2.35":
        pytest.skip("the restatements are pinned against glibc 2.35; this is glibc %s" % ver)
    args = inputs[fn]
    ok = domain(fn, args)
    bad = np.nonzero(~same(run_batch(HL, "twin", fn, args), run_batch(HL, "platform", fn, args)) & ok)[0]
    assert len(bad) == 0, (fn, len(bad), [tuple(a[i] for a in args) for i in bad[:5]])
    # the edge list once more, one foreign call per value: libm.so.6 itself against the scalar twins and the reference
    libm = C.CDLL("libm.so.6")
    f, t = getattr(libm, fn), getattr(HL, "vslamh_" + fn)
    f.argtypes, f.restype = [C.c_float] * len(args), C.c_float
    e = KC.libm_edges(fn)
    oke = domain(fn, e)
    want = np.array([f(*[float(a[i]) for a in e]) for i in range(len(e[0]))], F32)
    got = np.array([t(*[float(a[i]) for a in e]) for i in range(len(e[0]))], F32)
    assert (same(got, want) | ~oke).all() and (same(getattr(KR, fn)(*e), want) | ~oke).all()
    assert oke.sum() >= 0.6 * len(oke)


def test_sinf_cosf_take_negative_arguments(HL):
    """pinned for [-pi, pi]: odd / even, and every float next to the quadrant boundaries on both sides"""
    x = np.concatenate([np.linspace(-np.pi, np.pi, 100001).astype(F32), KC.libm_edges("sinf")[0]])
    x = np.ascontiguousarray(x[np.abs(x) <= F32(np.pi)])
    s, c = run_batch(HL, "twin", "sinf", (x,)), run_batch(HL, "twin", "cosf", (x,))
    sn, cn = run_batch(HL, "twin", "sinf", (-x,)), run_batch(HL, "twin", "cosf", (-x,))
    assert np.array_equal(bits(sn), bits(-s)) and np.array_equal(bits(cn), bits(c))
    assert np.abs(s.astype(np.float64) - np.sin(x.astype(np.float64))).max() < 1e-7


# ------------------------------------------------------------------------------------------------ 2. the camera
@pytest.fixture(scope="module")
def cam_refs():
    """project / unproject of the cases by the reference, once: name -> (xyz, uv, pixels, rays, steps, tmax)"""
    xyz = KC.project_points()
    out = {}
    for name in KC.CAMERAS:
        cam = KC.camera(name)
        px = KC.unproject_pixels(name)
        out[name] = (xyz, KR.project(cam, xyz), px) + KR.unproject(cam, px)
    return out


@pytest.mark.parametrize("name", list(KC.CAMERAS))
def test_project_unproject_twin_equals_reference(HL, cam_refs, name):
    xyz, uv, px, rays, steps, _ = cam_refs[name]
    cc = V.kb8_camera(*KC.CAMERAS[name])
    guv = np.zeros_like(uv)
    assert HL.vslamh_kb8_project(C.byref(cc), _p(xyz), len(xyz), _p(guv)) == 0
    bad = np.nonzero(~same(guv, uv).all(1))[0]
    assert len(bad) == 0, (name, xyz[bad[:5]], guv[bad[:5]], uv[bad[:5]])
    gr, gs = np.zeros_like(rays), np.zeros(len(px), np.int32)
    assert HL.vslamh_kb8_unproject(C.byref(cc), _p(px), len(px), _p(gr), _p(gs)) == 0
    bad = np.nonzero(~same(gr, rays).all(1))[0]
    assert len(bad) == 0, (name, px[bad[:5]], gr[bad[:5]], rays[bad[:5]])
    assert np.array_equal(gs, steps)
    assert HL.vslamh_kb8_project(None, _p(xyz), 1, _p(guv)) == -1
    bad_cam = V.kb8_camera(0.0, 190.0, 250.0, 250.0, KC.K_TUM)
    assert HL.vslamh_kb8_project(C.byref(bad_cam), _p(xyz), 1, _p(guv)) == -1


def test_camera_cases_meet_their_conditions(cam_refs):
    """asserted on the reference alone"""
    xyz, uv = cam_refs["tum"][:2]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for sx in (1, -1):
        for sy in (1, -1):
            assert ((np.sign(x) == sx) & (np.sign(y) == sy) & (z > 0)).sum() > 100  # the four quadrants of psi
    assert (z < 0).sum() > 100 and ((z == 0) & ~np.signbit(z)).sum() >= 10            # theta beyond and at 90 degrees
    assert (x == 1).sum() >= 10 and ((y == 0) & np.signbit(y)).sum() >= 6 and ((y == 0) & ~np.signbit(y)).sum() >= 6
    assert ((x == 0) & np.signbit(x)).sum() >= 6 and ((x == 0) & ~np.signbit(x)).sum() >= 6
    with np.errstate(all="ignore"):
        q = np.abs(y.astype(np.float64) / x.astype(np.float64))
    assert (q[np.isfinite(q)] > 2.0 ** 60).sum() >= 3 and ((q < 2.0 ** -60) & (q > 0)).sum() >= 3
    sub = np.abs(xyz) < np.finfo(F32).tiny
    assert (sub & (xyz != 0)).any()
    qb = bits(np.abs(y[x == 1]))
    for b in KC.ATAN_BOUNDS[:5]:  # |y / x| on both sides of every reduction boundary of atanf
        assert (qb == b - 1).any() and (qb == b).any() and (qb == b + 1).any()
    finite = np.isfinite(xyz).all(1)
    assert np.isfinite(uv[finite]).all()
    # the Newton loop: every exit count, the guard, and no theta anywhere near the end of the restated tanf
    counts = collections.Counter()
    for name in KC.CAMERAS:
        _, _, px, rays, steps, tmax = cam_refs[name]
        counts.update(steps.tolist())
        assert steps[0] == 0 and np.array_equal(bits(rays[0]), bits(np.array([0, 0, 1], F32)))  # theta_d <= 1e-8
        assert bits(tmax).max() < 0x4016cbe4, name  # 3*pi/4, the first float glibc_tanf does not restate
        assert np.isfinite(rays[np.isfinite(px).all(1)]).all(), name
    assert all(counts[k] >= 1 for k in range(0, 11)), sorted(counts.items())
    assert set(cam_refs["zero"][4].tolist()) == {0, 1}       # k = 0: the first fix is exactly zero
    assert set(cam_refs["tum"][4].tolist()) <= {0, 1, 2, 3}  # a mild lens at the default precision: three steps at most
    # a libm that is one ulp off (here: the correctly rounded atan2f, which glibc's is not) is seen by these points
    cr = KR.project(KC.camera("tum"), xyz, KR.atan2f_correctly_rounded)
    moved = (~same(cr, uv)).any(1) & finite
    print("uv moved by a correctly rounded atan2f: %d of %d points" % (moved.sum(), len(xyz)))
    assert moved.sum() > 0


# ------------------------------------------------------------------------------------------------ 3. frustum
def c_params(P):
    return V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                            (P["img_w"], P["img_h"]), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])


def records_equal(got, want):
    return all(np.array_equal(bits(got[f]) if got[f].dtype == F32 else got[f], bits(want[f]) if want[f].dtype == F32 else want[f])
               for f in want.dtype.names)


@pytest.fixture(scope="module")
def frustum_refs():
    P, cam, pts = KC.frustum_scene()
    mono = KR.frame_in_frustum(P, cam, pts, FR.bounds_of(P), FC.NLEVELS)
    Pr, camr, rig, ptsr = KC.rig_scene()
    return dict(P=P, pts=pts, mono=mono, rig=rig, rig_out=KR.frame_in_frustum_rig(Pr, camr, rig, ptsr, FR.bounds_of(Pr), FC.NLEVELS))


def test_frustum_cases_meet_their_conditions(frustum_refs):
    """asserted on the reference alone: the six exits of Frame::isInFrustum, both one-sided outcomes of the rig"""
    track, depth, nv, exits, _ = frustum_refs["mono"]
    n = len(track)
    c = collections.Counter(exits)
    six = dict(depth=c["behind"], u=c["left"] + c["right"], v=c["top"] + c["bottom"], dist=c["too_close"] + c["too_far"],
               view_cos=c["view_cos"], in_view=c["in_view"])
    assert all(v >= 0.01 * n for v in six.values()), six
    assert min(c["left"], c["right"], c["top"], c["bottom"], c["too_close"], c["too_far"]) >= 10, c
    assert nv == c["in_view"] >= 0.25 * n
    tl, tr, dl, dr, either = frustum_refs["rig_out"]
    l, r = (tl["flags"] & 1) != 0, (tr["flags"] & 1) != 0
    assert (l & ~r).sum() >= 0.01 * n and (~l & r).sum() >= 0.01 * n and (l & r).sum() >= 0.01 * n
    assert either == (l | r).sum() >= 0.25 * n
    assert (tl["level"][~l] == -1).all() and (tr["level"][~r] == -1).all() and (tl["level"][l] >= 0).all()
    # the left records of the rig are the mono records where in view, without proj_xr
    assert np.array_equal(bits(tl["proj_x"][l]), bits(track["proj_x"][l])) and np.array_equal(l, (track["flags"] & 1) != 0)


def test_frustum_twin_equals_reference(HL, frustum_refs):
    P, pts = frustum_refs["P"], np.ascontiguousarray(frustum_refs["pts"], V.MAP_POINT_DTYPE)
    cc = V.kb8_camera(*KC.CAMERAS["tum"])
    track, depth = np.zeros(len(pts), V.MP_TRACK_DTYPE), np.zeros(len(pts), F32)
    nv = HL.vslamh_in_frustum_kb8(C.byref(c_params(P)), C.byref(cc), None, FC.NLEVELS, _p(pts), len(pts), _p(track), _p(depth))
    wt, wd, wn = frustum_refs["mono"][:3]
    assert nv == wn and records_equal(track, wt) and np.array_equal(bits(depth), bits(wd))
    rig = frustum_refs["rig"]
    cr = V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), rig["Tlr"], rig["Trl"])
    tl, tr = np.zeros(len(pts), V.MP_TRACK_DTYPE), np.zeros(len(pts), V.MP_TRACK_DTYPE)
    dl, dr = np.zeros(len(pts), F32), np.zeros(len(pts), F32)
    nv = HL.vslamh_in_frustum_kb8_rig(C.byref(c_params(P)), C.byref(cc), C.byref(cr), None, FC.NLEVELS, _p(pts), len(pts),
                                      _p(tl), _p(tr), _p(dl), _p(dr))
    wl, wr, wdl, wdr, wn = frustum_refs["rig_out"]
    assert nv == wn and records_equal(tl, wl) and records_equal(tr, wr)
    assert np.array_equal(bits(dl), bits(wdl)) and np.array_equal(bits(dr), bits(wdr))


def test_frustum_twin_with_fractional_bounds(HL):
    s = KC.local_scene()
    b = np.array([-3.6, 322.3, -2.4, 241.7], F32)
    pts = np.ascontiguousarray(s["pts"], V.MAP_POINT_DTYPE)
    wt, wd, wn, exits, _ = KR.frame_in_frustum(s["P"], s["cam"], pts, b, FC.NLEVELS)
    assert 400 <= wn <= 600 and 650 <= len(pts) <= 750
    cc = V.kb8_camera(*KC.LOCAL_CAM)
    track, depth = np.zeros(len(pts), V.MP_TRACK_DTYPE), np.zeros(len(pts), F32)
    nv = HL.vslamh_in_frustum_kb8(C.byref(c_params(s["P"])), C.byref(cc), _p(b), FC.NLEVELS, _p(pts), len(pts), _p(track),
                                  _p(depth))
    assert nv == wn and records_equal(track, wt) and np.array_equal(bits(depth), bits(wd))


# ------------------------------------------------------------------------------------------------ 4. decisions, exports
def test_error_paths(HL):
    P, cam, pts = KC.frustum_scene(8)
    cp = c_params(P)
    cc = V.kb8_camera(*KC.CAMERAS["tum"])
    assert HL.vslamh_kb8_frustum_check(C.byref(cp), C.byref(cc)) == V.VSLAM_OK
    assert HL.vslamh_kb8_frustum_check(C.byref(cp), None) == V.VSLAM_OK  # pinhole: nothing to compare
    assert HL.vslamh_kb8_frustum_check(None, C.byref(cc)) == V.ERR_INVALID
    for field in ("fx", "fy", "cx", "cy"):  # one ulp off in any of the four
        q = c_params(P)
        setattr(q, field, float(np.nextafter(F32(getattr(q, field)), F32(1e9))))
        assert HL.vslamh_kb8_frustum_check(C.byref(q), C.byref(cc)) == V.ERR_INVALID, field
        t, d = np.zeros(8, V.MP_TRACK_DTYPE), np.zeros(8, F32)
        mp = np.ascontiguousarray(pts, V.MAP_POINT_DTYPE)
        assert HL.vslamh_in_frustum_kb8(C.byref(q), C.byref(cc), None, 8, _p(mp), 8, _p(t), _p(d)) == -1
    # KB8 and a distorted pinhole camera exclude each other, whichever comes second; k1 == 0 is no distortion
    # (the GPU suite sets both cameras in both orders on a real context, tests/test_gpu_kb8.py)
    assert HL.vslamh_kb8_exclusive(1, 0.1) == V.ERR_INVALID and HL.vslamh_kb8_exclusive(1, -0.2) == V.ERR_INVALID
    assert HL.vslamh_kb8_exclusive(1, 0.0) == V.VSLAM_OK and HL.vslamh_kb8_exclusive(0, 0.3) == V.VSLAM_OK
    # the projecting entry points refuse while a KB8 camera is set
    assert HL.vslamh_kb8_projecting_entry(1) == V.ERR_UNSUPPORTED and HL.vslamh_kb8_projecting_entry(0) == V.VSLAM_OK


NEW_SYMBOLS = ["vslam_fe_set_kb8_camera", "vslam_kb8_project", "vslam_kb8_unproject", "vslam_kb8_unproject_slot_async",
               "vslam_frame_in_frustum_rig"]


def test_exports_and_mirror():
    assert os.path.exists(V.LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(V.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in V.ABI_SYMBOLS, name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vslam_fe.h")).read()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in src, name
    assert C.sizeof(V._Kb8Camera) == 36 and C.sizeof(V._Kb8Rig) == 36 + 96
    assert [f[0] for f in V._Kb8Camera._fields_] == ["fx", "fy", "cx", "cy", "k", "precision"]
