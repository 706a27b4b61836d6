"""SearchByProjection(CurrentFrame, LastFrame) for a two-fisheye rig (fmatcher.cpp:2494-2684, Nleft != -1): the CPU half.

1. pin: the numpy restatement (tests/frame_projection_rig_ref.py), with Pinhole::project substituted, no right keypoints and no
   mvuRight, equals projection_bounds_ref.search_by_projection_frame -- itself pinned to oracle/orbo.py -- on every frame run of
   tests/projection_bounds_cases.py;
2. twin: the host twin (vslamh_search_by_projection_frame_rig, libvslam_host.so) equals the restatement on every case;
3. census: every branch named in frame_projection_rig_ref.CENSUS is taken by some case, and every case takes the entries it is
   there for; the histogram case tells one joint histogram from two per-side ones;
4. the export table, the intrinsics test and the Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_projection_rig_cases as FP
import frame_projection_rig_ref as RR
import projection_bounds_cases as PC
import projection_bounds_ref as PB
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vslam_search_by_projection_frame_rig_async", "vslam_search_by_projection_frame_rig_wait",
               "vslam_search_by_projection_frame_rig", "vslam_fe_get_frame_rig_profile"]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def HL():
    L = C.CDLL(V.HOST_LIB_PATH)
    vp, i = C.c_void_p, C.c_int
    L.vslamh_search_by_projection_frame_rig.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, vp, vp, i, vp, vp, i, vp, vp,
                                                        C.POINTER(i)]
    L.vslamh_frame_rig_camera_check.argtypes = [vp, vp]
    return L


def params_of(c, cam=None):
    cam = cam or FP.golden()["cam"]
    return V.proj_params(c["Tcw"], (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), c["th"], FP.IMG, c["forward"], c["backward"],
                         c["ori"], c["gf"])


def host_twin(HL, c, P=None):
    g = FP.golden()
    P = P or params_of(c)
    cam = V.kb8_camera(*[g["cam"][k] for k in ("fx", "fy", "cx", "cy")], g["cam"]["k"])
    Trl = np.ascontiguousarray(c["Trl"], np.float32)
    kp = np.ascontiguousarray(c["last_kps"], V.KP_DTYPE)
    fl, xw = np.ascontiguousarray(c["flags"], np.uint8), np.ascontiguousarray(c["x3dw"], np.float32)
    md = np.ascontiguousarray(c["desc"], np.uint8)
    kl, kr = np.ascontiguousarray(c["kl"], V.KP_DTYPE), np.ascontiguousarray(c["kr"], V.KP_DTYPE)
    dl, dr = np.ascontiguousarray(c["dl"], np.uint8), np.ascontiguousarray(c["dr"], np.uint8)
    occ = None if c["occ"] is None else np.ascontiguousarray(c["occ"], np.uint8)
    sf = np.ascontiguousarray(g["sf"], np.float32)
    b = np.asarray(FP.BOUNDS, np.float32)
    m = np.full(len(kl) + len(kr) + 1, -7, np.int32)
    nm = C.c_int(-1)
    rc = HL.vslamh_search_by_projection_frame_rig(C.byref(P), C.byref(cam), _p(Trl), _p(kp), len(kp), _p(fl), _p(xw), _p(md),
                                                  _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr), _p(occ), _p(sf), len(sf),
                                                  _p(b), _p(m), C.byref(nm))
    assert m[-1] == -7
    return rc, nm.value, m[:-1]


# ------------------------------------------------------------------------------------------------ 1. pin to the oracle
FRAME_RUNS = [s for m, s in PC.RUNS if m == "frame"]


@pytest.mark.parametrize("camera", sorted(PC.SIZES))
def test_restatement_with_pinhole_equals_frame_reference(camera):
    c = PC.make_case(camera)
    fx, fy, cx, cy = c["K"]
    cam = dict(fx=fx, fy=fy, cx=cx, cy=cy)
    e_k, e_d = c["uk1"][:0], c["d1"][:0]
    flags = np.full(len(c["uk0"]), 3, np.uint8)
    for bounds in (c["bounds"], PC.int_bounds(c)):
        for s in FRAME_RUNS:
            want = PC.reference(c, "frame", s, bounds)
            T = PC.frame_pose(c, s["T"])
            fwd, bwd = PB.projection_direction(T, PC.pose(), PC.MB, s["mono"], not s["gf"])
            assert (fwd, bwd) == want[2]
            nm, m, _ = RR.search_by_projection_frame_rig(T, np.eye(3, 4), cam, s["th"], c["uk0"], flags, c["X"], c["d0"], c["uk1"],
                                                         c["d1"], e_k, e_d, c["sf"], bounds, fwd, bwd, s["ori"], None, not s["gf"],
                                                         project=RR.pinhole_project)
            assert nm == want[0] and np.array_equal(m, want[1]), (camera, s)
        assert want[0] > 100


# ------------------------------------------------------------------------------------------------ 2. the host twin
@pytest.mark.parametrize("name", sorted(FP.cases()))
def test_host_twin_equals_restatement(HL, name):
    c = FP.cases()[name]
    nm, m, _ = FP.reference(c)
    rc, hn, hm = host_twin(HL, c)
    assert rc == V.VSLAM_OK
    assert hn == nm and np.array_equal(hm, m)


def test_host_twin_intrinsics_and_arguments(HL):
    c = FP.cases()["overwrite"]
    P = params_of(c)
    P.fx = float(np.nextafter(np.float32(P.fx), np.float32(np.inf)))  # one bit
    assert host_twin(HL, c, P)[0] == V.ERR_INVALID
    P = params_of(c)
    P.mbf = 123.0  # not read
    rc, hn, hm = host_twin(HL, c, P)
    assert rc == V.VSLAM_OK and hn == FP.reference(c)[0]


# ------------------------------------------------------------------------------------------------ 3. census
def test_census_lists_no_untaken_entry():
    total = dict.fromkeys(RR.CENSUS, 0)
    for name, c in FP.cases().items():
        census = FP.reference(c)[2]
        for k in c["takes"]:
            assert census[k] > 0, (name, k)
        for k, v in census.items():
            total[k] += v
    assert [k for k, v in total.items() if not v] == []


def test_cases_obey_the_limits():
    """2 to 60 queries in the hand-made cases, a few hundred keypoints per camera, every projection finite and below 1e6"""
    g = FP.golden()
    assert 200 <= len(g["kl"]) <= 1000 and 200 <= len(g["kr"]) <= 1000
    assert g["rig"]["cam2"]["k"] != g["cam"]["k"]
    for name, c in FP.cases().items():
        if not name.startswith(("scene", "no_")):
            assert 2 <= len(c["last_kps"]) <= 60, name
        T, Trl = np.asarray(c["Tcw"], np.float64), np.asarray(c["Trl"], np.float64)
        if not len(c["x3dw"]):
            continue
        xc = c["x3dw"].astype(np.float64) @ T[:, :3].T + T[:, 3]
        xr = xc @ Trl[:, :3].T + Trl[:, 3]
        for x in (xc, xr):
            uv = RR.KR.project(g["cam"], x.astype(np.float32))
            assert np.isfinite(uv).all() and np.abs(uv).max() < 1e6, name


def test_one_histogram_over_both_sides():
    c = FP.cases()["joint_histogram"]
    nm, m, census = FP.reference(c)
    sn, sm, _ = FP.reference(c, per_side_hist=True)
    assert census["joint_histogram_rejects"] > 0
    assert sn > nm and not np.array_equal(sm, m)  # a bin that its side's three maxima keep and the joint ones reject


# ------------------------------------------------------------------------------------------------ 4. exports, mirror
def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
    host_hdr = open(os.path.join(ROOT, "vi_slam_amd", "csrc", "vslam_host.h")).read()
    assert "vslamh_search_by_projection_frame_rig" in host_hdr
    not_covered = hdr[hdr.index("Not covered:"):hdr.index("typedef struct vslam_kb8_camera")]
    assert "SearchByProjection(CurrentFrame, LastFrame)" not in not_covered
    for name in ("search_by_projection_frame_rig_async", "search_by_projection_frame_rig_wait",
                 "search_by_projection_frame_rig", "get_frame_rig_profile"):
        assert callable(getattr(V.FExtractor, name, None)), name


def test_proj_params_mirror_layout():
    P = V.proj_params(np.arange(12), (1, 2, 3, 4, 5), 7.0, (320, 240), forward=True, check_orientation=False, gemm_float=True)
    assert C.sizeof(P) == 12 * 4 + 6 * 4 + 6 * 4
    assert (P.Tcw[11], P.fx, P.cy, P.mbf, P.th) == (11.0, 1.0, 4.0, 5.0, 7.0)
    assert (P.forward, P.backward, P.check_orientation, P.img_w, P.img_h, P.gemm_float) == (1, 0, 0, 320, 240, 1)
