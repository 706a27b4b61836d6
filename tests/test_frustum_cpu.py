"""CPU: Frame::isInFrustum.  The shared arithmetic (vi_slam_amd/csrc/vslam_frustum.h, host build in libvslam_host.so)
against the numpy restatement (tests/frustum_ref.py) bit for bit, on cases whose coverage is asserted on the restatement
alone first; the host end of vslam_search_local_points_wait; the export table and the Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frustum_cases as FC
import frustum_ref as FR
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def HL():
    L = C.CDLL(V.HOST_LIB_PATH)
    vp = C.c_void_p
    L.vslamh_in_frustum.argtypes = [C.POINTER(V._FrustumParams), vp, C.c_int, vp, C.c_int, vp, vp]
    L.vslamh_local_points_finish.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def c_params(P):
    return V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                            (P["img_w"], P["img_h"]), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])


def host_in_frustum(HL, P, pts, bounds):
    pts = np.ascontiguousarray(pts, V.MAP_POINT_DTYPE)
    track = np.zeros(len(pts), V.MP_TRACK_DTYPE)
    depth = np.zeros(len(pts), np.float32)
    b = None if bounds is None else np.asarray(bounds, np.float32)
    nv = HL.vslamh_in_frustum(C.byref(c_params(P)), _p(b) if b is not None else None, FC.NLEVELS, _p(pts), len(pts),
                              _p(track), _p(depth))
    return track, depth, nv


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_records_equal(got, want, what):
    gt, gd, gn = got
    wt, wd, wn = want[:3]
    for f in wt.dtype.names:
        bad = np.nonzero(bits(gt[f]) != bits(wt[f]))[0]
        assert len(bad) == 0, (what, f, bad[:5], gt[bad[:5]], wt[bad[:5]])
    assert np.array_equal(bits(gd), bits(wd)), what
    assert gn == wn, what


def test_branch_case_covers_every_exit_and_boundary():
    """asserted on the restatement alone: the comparison below means something only if the case goes everywhere"""
    (_, P, pts, b, lab), (_, Pg, gen, bg, _) = FC.branch_cases()
    t, d, nv, ex, det = FR.frame_in_frustum(P, pts, FR.bounds_of(P, b), FC.NLEVELS)
    assert set(ex) == set(FR.EXITS)
    for name, want in [("not_candidate", "not_candidate"), ("behind", "behind"), ("z_zero_pos_inf", "right"),
                       ("z_zero_neg_inf", "left"), ("left", "left"), ("right", "right"), ("top", "top"),
                       ("bottom", "bottom"), ("too_close", "too_close"), ("too_far", "too_far"), ("cos_below", "view_cos")]:
        assert ex[lab[name]] == want, name
    for name in ("z_zero_pos_inf", "z_zero_neg_inf"):  # PcZ == +0 passes the depth test; the projection is +-inf
        i = lab[name]
        assert det[i]["z"] == 0 and not np.signbit(det[i]["z"]) and np.isinf(det[i]["u"])
    on = lambda name: (ex[lab[name]] == "in_view", det[lab[name]], t[lab[name]])
    ok, dd, _ = on("u_eq_min")
    assert ok and dd["u"] == 0.0
    ok, dd, _ = on("u_eq_max")
    assert ok and dd["u"] == float(FC.W)
    ok, dd, _ = on("v_eq_min")
    assert ok and dd["v"] == 0.0
    ok, dd, _ = on("v_eq_max")
    assert ok and dd["v"] == float(FC.H)
    ok, dd, _ = on("dist_eq_min")
    assert ok and dd["dist"] == pts[lab["dist_eq_min"]]["min_dist"]
    ok, dd, rec = on("dist_eq_max")
    # dist <= max_dist on every accepted point, so the quotient is never negative: level 0 is reached at log(1) == 0
    assert ok and dd["dist"] == pts[lab["dist_eq_max"]]["max_dist"] and dd["log_ratio"] == 0.0 and rec["level"] == 0
    ok, dd, _ = on("cos_eq_limit")
    assert ok and dd["view_cos"] == P["viewing_cos_limit"]
    ok, dd, rec = on("level_top")
    assert ok and dd["log_ratio"] > FC.NLEVELS and rec["level"] == FC.NLEVELS - 1
    ok, dd, rec = on("log_ratio_integer")
    assert ok and dd["log_ratio"] == 1.0 and rec["level"] == 1
    i = lab["bounds_pass_then_far"]  # mTrackProjX / Y written although the point is rejected later (frame.cpp:557-558)
    assert ex[i] == "too_far" and t[i]["proj_x"] == 352.0 and t[i]["proj_y"] == 256.0 and t[i]["flags"] == 0
    # the general rotation: every exit but one taken again, more than two chunks of points
    tg, dg, nvg, exg, _ = FR.frame_in_frustum(Pg, gen, FR.bounds_of(Pg, bg), FC.NLEVELS)
    assert len(gen) > 2 * FC.CHUNK and len(set(exg)) >= len(FR.EXITS) - 1 and nvg >= 10
    assert (dg[(tg["flags"] & 1) == 1] > 0).all() and (dg[(tg["flags"] & 1) == 0] == 0).all()


@pytest.mark.parametrize("which", [0, 1])
def test_host_build_equals_restatement_on_the_branch_case(HL, which):
    name, P, pts, b, _ = FC.branch_cases()[which]
    assert_records_equal(host_in_frustum(HL, P, pts, b), FR.frame_in_frustum(P, pts, FR.bounds_of(P, b), FC.NLEVELS), name)


def test_fractional_bounds_case_uses_the_bands():
    (_, P, pts, b, lab), _ = FC.bounds_case()
    t, d, nv, ex, det = FR.frame_in_frustum(P, pts, FR.bounds_of(P, b), FC.NLEVELS)
    lo_x, hi_x, lo_y, hi_y = (np.float32(v) for v in b)
    i = lab["in_min_x_band"]
    assert ex[i] == "in_view" and lo_x <= det[i]["u"] < np.ceil(lo_x)
    i = lab["in_max_x_band"]
    assert ex[i] == "in_view" and np.floor(hi_x) < det[i]["u"] <= hi_x
    i = lab["in_min_y_band"]
    assert ex[i] == "in_view" and lo_y <= det[i]["v"] < np.ceil(lo_y)
    i = lab["in_max_y_band"]
    assert ex[i] == "in_view" and np.floor(hi_y) < det[i]["v"] <= hi_y
    assert [ex[lab[k]] for k in ("out_min_x", "out_max_x", "out_min_y", "out_max_y")] == ["left", "right", "top", "bottom"]
    # over the image size instead, the band points are outside: the bounds do decide
    t0 = FR.frame_in_frustum(P, pts, FR.bounds_of(P, None), FC.NLEVELS)[0]
    assert not np.array_equal(t0["flags"], t["flags"])


@pytest.mark.parametrize("which", [0, 1])
def test_host_build_equals_restatement_under_fractional_bounds(HL, which):
    name, P, pts, b, _ = FC.bounds_case()[which]
    want = FR.frame_in_frustum(P, pts, FR.bounds_of(P, b), FC.NLEVELS)
    assert want[2] >= 4
    assert_records_equal(host_in_frustum(HL, P, pts, b), want, name)


def test_float_and_double_accumulation_differ_and_the_host_build_is_the_float_one(HL):
    """cv::Matx products and Matx::dot accumulate in float; on this case a double accumulation gives other records, so the
    comparison can tell the two apart"""
    P, pts = FC.rotation_case()
    b = FR.bounds_of(P)
    flt = FR.frame_in_frustum(P, pts, b, FC.NLEVELS)
    dbl = FR.frame_in_frustum(P, pts, b, FC.NLEVELS, matx_double=True)
    differ = sum(1 for i in range(len(pts)) if flt[0][i].tobytes() != dbl[0][i].tobytes())
    assert differ >= 1 and flt[2] >= 50
    got = host_in_frustum(HL, P, pts, None)
    assert_records_equal(got, flt, "rotation")
    assert any(got[0][i].tobytes() != dbl[0][i].tobytes() for i in range(len(pts)))


def test_local_points_finish(HL):
    idx = np.array([3, 10, 11, 40, 900], np.int32)
    mc = np.array([-1, 4, 0, -1, 2, 2, 1], np.int32)
    out = np.zeros(len(mc), np.int32)
    assert HL.vslamh_local_points_finish(_p(mc), len(mc), _p(idx), len(idx), 4096, _p(out)) == V.VSLAM_OK
    assert out.tolist() == [-1, 900, 3, -1, 11, 11, 10]
    none = np.full(6, -1, np.int32)
    out = np.zeros(6, np.int32)
    assert HL.vslamh_local_points_finish(_p(none), 6, _p(idx), 0, 4096, _p(out)) == V.VSLAM_OK
    assert (out == -1).all()
    out = np.zeros(len(mc), np.int32)  # more kept points than the matcher takes
    assert HL.vslamh_local_points_finish(_p(mc), len(mc), _p(idx), 5, 4, _p(out)) == V.ERR_UNSUPPORTED
    assert (out == -1).all()
    assert HL.vslamh_local_points_finish(_p(mc), len(mc), _p(idx), 4, 4, _p(out)) == V.VSLAM_OK  # exactly full
    assert out.tolist() == [-1, -1, 3, -1, 11, 11, 10]  # an index beyond the kept count maps to no point
    assert HL.vslamh_local_points_finish(None, 3, _p(idx), 1, 4, _p(out)) == V.ERR_INVALID


NEW_SYMBOLS = ["vslam_frame_in_frustum", "vslam_search_local_points_async", "vslam_search_local_points_wait",
               "vslam_search_local_points", "vslam_fe_get_local_points_profile"]


def test_product_library_exports_the_new_entry_points():
    assert os.path.exists(V.LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(V.LIB_PATH)
    for name in NEW_SYMBOLS + ["vslamh_local_points_finish"]:
        assert hasattr(L, name), name
        assert name.startswith("vslamh_") or name in V.ABI_SYMBOLS
    assert hasattr(C.CDLL(V.HOST_LIB_PATH), "vslamh_in_frustum")


def test_python_mirror_matches_the_header():
    assert V.MAP_POINT_DTYPE.itemsize == 36 and V.MAP_POINT_DTYPE == FR.MAP_POINT_DTYPE
    assert V.MP_TRACK_DTYPE.itemsize == 24
    src = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    body = re.search(r"typedef struct vslam_frustum_params \{(.*?)\} vslam_frustum_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        assert ctype in ("float", "int32_t"), decl
        for item in rest.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            names.append(m.group(1))
            size += 4 * int(m.group(2) or 1)
    assert names == [f[0] for f in V._FrustumParams._fields_]
    assert size == C.sizeof(V._FrustumParams) == 104
    body = re.search(r"typedef struct vslam_map_point \{(.*?)\} vslam_map_point;", src, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == list(V.MAP_POINT_DTYPE.names)
    assert int(re.search(r"#define VSLAM_LOCAL_POINTS_MAX (\d+)", src).group(1)) == V.LOCAL_POINTS_MAX
