"""GPU (-m gpu): what the five enqueue / wait operations promise around their kernels -- SearchLocalPoints, SearchLocalPoints of
a rig, SearchByProjection(CurrentFrame, LastFrame) of a rig, SearchByBoW of a rig, two-view scoring --, one table-driven test: a
wait without an enqueue, an empty enqueue, one search in flight per block, the wait's result against the blocking entry's, and
the span sums of vslam_fe_set_profiling.  The results themselves are checked against their references in each operation's own
module; here the smallest case of each serves."""
import ctypes as C

import numpy as np
import pytest

import bow_rig_cases as BC
import frame_projection_rig_cases as FP
import frustum_cases as FC
import kb8_cases as KC
import local_points_rig_cases as LC
import two_view_cases as TC
import vi_slam_amd as V

pytestmark = pytest.mark.gpu
VP = C.c_void_p


def vparams(P):
    return V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]), P["log_scale_factor"],
                            (P["img_w"], P["img_h"]), P["viewing_cos_limit"], P["far_points"], P["th_far_points"])


def code_of(call, *a):
    """the return code of a wrapper call: VSLAM_OK, or the VslamError's"""
    try:
        call(*a)
    except V.VslamError as e:
        return e.code
    return V.VSLAM_OK


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


class Op:
    """one enqueue / wait operation: inputs (`full`) and an empty form of them (`empty`) as argument tuples of `enqueue` and
    `blocking`; `wait` -> the result; `raw_wait` -> the C entry's return code; `profile` -> (span sums, passes);
    `is_empty_result` says that every match slot is -1 and every count 0"""

    def __init__(self, ctx):
        self.fe, self.dev = ctx["fe"], ctx["dev"]

    def ptr(self, a, dtype):
        """device address of a host array, uploaded once"""
        import torch
        a = np.ascontiguousarray(a, dtype)
        if a.size == 0:
            return 0
        key = (a.dtype.str, a.shape, a.tobytes())
        if key not in self.dev:
            self.dev[key] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
        return self.dev[key].data_ptr()

    def raw_lp_wait(self, rig):
        m, i = np.zeros(4096, np.int32), C.c_int(0)
        tail = (None, None) if rig else (None,)
        fn = V.lib().vslam_search_local_points_rig_wait if rig else V.lib().vslam_search_local_points_wait
        return fn(self.fe._h, m.ctypes.data_as(VP), C.byref(i), C.byref(i), C.byref(i), *tail)

    others = ()  # (enqueue, raw wait) of the form that shares the block, and the blocking entries the block refuses


class LocalPoints(Op):
    """vslam_search_local_points*: the rig scene's left camera and its first 300 MapPoints"""

    def __init__(self, ctx):
        super().__init__(ctx)
        s = LC.scene()
        self.P, self.rig = vparams(s["P"]), V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), s["rig"]["Tlr"], s["rig"]["Trl"])
        self.pts, self.desc = s["pts"][:300], s["desc"][:300]
        cur = (self.ptr(s["kl"], V.KP_DTYPE), self.ptr(s["dl"], np.uint8), len(s["kl"]))
        self.n = len(s["kl"])
        self.full = (self.P, self.pts, self.desc) + cur
        self.empty = (self.P, self.pts[:0], self.desc[:0]) + cur
        self.frame = V.rig_frame(cur[0], cur[1], cur[2], self.ptr(s["kr"], V.KP_DTYPE), self.ptr(s["dr"], np.uint8), len(s["kr"]),
                                 s["l2r"], s["r2l"], None)
        self.rig_full = (self.P, self.rig, self.pts, self.desc, self.frame)

    def enqueue(self, a):
        self.fe.search_local_points_async(*a, None, None, 3.0, 0.8)

    def wait(self):
        return self.fe.search_local_points_wait()

    def blocking(self, a):
        return self.fe.search_local_points(*a, None, None, 3.0, 0.8)

    def raw_wait(self):
        return self.raw_lp_wait(False)

    def is_empty_result(self, r):
        nm, m, ntm, kept = r
        return (nm, ntm, kept) == (0, 0, 0) and len(m) == self.n and (m == -1).all()

    def profile(self):
        a, b, n = self.fe.get_local_points_profile()
        return (a, b), n

    @property
    def others(self):
        fe = self.fe
        return dict(enqueue=lambda: fe.search_local_points_rig_async(*self.rig_full, 3.0, 0.8),
                    raw_wait=lambda: self.raw_lp_wait(True),
                    blocked=[lambda: fe.frame_in_frustum(self.P, self.pts),
                             lambda: fe.frame_in_frustum_rig(self.P, self.rig, self.pts)])


class LocalPointsRig(LocalPoints):
    """vslam_search_local_points_rig*: the same MapPoints against both cameras"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.single_full = self.full
        self.n = self.frame.n_left + self.frame.n_right
        self.full = self.rig_full
        self.empty = (self.P, self.rig, self.pts[:0], self.desc[:0], self.frame)

    def enqueue(self, a):
        self.fe.search_local_points_rig_async(*a, 3.0, 0.8)

    def wait(self):
        return self.fe.search_local_points_rig_wait()

    def blocking(self, a):
        return self.fe.search_local_points_rig(*a, 3.0, 0.8)

    def raw_wait(self):
        return self.raw_lp_wait(True)

    def profile(self):
        a, b, n = self.fe.get_local_points_rig_profile()
        return (a, b), n

    @property
    def others(self):
        o = LocalPoints.others.fget(self)
        o["enqueue"] = lambda: self.fe.search_local_points_async(*self.single_full, None, None, 3.0, 0.8)
        o["raw_wait"] = lambda: self.raw_lp_wait(False)
        return o


class FrameRig(Op):
    """vslam_search_by_projection_frame_rig*: the case with the fewest last-frame entries"""

    def __init__(self, ctx):
        super().__init__(ctx)
        c = min((c for c in FP.cases().values() if len(c["last_kps"]) and len(c["kl"]) + len(c["kr"])),
                key=lambda c: len(c["last_kps"]))
        g = FP.golden()
        nl, nr = len(c["kl"]), len(c["kr"])
        self.n = nl + nr
        frame = V.rig_frame(self.ptr(c["kl"], V.KP_DTYPE), self.ptr(c["dl"], np.uint8), nl, self.ptr(c["kr"], V.KP_DTYPE),
                            self.ptr(c["dr"], np.uint8), nr, None, None, c["occ"])
        head = (V.proj_params(c["Tcw"], KC.LOCAL_CAM[:4], c["th"], FP.IMG, c["forward"], c["backward"], c["ori"], c["gf"]),
                V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), g["rig"]["Tlr"], c["Trl"]))
        self.full = head + (c["last_kps"], c["flags"], c["x3dw"], c["desc"], frame)
        self.empty = head + (c["last_kps"][:0], c["flags"][:0], c["x3dw"][:0], c["desc"][:0], frame)

    def enqueue(self, a):
        self.fe.search_by_projection_frame_rig_async(*a)

    def wait(self):
        return self.fe.search_by_projection_frame_rig_wait()

    def blocking(self, a):
        return self.fe.search_by_projection_frame_rig(*a)

    def raw_wait(self):
        m, nm = np.zeros(8192, np.int32), C.c_int(0)
        return V.lib().vslam_search_by_projection_frame_rig_wait(self.fe._h, m.ctypes.data_as(VP), C.byref(nm))

    def is_empty_result(self, r):
        nm, m = r
        return nm == 0 and len(m) == self.n and (m == -1).all()

    def profile(self):
        a, b, n = self.fe.get_frame_rig_profile()
        return (a, b), n


class BowRig(Op):
    """vslam_search_by_bow_rig*: one keyframe job of the realistic pair"""

    def __init__(self, ctx):
        super().__init__(ctx)
        c = BC.realistic()["real_lu2_r7_ori"]
        k, f = c["kf"], c["f"]
        self.m = V.FMatcher(self.fe, c["ratio"], c["ori"])
        nl = k["n_left"]
        job = dict(kps=k["kps"], flags=k["flags"], fv=k["fv"], n_left=nl, n_right=len(k["kps"]) - nl,
                   dev_desc_left=self.ptr(k["desc"][:nl], np.uint8), dev_desc_right=self.ptr(k["desc"][nl:], np.uint8))
        nl = f["n_left"]
        self.n = len(f["kps"])
        frame = V.rig_frame(self.ptr(f["kps"][:nl], V.KP_DTYPE), self.ptr(f["desc"][:nl], np.uint8), nl,
                            self.ptr(f["kps"][nl:], V.KP_DTYPE), self.ptr(f["desc"][nl:], np.uint8), self.n - nl, None, None)
        no_nodes = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
        self.full = ([job], frame, f["fv"])
        self.empty = ([job], frame, no_nodes)

    def enqueue(self, a):
        self.m.SearchByBoWRig_async(*a)

    def wait(self):
        return self.m.SearchByBoWRig_wait()

    def blocking(self, a):
        return self.m.SearchByBoWRig(*a)

    def raw_wait(self):
        m, nm = np.zeros(8192, np.int32), (C.c_int * 16)()
        ptrs = (VP * 16)(*[m.ctypes.data] * 16)
        return V.lib().vslam_search_by_bow_rig_wait(self.fe._h, ptrs, nm)

    def is_empty_result(self, r):
        (nm, m), = r
        return nm == 0 and len(m) == self.n and (m == -1).all()

    def profile(self):
        a, b, n = C.c_double(0), C.c_double(0), C.c_long(0)
        assert V.lib().vslam_fe_get_bow_rig_profile(self.fe._h, C.byref(a), C.byref(b), C.byref(n)) == V.VSLAM_OK
        return (a.value, b.value), n.value


class TwoView(Op):
    """vslam_two_view_score*: the planar case; the empty form has no keypoints, so no pairs"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.full = ([TC.job_of(TC.planar_case())],)
        self.empty = ([TC.job_of(TC.make("no keypoints", 0, 3, 3, seed=40))],)

    def enqueue(self, a):
        self.fe.two_view_score_async(*a)

    def wait(self):
        return self.fe.two_view_score_wait()

    def blocking(self, a):
        return self.fe.two_view_score(*a)

    def raw_wait(self):
        return V.lib().vslam_two_view_score_wait(self.fe._h, (V._TwoViewResult * 1)())

    def is_empty_result(self, r):
        r, = r
        return r["n_pairs"] == 0 and len(r["pairs"]) == 0 and len(r["inliers_h"]) == 0 and len(r["inliers_f"]) == 0

    def profile(self):
        a, b, c, n = self.fe.get_two_view_profile()
        return (a, b, c), n


OPS = dict(local_points=LocalPoints, local_points_rig=LocalPointsRig, frame_rig=FrameRig, bow_rig=BowRig, two_view=TwoView)


@pytest.fixture(scope="module")
def ctx():
    """one context with the rig scene's left KB8 camera; every operation leaves it idle"""
    fe = V.FExtractor(FC.HUT_NF, 1.2, 8, 20, 7, FC.HUT_W, FC.HUT_H, max_batch=1)
    assert np.array_equal(fe.GetScaleFactors(), LC.golden()["sf"])
    fe.set_kb8_camera(V.kb8_camera(*KC.LOCAL_CAM))
    yield dict(fe=fe, dev={})
    fe.close()


@pytest.mark.parametrize("name", sorted(OPS))
def test_enqueue_wait_contract(ctx, name):
    op = OPS[name](ctx)
    fe = op.fe
    # 1. nothing enqueued
    assert op.raw_wait() == V.ERR_INVALID
    # 2. an empty input: enqueued, waited for, gone
    op.enqueue(op.empty)
    r = op.wait()
    assert op.is_empty_result(r), r
    assert op.raw_wait() == V.ERR_INVALID
    # 3. one in flight
    want = op.blocking(op.full)
    assert not op.is_empty_result(want)
    op.enqueue(op.full)
    assert code_of(op.enqueue, op.full) == V.ERR_INVALID
    if op.others:
        o = op.others
        assert code_of(o["enqueue"]) == V.ERR_INVALID
        assert o["raw_wait"]() == V.ERR_INVALID
        for blocked in o["blocked"]:
            assert code_of(blocked) == V.ERR_INVALID
    got = op.wait()
    assert same(got, want), (got, want)
    assert op.raw_wait() == V.ERR_INVALID
    # 4. the span sums
    fe.set_profiling(True)
    try:
        ms0, n0 = op.profile()
        op.blocking(op.full)
        op.enqueue(op.full)
        op.wait()
        ms1, n1 = op.profile()
        fe.set_profiling(True)
        ms2, n2 = op.profile()
    finally:
        fe.set_profiling(False)
    print(name, "passes", n0, n1, n2, "ms", ms0, ms1, ms2)
    assert n1 - n0 == 2 and all(b > a for a, b in zip(ms0, ms1)), (n0, n1, ms0, ms1)
    assert n2 == 0 and all(v == 0 for v in ms2), (n2, ms2)
