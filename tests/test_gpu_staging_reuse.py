"""GPU: one context's staging blocks (vslam_staging.h) through matcher calls of different kinds and sizes.  Every entry
carves the shared block anew, so a call must not depend on what a larger, a smaller or an empty call before it left there:
each result of the sequence equals, bit for bit, the same call on a context that has made no other call, and the oracle's
where the oracle has the entry."""
import os

import numpy as np
import pytest

import frustum_cases as FC
import frustum_ref as FR
import vi_slam_amd as V
from conftest import kp_equal
from oracle import orbo
from vi_slam_amd import synth

pytestmark = pytest.mark.gpu

W, H, NF = FC.HUT_W, FC.HUT_H, FC.HUT_NF
T0 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
LEVELSUP = 2


class Ctx:
    """The hut pair extracted into one context: slot 0 the last frame (the fixture's left image), slot 1 the current one."""

    def __init__(self, S):
        self.fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, max_batch=2)
        (kL, dL, _), (kC, dC, _) = self.fe.compute_batch([S["L"], S["C"]])
        assert kp_equal(kL, S["kL"]) and np.array_equal(dL, S["dL"]) and kp_equal(kC, S["kC"]) and np.array_equal(dC, S["dC"])
        self.last, self.cur = self.fe.slot_dev_ptrs(0), self.fe.slot_dev_ptrs(1)
        self.m = V.FMatcher(self.fe, 0.8, True)

    def close(self):
        self.fe.close()


@pytest.fixture(scope="module")
def S():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    p = np.load(os.path.join(golden, "pipeline_hut_320x240.npz"))
    g = np.load(os.path.join(golden, "tracking_hut_320x240.npz"))
    hut = FC.hut_scene()
    s = dict(L=p["L"], C=g["C"], kL=p["kL"], dL=p["dL"], kC=g["kC"], dC=g["dC"], x3=g["x3"], flags=g["flags"], Tcw=g["Tcw"],
             cam=tuple(float(v) for v in g["cam"]), mps=g["mps"], occ=g["occ"], dist_desc=g["dist_desc"], dist_off=g["dist_off"],
             sf=hut["sf"], pts=hut["pts"], desc=hut["desc"], u_right=hut["u_right"], occupied=hut["occupied"])
    assert 400 < len(s["kL"]) < 500 and 400 < len(s["kC"]) < 500 and len(s["pts"]) > 700
    # the last frame's stereo points as Fuse candidates: the range MapPoint::UpdateNormalAndDepth would give them
    X, sf = s["x3"].astype(np.float32), s["sf"]
    d = np.linalg.norm(X, axis=1).astype(np.float32)
    fp = np.zeros(len(X), V.FUSE_POINT_DTYPE)
    fp["pos"], fp["normal"] = X, X / d[:, None]
    fp["max_distance"] = 1.2 * d * sf[s["kL"]["octave"]]
    fp["min_distance"] = 0.8 * d * sf[s["kL"]["octave"]] / sf[-1]
    fp["valid"] = s["flags"] & 1
    s["fuse_pts"] = fp
    s["voc"] = synth.make_vocabulary(10, 4, seed=17)
    s["bw"] = [orbo.bow_transform(s["voc"], s[k], LEVELSUP) for k in ("dL", "dC")]
    s["inv_sigma2"] = np.asarray(orbo.Extractor(NF).tables()["inv_sigma2"], np.float32)
    return s


# ---- the calls: each takes a Ctx and the scene, returns a tuple of arrays / numbers ----
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def fuse(c, S, n):
    """the last frame's stereo points fused into the last frame itself as a KeyFrame: most of them find their own keypoint"""
    return c.m.FuseSearch(S["fuse_pts"][:n], S["dL"][:n], c.last[0], c.last[1], len(S["kL"]), None, I3, Z3, Z3, S["cam"][:5], 3.0,
                          float(FC.LSF), (W, H))


def fuse_oracle(S, n):
    wi, wd = orbo.fuse_search(S["fuse_pts"][:n], S["dL"][:n], S["kL"], S["dL"], np.full(len(S["kL"]), -1, np.float32), S["sf"],
                              S["inv_sigma2"], I3, Z3, Z3, S["cam"][:5], 3.0, float(FC.LSF), W, H, False, True)
    return wi, np.minimum(wd, np.where(wi >= 0, 255, 256)).astype(np.int32)  # the device clamps an accepted distance to 255


def sbp_frame(c, S, n):
    nm, mc, _ = c.m.SearchByProjection(S["Tcw"], T0, S["cam"], 15, S["kL"][:n], S["flags"][:n], S["x3"][:n], S["dL"][:n], c.cur[0],
                                       c.cur[1], len(S["kC"]), None, False, (W, H))
    return nm, mc


def sbp_frame_oracle(S, n):
    nm, mc, _ = orbo.search_by_projection_frame(S["Tcw"], T0, S["cam"], 15, S["kL"][:n], S["flags"][:n], S["x3"][:n], S["dL"][:n],
                                                S["kC"], S["dC"], np.full(len(S["kC"]), -1, np.float32), S["sf"], W, H)
    return nm, mc


def distinctive(c, S, nsets):
    return (V.ComputeDistinctiveDescriptors(c.fe, S["dist_desc"], S["dist_off"][:nsets + 1]),)


def sbp_mappoints(c, S, n):
    return c.m.SearchByProjectionMapPoints(S["mps"][:n], S["dL"][:n], c.cur[0], c.cur[1], len(S["kC"]), None, 3.0, S["occ"], (W, H))


def sbp_mappoints_oracle(S, n):
    return orbo.search_by_projection_mappoints(S["mps"][:n], S["dL"][:n], S["kC"], S["dC"], np.full(len(S["kC"]), -1, np.float32),
                                               S["sf"], W, H, 3.0, 0.8, S["occ"])


def _fv(bw, n):
    if n:
        return bw
    return dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))


def by_bow(c, S, n):
    return c.m.SearchByBoW(S["kL"][:n], c.last[1], (S["flags"][:n] & 1), _fv(S["bw"][0], n), S["kC"], c.cur[1], S["bw"][1])


def local_points(c, S, n):
    P = V.frustum_params(**FC.hut_params(False))
    return c.fe.search_local_points(P, S["pts"][:n], S["desc"][:n], c.cur[0], c.cur[1], len(S["kC"]), S["u_right"], S["occupied"],
                                    3.0, 0.8, want_track=True)


def local_points_ref(S, n):
    P = FR.params(**FC.hut_params(False))
    return FR.search_local_points_ref(P, S["pts"][:n], S["desc"][:n], S["kC"], S["dC"], S["u_right"], S["sf"], 3.0, 0.8,
                                      S["occupied"])


def in_frustum(c, S, n):
    return c.fe.frame_in_frustum(V.frustum_params(**FC.hut_params(False)), S["pts"][:n])


def compute_bow(c, S, nslots):
    vv = V.Vocabulary(S["voc"])
    try:
        if nslots == 0:  # a few features of the current frame through the single-set entry
            return tuple(vv.transform(c.fe, c.cur[1], 7)[k] for k in ("fv_nodes", "fv_off", "fv_feat", "bow_ids", "bow_vals"))
        vv.transform_slots_async(c.fe, 0, nslots, LEVELSUP)
        bw = vv.transform_slots_wait([len(S["kL"]), len(S["kC"])][:nslots])
        return tuple(b[k] for b in bw for k in ("fv_nodes", "fv_off", "fv_feat", "bow_ids", "bow_vals"))
    finally:
        vv.close()


def compute_bow_oracle(S, nslots):
    return tuple(S["bw"][s][k] for s in range(nslots) for k in ("fv_nodes", "fv_off", "fv_feat", "bow_ids", "bow_vals"))


ALL = 1 << 20  # slices to everything
#: (name, call, size, oracle or None) in the order the shared context makes them
SEQUENCE = [
    ("fuse all", fuse, ALL, fuse_oracle),
    ("projection(frame) 3", sbp_frame, 3, sbp_frame_oracle),
    ("distinctive 2 sets", distinctive, 2, lambda S, n: (orbo.distinctive_descriptors(S["dist_desc"], S["dist_off"][:n + 1]),)),
    ("projection(map points) all", sbp_mappoints, ALL, sbp_mappoints_oracle),
    ("ComputeBoW 7 features", compute_bow, 0, None),
    ("ComputeBoW 2 slots", compute_bow, 2, compute_bow_oracle),
    ("SearchByBoW", by_bow, ALL, lambda S, n: orbo.search_by_bow(S["kL"], S["dL"], S["flags"] & 1, S["bw"][0], S["kC"], S["dC"],
                                                                S["bw"][1], 0.8, True)),
    ("local points 5", local_points, 5, local_points_ref),
    ("isInFrustum 300", in_frustum, 300, None),
    ("local points all", local_points, ALL, local_points_ref),
    ("projection(frame) all", sbp_frame, ALL, sbp_frame_oracle),
    ("fuse 0", fuse, 0, None),
    ("projection(frame) 0", sbp_frame, 0, None),
    ("distinctive 0 sets", distinctive, 0, None),
    ("projection(map points) 0", sbp_mappoints, 0, None),
    ("SearchByBoW 0", by_bow, 0, None),
    ("local points 0", local_points, 0, None),
    ("isInFrustum 0", in_frustum, 0, None),
    ("fuse all again", fuse, ALL, fuse_oracle),
    ("local points 5 again", local_points, 5, local_points_ref),
]


def bits(v):
    return np.ascontiguousarray(v).reshape(-1).view(np.uint8).tobytes() if isinstance(v, np.ndarray) else v


def same(a, b):
    return len(a) == len(b) and all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def shared(S):
    """the whole sequence on ONE context, in order"""
    c = Ctx(S)
    try:
        return [call(c, S, n) for _, call, n, _ in SEQUENCE]
    finally:
        c.close()


def test_the_sequence_grows_reuses_and_underfills(S, shared):
    """asserted on the inputs and the shared context's results alone: the calls are not trivial ones"""
    r = dict(zip([s[0] for s in SEQUENCE], shared))
    assert ((r["fuse all"][0] >= 0) & (r["fuse all"][1] <= 50)).sum() > 300 and r["projection(frame) all"][0] > 50
    assert r["projection(map points) all"][0] > 20 and r["SearchByBoW"][0] > 10
    assert r["local points all"][0] >= 30 and 0 < r["local points all"][3] < len(S["pts"])
    assert r["projection(frame) 3"][0] <= 3 and len(r["distinctive 2 sets"][0]) == 2
    for name in ("projection(frame) 0", "projection(map points) 0", "SearchByBoW 0", "local points 0"):
        assert r[name][0] == 0 and np.all(r[name][1] == -1), name
    assert len(r["fuse 0"][0]) == 0 and len(r["distinctive 0 sets"][0]) == 0 and r["isInFrustum 0"][2] == 0


@pytest.mark.parametrize("i", range(len(SEQUENCE)), ids=[s[0] for s in SEQUENCE])
def test_call_in_the_sequence_equals_the_call_on_a_fresh_context(S, shared, i):
    name, call, n, _ = SEQUENCE[i]
    c = Ctx(S)
    try:
        assert same(shared[i], call(c, S, n)), name
    finally:
        c.close()


@pytest.mark.parametrize("i", [i for i, s in enumerate(SEQUENCE) if s[3]], ids=[s[0] for s in SEQUENCE if s[3]])
def test_call_in_the_sequence_equals_the_oracle(S, shared, i):
    name, _, n, oracle = SEQUENCE[i]
    want = oracle(S, n)
    got = shared[i]
    if oracle is local_points_ref:  # (nmatches, matches, nToMatch, kept, records): the records field by field
        assert same(got[:4], want[:4]), name
        assert all(bits(got[4][f]) == bits(want[4][f]) for f in want[4].dtype.names), name
    else:
        assert same(got, tuple(want)[:len(got)]), name
