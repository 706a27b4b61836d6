"""Deterministic inputs of the rig SearchByBoW tests (F.Nleft != -1, fmatcher.cpp:546-748): tests/test_bow_rig_cpu.py,
tests/test_gpu_bow_rig.py, tests/test_cpp_bow_rig.py, tests/tools/dump_bow_rig_cases.py, tests/tools/time_bow_rig.py.  No GPU.

Everything comes from the committed golden (tests/golden/pipeline_hut_320x240.npz) and vi_slam_amd.synth.make_vocabulary:
  - the rig KeyFrame is kL + kR of the golden, 913 features, left first;
  - the realistic frame holds noisy copies of KeyFrame descriptors (3 to 45 bits flipped).  Most sources appear on BOTH sides,
    and each side has near-twin pairs (a copy of a copy, a few bits apart), which fail a ratio test;
  - it is matched at levelsup 0, 1, 2 and L (the root: one node holds every feature), ratio 0.7 and 0.9, orientation on / off;
  - hand-made cases of 2 to 40 features, one vocabulary node, for every census entry and every switch of tests/bow_rig_ref.py;
  - exactly 2049 frame features under the root: beyond the device's 2048 rule;
  - a batch of 5 keyframe jobs of different sizes against the realistic frame, one with n_right == 0 and one empty.

A case: dict(kf=dict(kps, desc, n_left, flags, fv), f=dict(kps, desc, n_left, fv), ratio, ori, takes, switches); `takes` names
the census entries and `switches` the switches of bow_rig_ref the case is there for.  reference(c) evaluates one (cached)."""
import os

import numpy as np

import bow_rig_ref as BR
from oracle import orbo
from vi_slam_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_hut_320x240.npz")
VOC_ARGS = (8, 3, 11)  # k, L, seed
LEVELSUP = (0, 1, 2, 3)
RATIOS = (0.7, 0.9)
KP = orbo.KP_DTYPE
_cache = {}


def vocabulary():
    if "voc" not in _cache:
        _cache["voc"] = synth.make_vocabulary(VOC_ARGS[0], VOC_ARGS[1], seed=VOC_ARGS[2])
    return _cache["voc"]


def fv_of(desc, levelsup):
    """the FeatureVector of the concatenated descriptors (Frame::ComputeBoW of a rig) by the oracle"""
    t = orbo.bow_transform(vocabulary(), desc, levelsup)
    return {k: t[k] for k in ("fv_nodes", "fv_off", "fv_feat")}


def keyframe():
    """the rig KeyFrame: kL + kR, 913 features, about 85 % with a good MapPoint"""
    if "kf" not in _cache:
        p = np.load(GOLDEN)
        kps = np.concatenate([p["kL"].astype(KP), p["kR"].astype(KP)])
        desc = np.ascontiguousarray(np.concatenate([p["dL"], p["dR"]]), np.uint8)
        flags = (np.random.default_rng(21).random(len(kps)) < 0.85).astype(np.uint8)
        _cache["kf"] = dict(kps=kps, desc=desc, n_left=len(p["kL"]), flags=flags)
    return _cache["kf"]


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _copies(rng, kf, sources, twins):
    """noisy copies of kf's features `sources`, then `twins` near-twins of earlier copies"""
    n = len(sources)
    desc = np.zeros((n + twins, 32), np.uint8)
    kps = np.zeros(n + twins, KP)
    for i, s in enumerate(sources):
        desc[i] = _flip(kf["desc"][s], rng.choice(256, int(rng.integers(3, 46)), replace=False))
        kps[i] = kf["kps"][s]
    for t in range(twins):
        o = int(rng.integers(0, n))
        desc[n + t] = _flip(desc[o], rng.choice(256, int(rng.integers(1, 4)), replace=False))
        kps[n + t] = kps[o]
    # the rig turned by about 40 degrees; one copy in eight has an unrelated orientation
    ang = kps["angle"].astype(np.float64) - 40.0 + rng.normal(0.0, 4.0, n + twins)
    odd = rng.random(n + twins) < 0.125
    ang[odd] = rng.uniform(0.0, 360.0, int(odd.sum()))
    kps["angle"] = np.mod(ang, 360.0).astype(np.float32)
    order = rng.permutation(n + twins)
    return kps[order], desc[order]


def frame(n_left=470, n_right=450, twins=30, seed=33):
    """the realistic rig frame: (kps, desc, n_left) with left rows first.  Two thirds of the right side's sources are on the
    left side too."""
    key = ("frame", n_left, n_right, twins, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        kf = keyframe()
        nk = len(kf["kps"])
        src_l = rng.choice(nk, n_left, replace=n_left > nk)
        shared = rng.choice(src_l, (2 * n_right) // 3, replace=(2 * n_right) // 3 > n_left)
        src_r = np.concatenate([shared, rng.choice(nk, n_right - len(shared), replace=n_right - len(shared) > nk)])
        kl, dl = _copies(rng, kf, src_l, twins)
        kr, dr = _copies(rng, kf, src_r, twins)
        _cache[key] = dict(kps=np.concatenate([kl, kr]), desc=np.ascontiguousarray(np.concatenate([dl, dr])), n_left=len(kl))
    return _cache[key]


def _with_fv(side, levelsup):
    out = dict(side)
    if len(side["desc"]) == 0:
        out["fv"] = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
        return out
    out["fv"] = fv_of(side["desc"], levelsup)
    return out


def realistic():
    """name -> case: the KeyFrame against the realistic frame at every levelsup, ratio and orientation setting"""
    if "realistic" not in _cache:
        out = {}
        for lu in LEVELSUP:
            kf, f = _with_fv(keyframe(), lu), _with_fv(frame(), lu)
            for ratio in RATIOS:
                for ori in (True, False):
                    out["real_lu%d_r%d_%s" % (lu, int(ratio * 10), "ori" if ori else "noori")] = dict(
                        kf=kf, f=f, ratio=ratio, ori=ori, levelsup=lu, takes=(), switches=())
        _cache["realistic"] = out
    return _cache["realistic"]


# ---- hand-made cases: every feature under vocabulary node 1, distances by construction ----
def _one_node(order):
    return dict(fv_nodes=np.array([1], np.int32), fv_off=np.array([0, len(order)], np.int32),
                fv_feat=np.asarray(order, np.int32))


def _hand(queries, left, right, takes, switches, ratio=0.7, ori=False, f_order=None, kf_flags=None):
    """queries: [(desc, angle)], KeyFrame features, the first half of them left; left / right: [(desc, angle)] of the frame"""
    def side(items):
        kps = np.zeros(len(items), KP)
        kps["angle"] = [a for _, a in items]
        kps["octave"] = 0
        return kps, np.array([d for d, _ in items], np.uint8).reshape(-1, 32)
    qk, qd = side(queries)
    fk, fd = side(left + right)
    kf = dict(kps=qk, desc=qd, n_left=len(queries) // 2, fv=_one_node(range(len(queries))),
              flags=np.ones(len(queries), np.uint8) if kf_flags is None else np.asarray(kf_flags, np.uint8))
    f = dict(kps=fk, desc=fd, n_left=len(left), fv=_one_node(range(len(fk)) if f_order is None else f_order))
    return dict(kf=kf, f=f, ratio=ratio, ori=ori, takes=tuple(takes), switches=tuple(switches))


def hand_made():
    """name -> case.  B, C, .. are unrelated descriptors (about 128 bits apart); b(..) flips the named bits of B, so the
    distance of two of them is the size of the symmetric difference of their bit sets."""
    if "hand" in _cache:
        return _cache["hand"]
    rng = np.random.default_rng(5)
    B, Cd = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))
    R = range

    def b(*ranges):
        return _flip(B, [x for r in ranges for x in r])

    out = {}
    # left 10 < 0.7 * 40 is written, right 5 <= TH_LOW is written; the second query (the KeyFrame's right half) finds nothing
    out["both_written"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 10)), 0), (b(R(100, 140)), 0)], [(b(R(10, 15)), 0)],
                                ["left_write", "right_write"], [])
    # left 10 against 12 fails the ratio test; the right branch still runs
    out["right_after_left_ratio_failure"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 10)), 0), (b(R(20, 32)), 0)], [(b(R(40, 45)), 0)],
                                                  ["right_write", "right_after_left_ratio_fail"], ["left_fail_continue"])
    # right 20 against 22: its own ratio test would refuse, `|| true` writes
    out["right_ratio_is_dead"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 10)), 0), (b(R(100, 140)), 0)],
                                       [(b(R(40, 60)), 0), (b(R(70, 92)), 0)],
                                       ["left_write", "right_write", "right_own_ratio_refused"], ["right_ratio"])
    # left best 60 > TH_LOW: the right 5 is never looked at
    out["right_cut_by_left_threshold"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 60)), 0)], [(b(R(100, 105)), 0)],
                                               ["right_cut_left_above_th"], ["right_unnested"])
    # the only left slot goes to the first query; the second has no free left candidate, its right 5 is never looked at
    out["right_cut_without_left_candidate"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 3)), 0)], [(_flip(Cd, R(0, 5)), 0)],
                                                    ["left_write", "right_cut_no_left_candidate"], ["right_unnested"])
    # both queries are nearest to l0 / r0; the second finds them occupied and takes l1 / r1
    q1 = b(R(0, 2))
    out["occupied_best_is_skipped"] = _hand(
        [(B, 0), (q1, 0)], [(b(R(2, 4)), 0), (b(R(0, 2), R(100, 130)), 0)], [(b(R(4, 6)), 0), (b(R(0, 2), R(140, 170)), 0)],
        ["left_write", "right_write", "occupied_best_left", "occupied_best_right"], ["right_occ_ignored"])
    # distance 50 exactly on both sides
    out["threshold_is_closed"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 50)), 0)], [(b(R(60, 110)), 0)],
                                       ["left_write", "right_write"], ["strict_th"], ratio=0.9)
    # two right candidates at distance 5: the first in FeatureVector order wins, which is the one with the higher index
    out["first_in_featurevector_order_wins"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 10)), 0)],
                                                     [(b(R(20, 25)), 0), (b(R(30, 35)), 0)], ["left_write", "right_write"], [],
                                                     f_order=[2, 1, 0])
    # a query without a MapPoint is no query
    out["flag_cleared"] = _hand([(B, 0), (Cd, 0)], [(b(R(0, 10)), 0)], [(b(R(20, 25)), 0)], [], [], kf_flags=[0, 1])
    # 12 queries, each written left and right.  Left bins 0 x 6, 1 x 3, 2 x 2, 3 x 1; right bins 4 x 5, 5 x 4, 6 x 2, 3 x 1: the joint
    # histogram keeps bins 0, 4, 5; a histogram per side would keep 0, 1, 2 and 4, 5, 6
    qs = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(12)]
    lb, rb = [0] * 6 + [1] * 3 + [2] * 2 + [3], [4] * 5 + [5] * 4 + [6] * 2 + [3]

    def ang(k):  # KeyFrame angle 0 - this = 30 * k after the wrap: bin k
        return (360.0 - 30.0 * k) % 360.0
    out["one_histogram_for_both_sides"] = _hand(
        [(q, 0.0) for q in qs], [(_flip(q, R(0, 4)), ang(lb[i])) for i, q in enumerate(qs)],
        [(_flip(q, R(8, 14)), ang(rb[i])) for i, q in enumerate(qs)], ["left_write", "right_write"], ["hist_per_side"], ori=True)
    _cache["hand"] = out
    return out


def overflow():
    """exactly 2049 frame features under the root against 60 KeyFrame features: one more than the device takes"""
    if "overflow" not in _cache:
        kf = keyframe()
        sub = np.concatenate([np.arange(30), kf["n_left"] + np.arange(30)])
        k = dict(kps=kf["kps"][sub], desc=np.ascontiguousarray(kf["desc"][sub]), n_left=30, flags=np.ones(60, np.uint8))
        f = frame(1025, 1024, 0, seed=34)
        # every feature under the root (node 0), in index order: a stopped word would leave the oracle's FeatureVector
        k, f = dict(k), dict(f)
        k["fv"], f["fv"] = _one_node(range(60)), _one_node(range(2049))
        k["fv"]["fv_nodes"][0] = f["fv"]["fv_nodes"][0] = 0
        _cache["overflow"] = dict(kf=k, f=f, ratio=0.7, ori=True, takes=(), switches=())
    return _cache["overflow"]


def _sub_keyframe(idx, n_left, levelsup, seed):
    kf = keyframe()
    idx = np.asarray(idx, np.int64)
    k = dict(kps=kf["kps"][idx], desc=np.ascontiguousarray(kf["desc"][idx].reshape(-1, 32)), n_left=n_left,
             flags=(np.random.default_rng(seed).random(len(idx)) < 0.85).astype(np.uint8))
    return _with_fv(k, levelsup)


def batch(levelsup=2):
    """5 keyframe jobs against the realistic frame -> (jobs, frame side with fv, ratio, ori): the whole KeyFrame; 300 left
    features alone (n_right == 0); an empty one; the two cameras swapped; 100 left + 57 right features"""
    key = ("batch", levelsup)
    if key not in _cache:
        kf = keyframe()
        nl, n = kf["n_left"], len(kf["kps"])
        jobs = [_with_fv(kf, levelsup), _sub_keyframe(np.arange(300), 300, levelsup, 1), _sub_keyframe([], 0, levelsup, 2),
                _sub_keyframe(np.concatenate([np.arange(nl, n), np.arange(nl)]), n - nl, levelsup, 3),
                _sub_keyframe(np.concatenate([np.arange(100, 200), nl + np.arange(57)]), 100, levelsup, 4)]
        _cache[key] = (jobs, _with_fv(frame(), levelsup), 0.7, True)
    return _cache[key]


def cases():
    """every single-keyframe case the device, the twin and the restatement are compared on"""
    out = dict(realistic())
    out.update(hand_made())
    return out


def reference(c, switches=(), census=None):
    key = ("ref", id(c), tuple(sorted(switches)))
    if census is not None or key not in _cache:
        r = BR.search_by_bow_rig(c["kf"]["kps"], c["kf"]["desc"], c["kf"]["flags"], c["kf"]["fv"], c["f"]["kps"], c["f"]["desc"],
                                 c["f"]["n_left"], c["f"]["fv"], c["ratio"], c["ori"], switches, census)
        if census is not None:
            return r
        _cache[key] = (r, c)  # keeps c alive: its id stays its own
    return _cache[key][0]
