"""Cases of the covisibility tests.  A scene is a list of mutator calls ("name", args...) that `apply` replays on any
target with the mirror's method names: covis_ref.Graph, V.CovisibilityMapHost, V.CovisibilityMap.  CENSUS lists the
branches of covis_ref that the query cases below must reach (tests/test_covis_cpu.py::test_census)."""
import numpy as np

import covis_ref

CONN, VOTE = 0, 1

CENSUS = [
    "conn.th15_path", "conn.fallback_single", "conn.tie_for_nmax", "conn.equal_weights_in_ordered", "conn.count_eq_14",
    "conn.count_eq_15", "conn.observer_self", "conn.observer_bad", "conn.observer_other_map", "conn.point_listed_twice",
    "conn.bad_point", "conn.null_point", "conn.empty_counter", "vote.bad_point", "vote.bad_keyframe", "mode.0", "mode.1",
    "cull.nobs_eq_3", "cull.nobs_eq_4", "cull.qualifying_eq_3", "cull.qualifying_eq_4", "cull.level_eq_plus_1",
    "cull.level_eq_plus_2", "cull.left_only", "cull.rig_right_only", "cull.rig_both_right_smaller",
    "cull.stereo_lifts_two_keyframes", "cull.bad_point",
]


def key_of(kf_id):
    """an order_key that is neither ascending nor descending in the id, as heap addresses are"""
    return 0x7F0000000000 + ((kf_id * 7919 + 13) % 10007) * 0x1D0 + kf_id % 3


def apply(target, ops):
    for op in ops:
        getattr(target, op[0])(*op[1:])


def build(ops, target=None):
    g = target if target is not None else covis_ref.Graph()
    apply(g, ops)
    return g


def observe(ops, mp, kfs, level=0, idx=None):
    ops.append(("add_point", mp))
    for k in kfs:
        ops.append(("add_observation", mp, k, mp % 1000 if idx is None else idx, False, level, False))


def connections_scene():
    """-> (ops, jobs).  Keyframes 0-8 of map 0, 9 of map 1, 10 bad; see the comments for what each group is for."""
    ops = [("add_keyframe", k, 1 if k == 9 else 0, key_of(k)) for k in range(11)]
    mp = 0
    lists = {k: [] for k in range(11)}

    def group(n, kfs):
        nonlocal mp
        for _ in range(n):
            observe(ops, mp, kfs)
            for k in kfs:
                lists[k].append(mp)
            mp += 1
    group(20, (0, 1, 2))        # 1 and 2 tie for n_max and have equal weights in the ordered list
    group(15, (0, 3))           # a count of exactly 15
    group(14, (0, 4))           # a count of exactly 14: in the counter, not in the ordered list
    group(5, (0, 9, 10))        # observers of another map and a bad one
    group(3, (5, 6, 7))         # nothing reaches 15: the single (n_max, kf_max), with a tie for it
    ops.append(("set_keyframe_bad", 10))
    observe(ops, mp, (0, 1, 2, 3))
    ops.append(("clear_point", mp))  # a point that is bad in the mirror
    bad_mp = mp
    l0 = lists[0] + [lists[0][0], bad_mp, None]  # a point listed twice, a bad one, a NULL
    jobs = [
        dict(mode=CONN, self_kf=0, map_id=0, min_obs=0, mp_ids=l0),
        dict(mode=CONN, self_kf=5, map_id=0, min_obs=3, mp_ids=lists[5]),
        dict(mode=CONN, self_kf=8, map_id=0, min_obs=0, mp_ids=[None, None]),      # an empty counter
        dict(mode=CONN, self_kf=1, map_id=0, min_obs=4, mp_ids=lists[1]),
        dict(mode=VOTE, self_kf=-1, map_id=0, min_obs=0, mp_ids=l0),               # the frame's vote over the same list
        dict(mode=VOTE, self_kf=-1, map_id=0, min_obs=2, mp_ids=[]),
        dict(mode=CONN, self_kf=9, map_id=1, min_obs=0, mp_ids=lists[9]),          # the only keyframe of its map
        dict(mode=CONN, self_kf=0, map_id=0, min_obs=0, mp_ids=[123456]),          # an id the mirror does not know
        dict(mode=CONN, self_kf=777, map_id=0, min_obs=0, mp_ids=lists[0]),        # an unknown self_kf
    ]
    return ops, jobs


def culling_scene():
    """-> (ops, jobs): keyframe 0 is the one examined; 1-4 are monocular observers, 5-8 a rig's"""
    ops = [("add_keyframe", k, 0, key_of(k)) for k in range(10)]
    A = lambda mp, k, idx, right, level, stereo=False: ops.append(("add_observation", mp, k, idx, right, level, stereo))
    ids, levels = [], []

    def point(mp, level):
        ops.append(("add_point", mp))
        ids.append(mp)
        levels.append(level)
    point(0, 0)                                  # nObs exactly 3: counted in nMPs only
    for k in (0, 1, 2):
        A(0, k, 0, False, 0)
    point(1, 0)                                  # nObs exactly 4, three qualifying observers: not redundant
    for k in (0, 1, 2, 3):
        A(1, k, 1, False, 0)
    point(2, 0)                                  # four qualifying observers: redundant
    for k in (0, 1, 2, 3, 4):
        A(2, k, 2, False, 0)
    point(3, 1)                                  # levels level + 1 (counts) and level + 2 (does not): three qualify
    A(3, 0, 3, False, 1)
    A(3, 1, 3, False, 2)
    A(3, 2, 3, False, 3)
    A(3, 3, 3, False, 0)
    A(3, 4, 3, False, 0)
    point(4, 2)                                  # rig observers: left only, right only, both
    A(4, 0, 4, False, 2)
    A(4, 5, 4, False, 1)
    A(4, 6, 1004, True, 1)
    A(4, 7, 4, False, 5)
    A(4, 7, 1004, True, 2)                       # the right level is the smaller one and qualifies
    A(4, 8, 4, False, 1)
    A(4, 8, 1004, True, 6)
    point(5, 0)                                  # two stereo observations: nObs = 4 with two keyframes
    A(5, 0, 5, False, 0, True)
    A(5, 1, 5, False, 0, True)
    point(6, 0)                                  # bad in the mirror
    for k in (0, 1, 2, 3, 4):
        A(6, k, 6, False, 0)
    ops.append(("clear_point", 6))
    ids.insert(3, None)
    levels.insert(3, 0)
    jobs = [
        dict(kf_id=0, mp_ids=ids, levels=levels),
        dict(kf_id=1, mp_ids=[0, 1, 2, 3, 5], levels=[0, 0, 0, 2, 0]),
        dict(kf_id=9, mp_ids=[], levels=[]),
        dict(kf_id=0, mp_ids=[99999], levels=[0]),          # an unknown MapPoint
        dict(kf_id=4242, mp_ids=[0], levels=[0]),           # an unknown keyframe
    ]
    return ops, jobs


def walk_scene():
    """-> (ops, jobs, redundant_th): culling keyframe 1 takes one observer from every point, after which 2 is no longer
    redundant; 3 is examined with the graph as it is then"""
    ops = [("add_keyframe", k, 0, key_of(k)) for k in range(6)]
    for mp in range(12):
        observe(ops, mp, (1, 2, 3, 4, 5))
    jobs = [dict(kf_id=k, mp_ids=list(range(12)), levels=[0] * 12) for k in (1, 2, 3)]
    return ops, jobs, 0.9


def culling_walk(run, jobs, redundant_th, cull):
    """The walk rule: `run(jobs)` answers a list of jobs in one enqueue; its results hold up to and including the first
    job whose keyframe is culled, so the walk applies that cull (`cull(job)`: the mutators) and enqueues the rest again.
    -> (results in job order, ids of the culled keyframes)"""
    results, culled, at = [], [], 0
    while at < len(jobs):
        res = run(jobs[at:])
        for r in res:
            results.append(r)
            job = jobs[at]
            at += 1
            if not r["error"] and r["n_redundant"] > redundant_th * r["n_mps"]:  # localmapping.cpp:1054
                cull(job)
                culled.append(job["kf_id"])
                break
    return results, culled


def random_scene(n_kf, n_mp, obs_per_point, seed, n_maps=1):
    """ops: n_kf keyframes (added in bulk), n_mp points with up to obs_per_point observers each"""
    rng = np.random.RandomState(seed)
    kf = np.arange(n_kf)
    ops = [("add_keyframes", kf, kf % n_maps, np.array([key_of(int(k)) for k in kf], np.uint64))]
    for mp in range(n_mp):
        ops.append(("add_point", mp))
        n = int(rng.randint(0, obs_per_point + 1))
        for k in rng.choice(n_kf, size=min(n, n_kf), replace=False):
            ops.append(("add_observation", mp, int(k), int(rng.randint(0, 2000)), bool(rng.randint(0, 4) == 0),
                        int(rng.randint(0, 8)), bool(rng.randint(0, 3) == 0)))
    return ops


def same_connections(got, want):
    """every output array of a job, for equality"""
    for f in ("error", "kf_max", "n_max", "n_tracked"):
        assert int(got[f]) == int(want[f]), (f, got[f], want[f])
    for f in ("counter_kf", "counter_n", "ordered_kf", "ordered_w"):
        assert list(map(int, got[f])) == list(map(int, want[f])), (f, list(got[f]), list(want[f]))


def same_point(got, want):
    nobs, bad, obs = got
    assert (nobs, bool(bad)) == (want[0], want[1]), (got, want)
    rows = [tuple(int(v) for v in (o["kf_id"], o["left_idx"], o["right_idx"], o["left_level"], o["right_level"], o["stereo"]))
            for o in obs]
    assert rows == want[2], (rows, want[2])


def random_mutations(n, seed, n_kf=12, n_mp=40):
    """-> [(op, ok)]: n random mutator calls over small id spaces, so that ids collide, are erased and come back; ok is
    False where covis_ref refuses the call (the mirror must answer VSLAM_ERR_INVALID and change nothing)"""
    rng = np.random.RandomState(seed)
    g = covis_ref.Graph()
    out = []
    for step in range(n):
        r = rng.rand()
        mp, kf = int(rng.randint(0, n_mp)), int(rng.randint(0, n_kf))
        if g.mps and r >= 0.18 and rng.rand() < 0.85:  # mostly a point that exists, for the calls that need one
            mp = sorted(g.mps)[int(rng.randint(0, len(g.mps)))]
        if g.kfs and r >= 0.18 and rng.rand() < 0.85:
            kf = sorted(g.kfs)[int(rng.randint(0, len(g.kfs)))]
        if step < n_kf:
            op = ("add_keyframe", step, step % 2, key_of(step))
        elif r < 0.04:
            op = ("add_keyframe", kf, int(rng.randint(0, 2)), key_of(kf + n_kf * int(rng.randint(0, 2))))
        elif r < 0.18:
            op = ("add_point", mp)
        elif r < 0.66:
            op = ("add_observation", mp, kf, int(rng.randint(-1, 500)), bool(rng.randint(0, 3) == 0), int(rng.randint(0, 9)),
                  bool(rng.randint(0, 4) == 0))
        elif r < 0.84:
            op = ("erase_observation", mp, kf)
        elif r < 0.88:
            op = ("clear_point", mp)
        elif r < 0.93:
            op = ("erase_point", mp)
        elif r < 0.97:
            op = ("erase_keyframe", kf)
        elif r < 0.98:
            op = ("set_keyframe_bad", kf)
        elif r < 0.99:
            op = ("set_keyframe_map", kf, int(rng.randint(0, 2)))
        elif r < 0.996:
            op = ("clear_map", int(rng.randint(0, 2)))
        else:
            op = ("clear",)
        try:
            getattr(g, op[0])(*op[1:])
            ok = True
        except covis_ref.Invalid:
            ok = False
        out.append((op, ok))
    return out
