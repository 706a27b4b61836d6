"""The covisibility mirror on the device against the line-by-line restatement tests/covis_ref.py: every output array of
every job for equality, at the smallest shapes where the kernels can go wrong (slot counts around a wave and around the LDS
histogram limit, list lengths around a wave and at the maximum, 1 / 2 / 128 jobs, every segment size of the pool), the
census cases, mutate -> query chains with growth, compaction and a re-added keyframe id, and the async discipline."""
import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
import vi_slam_amd as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = V.FExtractor(500, 1.2, 8, 20, 7, 320, 240, max_batch=1)
    yield f
    f.close()


def check_connections(cov, fe, g, jobs):
    got = cov.connections(fe, jobs)
    assert len(got) == len(jobs)
    for r, job in zip(got, jobs):
        CC.same_connections(r, g.connections(job))
    return got


def check_culling(cov, fe, g, jobs, th_obs=3):
    assert cov.culling(fe, jobs, th_obs) == [g.culling(j, th_obs) for j in jobs]


def both(ops, initial_entries=0):
    return CC.build(ops), CC.build(ops, V.CovisibilityMap(initial_entries=initial_entries))


def random_list(rng, n, n_mp):
    """ids with repeats and NULLs"""
    return [None if v < 0 else int(v) for v in rng.randint(-n_mp // 8 - 1, n_mp, size=n)]


@pytest.fixture(scope="module")
def small_scene():
    """30 keyframes of two maps, 300 points with up to 6 observers, three bad keyframes; computed once, never changed"""
    ops = CC.random_scene(30, 300, 6, seed=17, n_maps=2) + [("set_keyframe_bad", k) for k in (3, 11, 20)]
    g, cov = both(ops)
    yield g, cov
    cov.close()


def test_census_cases_with_both_modes_in_one_enqueue(fe):
    ops, jobs = CC.connections_scene()
    g, cov = both(ops, initial_entries=16)
    assert {j["mode"] for j in jobs} == {CC.CONN, CC.VOTE}
    got = check_connections(cov, fe, g, jobs)
    assert got[7]["error"] == 1 and got[8]["error"] == 2 and list(got[0]["ordered_w"][:2]) == [21, 21]
    ops, jobs = CC.culling_scene()
    g, cov2 = both(ops, initial_entries=16)
    check_culling(cov2, fe, g, jobs)
    check_culling(cov2, fe, g, jobs, th_obs=2)
    for m in g.mps:
        CC.same_point(cov2.get_point(m), g.get_point(m))


@pytest.mark.parametrize("which", ["1", "63", "64", "65", "lds-1", "lds", "lds+1"])
def test_keyframe_slot_counts(fe, which):
    lim = V.CovisibilityMap.limits()
    assert lim["max_jobs"] == 128 and lim["max_list"] == 8192
    R = {"lds-1": lim["lds_slots"] - 1, "lds": lim["lds_slots"], "lds+1": lim["lds_slots"] + 1}.get(which) or int(which)
    rng = np.random.RandomState(R)
    kf = np.arange(R)
    ops = [("add_keyframes", kf, kf % 1, np.array([CC.key_of(int(k)) for k in kf], np.uint64))]
    by_key = sorted(range(R), key=CC.key_of)
    ends = sorted({by_key[0], by_key[-1], by_key[R // 2], by_key[min(63, R - 1)], by_key[min(64, R - 1)], by_key[max(R - 65, 0)]})
    for mp in range(40):  # a handful of observations each: the ends of the key order, and a few anywhere
        ops.append(("add_point", mp))
        seen = set(ends if mp < 30 else ends[:2]) | {int(k) for k in rng.randint(0, R, size=4)}
        for k in sorted(seen):
            ops.append(("add_observation", mp, k, mp, False, int(rng.randint(0, 8)), False))
    g, cov = both(ops)
    lst = list(range(40)) + [None, 5]
    jobs = [dict(mode=CC.CONN, self_kf=ends[0], map_id=0, min_obs=0, mp_ids=lst), dict(mode=CC.VOTE, map_id=0, min_obs=7, mp_ids=lst),
            dict(mode=CC.CONN, self_kf=int(rng.randint(0, R)), map_id=0, min_obs=1, mp_ids=lst[:7])]
    got = check_connections(cov, fe, g, jobs)
    if R > 1:
        assert len(got[1]["counter_kf"]) >= min(R, len(ends)) and got[1]["n_max"] >= 30
    check_culling(cov, fe, g, [dict(kf_id=ends[0], mp_ids=lst, levels=[i % 8 for i in range(len(lst))])])
    cov.close()


@pytest.mark.parametrize("n", [0, 1, 64, 65, 8192])
def test_list_lengths(fe, small_scene, n):
    g, cov = small_scene
    rng = np.random.RandomState(n)
    lst = random_list(rng, n, 300)
    check_connections(cov, fe, g, [dict(mode=CC.CONN, self_kf=4, map_id=0, min_obs=3, mp_ids=lst),
                                   dict(mode=CC.VOTE, map_id=0, min_obs=0, mp_ids=lst)])
    check_culling(cov, fe, g, [dict(kf_id=4, mp_ids=lst, levels=list(rng.randint(0, 8, size=n)))])


@pytest.mark.parametrize("n_jobs", [1, 2, 128])
def test_jobs_per_enqueue(fe, small_scene, n_jobs):
    g, cov = small_scene
    rng = np.random.RandomState(100 + n_jobs)
    jobs = [dict(mode=j % 2, self_kf=j % 30, map_id=j % 2, min_obs=j % 5, mp_ids=random_list(rng, int(rng.randint(0, 200)), 300))
            for j in range(n_jobs)]
    check_connections(cov, fe, g, jobs)
    check_culling(cov, fe, g, [dict(kf_id=j["self_kf"], mp_ids=j["mp_ids"], levels=list(rng.randint(0, 8, size=len(j["mp_ids"]))))
                               for j in jobs])


def test_129_jobs_are_refused(fe, small_scene):
    g, cov = small_scene
    job = dict(mode=CC.CONN, self_kf=1, map_id=0, min_obs=0, mp_ids=[1, 2])
    for call in (lambda: cov.connections(fe, [job] * 129), lambda: cov.connections(fe, []),
                 lambda: cov.culling(fe, [dict(kf_id=1, mp_ids=[1], levels=[0])] * 129),
                 lambda: cov.connections(fe, [dict(job, mp_ids=[1] * 8193)])):
        with pytest.raises(V.VslamError) as e:
            call()
        assert e.value.code == V.ERR_INVALID
    check_connections(cov, fe, g, [job])  # and the mirror goes on working


def test_every_segment_size_is_read_by_a_kernel(fe):
    sizes = [0, 1, 2, 3, 4, 5, 8, 9, 17, 300]
    kf = np.arange(320)
    ops = [("add_keyframes", kf, kf * 0, np.array([CC.key_of(int(k)) for k in kf], np.uint64))]
    for mp, n in enumerate(sizes):
        ops.append(("add_point", mp))
        ops += [("add_observation", mp, (k * 7 + mp) % 320, k, k % 5 == 0, (k + mp) % 8, k % 4 == 0) for k in range(n)]
    g, cov = both(ops, initial_entries=8)
    assert cov.stats()["growths"] >= 1
    lst = list(range(len(sizes)))
    check_connections(cov, fe, g, [dict(mode=CC.CONN, self_kf=7, map_id=0, min_obs=2, mp_ids=lst), dict(mode=CC.VOTE, mp_ids=lst)])
    check_culling(cov, fe, g, [dict(kf_id=k, mp_ids=lst, levels=[3] * len(lst)) for k in (7, 9, 300)])
    for m in g.mps:
        CC.same_point(cov.get_point(m), g.get_point(m))
    cov.close()


def test_mutate_query_mutate_query(fe):
    """nothing between a mutation and the next query: a stale upload shows as a difference"""
    ops = CC.random_scene(24, 60, 5, seed=9)
    g, cov = both(ops, initial_entries=512)
    rng = np.random.RandomState(9)
    lists = [random_list(rng, 80, 60) for _ in range(4)]

    def query():
        check_connections(cov, fe, g, [dict(mode=j % 2, self_kf=j, map_id=0, min_obs=j, mp_ids=lists[j]) for j in range(4)])
        check_culling(cov, fe, g, [dict(kf_id=j, mp_ids=lists[j], levels=[2] * 80) for j in range(4)])

    def mutate(ops):
        CC.apply(g, ops)
        CC.apply(cov, ops)
    query()
    st0 = cov.stats()
    mutate([("add_observation", 5, 3, 77, False, 1, True), ("set_keyframe_bad", 2)])  # one record, one keyframe flag
    query()
    grow = [("add_point", 1000 + i) for i in range(150)]
    grow += [("add_observation", 1000 + i, (i + k) % 24, i, False, k, False) for i in range(150) for k in range(5)]
    mutate(grow)  # 150 segments of 4 then 8 records: the pool of 512 grows
    lists[0] = lists[0][:40] + [1000 + i for i in range(40)]
    query()
    st1 = cov.stats()
    assert st1["growths"] > st0["growths"] and st1["compactions"] == st0["compactions"]
    mutate([("erase_point", 1000 + i) for i in range(40, 150)] + [("clear_point", m) for m in range(0, 60, 2)])
    assert cov.stats()["compactions"] > st1["compactions"]  # abandoned segments exceed half of what was handed out
    query()
    # a keyframe id leaves and comes back with another key and map: its slot is reused
    gone = [m for m, mp in g.mps.items() if 6 in mp.mObservations]
    mutate([("erase_observation", m, 6) for m in gone] + [("erase_keyframe", 6), ("add_keyframe", 6, 0, CC.key_of(5000)),
                                                          ("add_observation", 1001, 6, 9, True, 0, False),
                                                          ("add_observation", 1002, 6, 9, False, 4, False)])
    query()
    mutate([("clear_map", 0)])
    assert cov.size() == g.size() == (0, len(g.mps), 0)
    assert cov.connections(fe, [dict(mode=CC.VOTE, mp_ids=[None])])[0]["n_tracked"] == 0
    cov.close()


def test_async_discipline(fe):
    ops, jobs = CC.connections_scene()
    g, cov = both(ops)
    with pytest.raises(V.VslamError) as e:  # a wait with nothing enqueued
        cov.connections_wait()
    assert e.value.code == V.ERR_INVALID
    want = [g.connections(j) for j in jobs]
    cov.connections_async(fe, jobs)
    with pytest.raises(V.VslamError) as e:  # one query per mirror
        V._check(V.lib().vslam_covis_connections_async(cov._h, fe._h, 1, cov._jobs(jobs[:1])[0]))
    assert e.value.code == V.ERR_INVALID
    with pytest.raises(V.VslamError) as e:  # the other query's wait
        V._check(V.lib().vslam_covis_culling_wait(cov._h, fe._h, (V._CovisCullResult * 16)()))
    assert e.value.code == V.ERR_INVALID
    # a mutator while the query is in flight settles; the results are those of the state before it
    mut = [("add_observation", 0, 8, 5, False, 0, False), ("set_keyframe_bad", 1), ("clear_point", 3)]
    CC.apply(cov, mut)
    CC.apply(g, mut)
    for r, w in zip(cov.connections_wait(), want):
        CC.same_connections(r, w)
    check_connections(cov, fe, g, jobs)  # and the next query sees the mutations
    assert g.connections(jobs[0]) != want[0]
    fe.set_profiling(True)
    check_connections(cov, fe, g, jobs)
    fe.set_profiling(False)
    p = cov.profile()
    assert p["passes"] == 1 and p["query_ms"] > 0
    cov.close()
