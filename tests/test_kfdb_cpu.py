"""KeyFrameDatabase without a GPU: the restated L1Scoring::score against literals worked out by hand, and the
selection stage of libvslam_host.so (vslam_kfdb_select_relocalization / _nbest) against tests/kfdb_ref.py on hit lists
that a RefDatabase produced."""
import ctypes as C

import numpy as np
import pytest

import kfdb_ref as R
import vi_slam_amd as V

NW = 500  # vocabulary words of the hand-made cases
Q_IDS = np.arange(0, 40, 2, dtype=np.int32)  # the query: 20 words, even ids


def bow(ids, vals):
    return np.asarray(ids, np.int32), np.asarray(vals, np.float64)


# ------------------------------------------------------------------ l1_score against hand-worked literals
def test_l1_score_two_of_three_words_shared():
    """v = {1: .5, 4: .25, 9: .25}, w = {1: .25, 4: .5, 7: .25}: words 1 and 4 are common, each term is
    |.25| - .5 - .25 = -.5 resp. |-.25| - .25 - .5 = -.5, the sum -1, the score 0.5 (all exact in binary)."""
    assert R.l1_score(bow([1, 4, 9], [.5, .25, .25]), bow([1, 4, 7], [.25, .5, .25])) == 0.5


def test_l1_score_identical_normalised_vectors_is_one():
    v = bow([3, 5, 8, 13], [.125, .5, .25, .125])
    assert R.l1_score(v, v) == 1.0


def test_l1_score_disjoint_vectors():
    """no common word: the sum stays +0.0 and -0.0 / 2 is returned"""
    s = R.l1_score(bow([1, 3], [.5, .5]), bow([2, 4], [.5, .5]))
    assert s == 0.0 and np.signbit(s)


def test_l1_score_adds_in_ascending_word_order():
    """equal vectors {1: 2^52, 2: .5, 3: .5}: the terms are -2^53, -1, -1.  Ascending: -2^53 - 1 rounds back to -2^53
    (ties to even) twice, score 2^52; descending: -1 - 1 = -2, then -(2^53 + 2) exactly, score 2^52 + 1."""
    v = bow([1, 2, 3], [2.0 ** 52, .5, .5])
    assert R.l1_score(v, v) == 2.0 ** 52 and R.l1_score_reversed(v, v) == 2.0 ** 52 + 1


# ------------------------------------------------------------------ hit lists from a RefDatabase
def make_kf(rng, shared, extra, first_private=100, weight=None):
    """a keyframe's BowVector: the query words Q_IDS[shared] plus `extra` private odd word ids; L1-normalised"""
    ids = np.concatenate([Q_IDS[list(shared)], first_private + 1 + 2 * rng.choice(120, extra, replace=False)]).astype(np.int32)
    vals = rng.uniform(0.5, 2.0, len(ids)) if weight is None else np.full(len(ids), weight)
    o = np.argsort(ids)
    vals = vals[o] / vals.sum()
    return ids[o], vals


def query(rng):
    vals = rng.uniform(0.5, 2.0, len(Q_IDS))
    return Q_IDS.copy(), vals / vals.sum()


class Pair:
    """a RefDatabase and the state the Python wrapper keeps (the two stale-score dicts), driven side by side"""

    def __init__(self):
        self.db, self.reloc, self.place = R.RefDatabase(NW), {}, {}

    def add(self, kf_id, map_id, v):
        self.db.add(kf_id, map_id, *v)

    def _io(self, hits, stale):
        return np.array([stale.get(int(k), 0.0) for k in hits["kf"]], np.float32)

    def reloc_both(self, q, map_id, neigh):
        hits = self.db.hits(q)
        io = self._io(hits, self.reloc)
        got = V.kfdb_select_relocalization(hits, io, map_id, neigh)
        self.reloc.update({int(k): float(v) for k, v in zip(hits["kf"], io)})
        want = self.db.DetectRelocalizationCandidates(q, map_id, neigh)
        assert got == want
        for k in self.db.kfs.values():  # mRelocScore of every keyframe, scored by this query or not
            assert np.float32(self.reloc.get(k.mnId, 0.0)) == k.mRelocScore
        return got, hits

    def nbest_both(self, q, map_id, connected, neigh, n=3, bad_maps=()):
        hits = self.db.hits(q)
        io = self._io(hits, self.place)
        got = V.kfdb_select_nbest(hits, io, map_id, connected, neigh, n, bad_maps)
        self.place.update({int(k): float(v) for k, v in zip(hits["kf"], io)})
        want = self.db.DetectNBestCandidates(q, map_id, connected, neigh, n, bad_maps)
        assert got == (list(want[0]), list(want[1]))
        for k in self.db.kfs.values():
            assert np.float32(self.place.get(k.mnId, 0.0)) == k.mPlaceRecognitionScore
        return got, hits


def test_empty_hit_list():
    rng, p = np.random.default_rng(1), Pair()
    p.add(1, 0, make_kf(rng, [], 10))
    got, hits = p.reloc_both(query(rng), 0, {})
    assert got == [] and len(hits["kf"]) == 0
    assert p.nbest_both(query(rng), 0, [], {})[0] == ([], [])


def test_one_hit():
    rng, p = np.random.default_rng(2), Pair()
    p.add(7, 0, make_kf(rng, [3], 5))
    assert p.reloc_both(query(rng), 0, {})[0] == [7]
    assert p.reloc_both(query(rng), 1, {})[0] == []  # another map
    assert p.nbest_both(query(rng), 0, [], {})[0] == ([7], [])
    assert p.nbest_both(query(rng), 1, [], {})[0] == ([], [7])


def test_min_common_words_is_a_float_product_truncated():
    """minCommonWords = (int)(maxCommonWords * 0.8f).  0.8f is a little ABOVE 0.8, so the product could exceed an
    integer that m * 4 / 5 reaches exactly; it never does: for multiples of 5 the float product rounds back to the
    integer itself and otherwise the fraction is at least 0.2.  Checked here for every m up to 2^20 -- no m with
    (int)(m * 0.8f) != m * 4 / 5 exists in any range a BowVector can reach -- so the case tests the boundaries instead:
    max = 5, 10, 20 give min = 4, 8, 16, a hit with exactly min words is not scored, one with min + 1 is."""
    m = np.arange(1, 1 << 20)
    assert np.array_equal((m.astype(np.float32) * np.float32(0.8)).astype(np.int64), m * 4 // 5)
    for mx in (5, 10, 20):
        mn = mx * 4 // 5
        rng, p = np.random.default_rng(mx), Pair()
        p.add(1, 0, make_kf(rng, range(mn), 3))      # exactly min: sharing, not scored
        p.add(2, 0, make_kf(rng, range(mx), 3))      # the maximum
        p.add(3, 0, make_kf(rng, range(mn + 1), 30))  # min + 1: scored, but far from the best score
        (got, hits) = p.reloc_both(query(rng), 0, {})
        assert hits["words"].tolist() == [mn, mx, mn + 1] and 2 in got and 1 not in got
        assert p.reloc[1] == 0.0 and p.reloc[2] > 0.0 and p.reloc[3] > 0.0


def test_only_the_maximum_is_scored():
    rng, p = np.random.default_rng(4), Pair()
    for k, sh in enumerate([range(8), range(2, 10), range(10), range(3), range(12, 20)]):
        p.add(10 + k, 0, make_kf(rng, sh, 4))
    got, hits = p.reloc_both(query(rng), 0, {10: [11, 12], 12: [10, 11, 13]})
    assert got == [12] and hits["words"].max() == 10
    assert [k for k, v in p.reloc.items() if v != 0.0] == [12]


def test_neighbours_excluded_absent_and_stale():
    """Query A scores keyframe 5 high.  Query B shares too few words with 5 to score it, but 5 is a neighbour of the
    scored keyframes: its STALE score of query A is accumulated, as the reference reads the old member.  Neighbour 99
    is not in the database, 6 is not a hit of B, and (N-best) a connected keyframe is neither listed nor accumulated."""
    rng, p = np.random.default_rng(5), Pair()
    p.add(5, 0, make_kf(rng, [0, 1], 12, first_private=200))
    qa = bow(*p.db.kfs[5].mBowVec)  # identical to keyframe 5
    p.add(6, 0, make_kf(rng, [], 6))
    p.add(1, 0, make_kf(rng, range(10), 2))
    p.add(2, 0, make_kf(rng, range(1, 11), 2))
    p.add(3, 1, make_kf(rng, range(9), 2))
    assert p.reloc_both(qa, 0, {})[0] == [5] and p.reloc[5] == 1.0
    assert p.nbest_both(qa, 0, [], {})[0][0][0] == 5 and p.place[5] == 1.0
    neigh = {1: [5, 99, 6, 2], 2: [99, 5], 3: [5, 99]}
    got, hits = p.reloc_both(query(rng), 0, neigh)
    assert dict(zip(hits["kf"].tolist(), hits["words"].tolist()))[5] == 2
    assert got == [5] and p.reloc[5] == 1.0  # the stale 1.0 beats every fresh score: pBestKF = 5 three times, listed once
    got, _ = p.nbest_both(query(rng), 0, [], neigh)
    assert got == ([5], [])
    got, _ = p.nbest_both(query(rng), 0, [5], neigh)  # connected: 5 is not seen by the neighbour step any more
    assert 5 not in got[0] and got[0] and got[1] == [3]
    got, _ = p.nbest_both(query(rng), 0, [1, 2, 3, 5], neigh)  # everything sharing words is connected
    assert got == ([], [])


def test_best_keyframe_replaced_by_neighbour_and_deduplicated():
    rng, p = np.random.default_rng(6), Pair()
    p.add(1, 0, make_kf(rng, range(17), 20))
    p.add(2, 0, make_kf(rng, range(2, 19), 20))
    p.add(3, 0, make_kf(rng, range(20), 0))  # the query's words, nothing else: by far the best score
    p.add(4, 0, make_kf(rng, range(18), 25))
    neigh = {1: [3], 2: [4, 3], 4: [1]}
    got, _ = p.reloc_both(query(rng), 0, neigh)
    assert got == [3] or got[0] == 3 and got.count(3) == 1
    loop, merge = p.nbest_both(query(rng), 0, [], neigh)[0]
    assert loop.count(3) == 1 and merge == []


def test_nbest_ties_keep_hit_order_and_fewer_than_n():
    """keyframes 21, 22, 23 carry one and the same BowVector: equal si, equal accScore; list::sort is stable, so they
    stay in hit order (add order, since their first common word is the same)"""
    rng, p = np.random.default_rng(7), Pair()
    v = make_kf(rng, range(15), 3)
    p.add(20, 0, make_kf(rng, range(14), 30))
    for k in (23, 21, 22):
        p.add(k, 0, v)
    p.add(30, 2, v)
    (loop, merge), _ = p.nbest_both(query(rng), 0, [], {}, n=2)
    assert loop == [23, 21] and merge == [30]
    (loop, merge), _ = p.nbest_both(query(rng), 0, [], {}, n=10)  # fewer than n
    assert loop[:3] == [23, 21, 22] and len(loop) == 4 and merge == [30]
    assert p.nbest_both(query(rng), 0, [], {}, n=0)[0] == ([], [])


def test_nbest_bad_map_and_vectors_filling_at_different_times():
    """Map 0 is the query's, 1 is bad, 2 and 3 are good.  The loop vector is full after two entries while the merge
    vector still waits: later loop-map keyframes enter spAlreadyAddedKF without being taken, bad-map keyframes too."""
    rng, p = np.random.default_rng(8), Pair()
    maps = [0, 0, 1, 0, 1, 2, 0, 3, 2]
    for k, m in enumerate(maps):
        p.add(40 + k, m, make_kf(rng, range(k % 3, 14 + k % 3), 2 + k))
    neigh = {40: [42], 43: [44, 45], 46: [47]}
    (loop, merge), hits = p.nbest_both(query(rng), 0, [], neigh, n=2, bad_maps=[1])
    assert len(loop) == 2 and len(merge) == 2 and all(p.db.kfs[k].map == 0 for k in loop)
    assert all(p.db.kfs[k].map in (2, 3) for k in merge)
    (loop, merge), _ = p.nbest_both(query(rng), 0, [], neigh, n=3, bad_maps=[1, 2])
    assert merge == [47] and len(loop) == 3
    (loop, merge), _ = p.nbest_both(query(rng), 2, [], neigh, n=5, bad_maps=[])
    assert sorted(loop) == [45, 48] and len(merge) == 5


def test_random_sequences_equal_reference():
    """several queries against one database, stale scores carried from query to query, both functions"""
    rng, p = np.random.default_rng(9), Pair()
    for k in range(40):
        p.add(k, k % 3, make_kf(rng, rng.choice(20, rng.integers(1, 20), replace=False), int(rng.integers(0, 30))))
    neigh = {k: rng.choice(45, rng.integers(0, 13), replace=False).tolist() for k in range(40)}
    for it in range(12):
        q = query(rng)
        q = (q[0][it % 4:], q[1][it % 4:])
        p.reloc_both(q, it % 3, neigh)
        p.nbest_both(q, it % 3, rng.choice(40, 5, replace=False).tolist(), lambda k: neigh.get(k, ()), n=1 + it % 4,
                     bad_maps=[2] if it % 2 else [])


# ------------------------------------------------------------------ argument validation
def test_select_argument_validation():
    L = V.host_lib()
    kf, mp, wd = np.array([1, 2], np.int64), np.zeros(2, np.int32), np.array([4, 4], np.int32)
    si, io, out = np.array([.5, .5], np.float32), np.zeros(2, np.float32), np.zeros(4, np.int64)
    n1, n2, p, nocb = C.c_int(), C.c_int(), V._p, V.KFDB_NEIGHBOURS_FN()
    rel = L.vslam_kfdb_select_relocalization
    assert rel(p(kf), p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, p(out), 4, C.byref(n1)) == 0 and n1.value == 2
    assert rel(p(kf), p(mp), p(wd), p(si), -1, p(io), 0, nocb, None, p(out), 4, C.byref(n1)) == V.ERR_INVALID
    assert rel(None, p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, p(out), 4, C.byref(n1)) == V.ERR_INVALID
    assert rel(p(kf), p(mp), p(wd), p(si), 2, None, 0, nocb, None, p(out), 4, C.byref(n1)) == V.ERR_INVALID
    assert rel(p(kf), p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, p(out), 4, None) == V.ERR_INVALID
    assert rel(p(kf), p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, None, 4, C.byref(n1)) == V.ERR_INVALID
    assert rel(p(kf), p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, p(out), -1, C.byref(n1)) == V.ERR_INVALID
    assert rel(p(kf), p(mp), p(wd), p(si), 2, p(io), 0, nocb, None, p(out), 1, C.byref(n1)) == V.ERR_CAPACITY
    assert n1.value == 2
    assert rel(None, None, None, None, 0, None, 0, nocb, None, None, 0, C.byref(n1)) == 0 and n1.value == 0
    nb = L.vslam_kfdb_select_nbest
    lo, me, conn, bad = np.zeros(3, np.int64), np.zeros(3, np.int64), np.array([2], np.int64), np.array([1], np.int32)

    def call(**kw):
        a = dict(kf=p(kf), n=2, io=p(io), conn=p(conn), nc=1, cand=3, bad=p(bad), nbad=1, lo=p(lo), nl=C.byref(n1),
                 me=p(me), nm=C.byref(n2))
        a.update(kw)
        return nb(a["kf"], p(mp), p(wd), p(si), a["n"], a["io"], 0, a["conn"], a["nc"], a["cand"], a["bad"], a["nbad"],
                  nocb, None, a["lo"], a["nl"], a["me"], a["nm"])
    assert call() == 0 and (n1.value, n2.value, lo[0]) == (1, 0, 1)
    for bad_args in (dict(kf=None), dict(n=-1), dict(io=None), dict(conn=None), dict(nc=-1), dict(cand=-1),
                     dict(bad=None), dict(nbad=-1), dict(lo=None), dict(me=None), dict(nl=None), dict(nm=None)):
        assert call(**bad_args) == V.ERR_INVALID, bad_args
    assert call(conn=None, nc=0, bad=None, nbad=0) == 0 and n1.value == 2
