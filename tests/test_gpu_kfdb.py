"""KeyFrameDatabase on the device (vslam_kfdb.hip) against tests/kfdb_ref.py: hit lists and L1 scores bit for bit,
the pool's growth / compaction / erase paths, argument errors, and the relocalisation chain end to end on real
descriptors."""
import ctypes as C

import numpy as np
import pytest

import kfdb_ref as R
import vi_slam_amd as V
from vi_slam_amd import synth

pytestmark = pytest.mark.gpu

NW, K = 20000, 300
HOT = 6000  # most word ids are drawn below this, so that pairs share dozens of words


@pytest.fixture(scope="module")
def fe():
    f = V.FExtractor(1000, 1.2, 8, 20, 7, 640, 480, max_batch=8)
    yield f
    f.close()


def assert_hits_equal(got, want, what=""):
    """bit for bit: ids, order, word counts, the double score (as uint64) and the float si (as uint32)"""
    assert got["kf"].tolist() == want["kf"].tolist(), what
    assert np.array_equal(got["map"], want["map"]) and np.array_equal(got["words"], want["words"]), what
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64)), what
    assert np.array_equal(got["si"].view(np.uint32), want["si"].view(np.uint32)), what


@pytest.fixture(scope="module")
def raw_case():
    """the database, the 32 queries and the reference's hit lists of the raw-query test, computed once"""
    rng = np.random.default_rng(2024)
    lens = [0, 1, 63, 64, 65, 129, 1500, 1200]
    kfs = []
    for k in range(K - 3):
        n = lens[k] if k < len(lens) else int(rng.integers(20, 400))
        ids, vals = R.random_bow(rng, NW, n, hi=17000 if k % 7 == 0 else HOT)
        if k % 9 == 4 and n:  # unnormalised values over fifteen decades
            vals = 10.0 ** rng.uniform(-12, 3, n)
        kfs.append((ids, vals))
    # a keyframe and a query whose only common word is the last word of both
    tail_kf = (np.append(np.sort(rng.choice(np.arange(19000, 19990), 40, replace=False)), NW - 1).astype(np.int32),
               np.full(41, 1.0 / 41))
    tail_q = (np.append(np.sort(rng.choice(np.arange(18000, 18990), 64, replace=False)), NW - 1).astype(np.int32),
              rng.dirichlet(np.ones(65)))
    kfs.append(tail_kf)
    kfs.append((kfs[7][0].copy(), kfs[7][1].copy()))  # the same BowVector as keyframe 7: equal first word, slot order decides
    kfs.append((kfs[7][0][:3].copy(), np.array([.5, .25, .25])))
    assert len(kfs) == K
    ref = R.RefDatabase(NW)
    for k, (ids, vals) in enumerate(kfs):
        ref.add(1000 + k, k % 3, ids, vals)
    queries = [(kfs[7][0].copy(), kfs[7][1].copy()),       # 1200 words, identical to keyframe 7 (and 298)
               (np.zeros(0, np.int32), np.zeros(0)),       # 0
               (kfs[20][0][:1].copy(), np.array([1.0])),   # 1
               (kfs[3][0].copy(), kfs[3][1].copy()),       # 64, identical to keyframe 3
               tail_q]                                     # 65
    while len(queries) < 32:
        n = int(rng.integers(1, 700))
        q = R.random_bow(rng, NW, n, hi=HOT if len(queries) % 4 else NW)
        if len(queries) % 5 == 0:
            q = (q[0], 10.0 ** rng.uniform(-12, 3, n))
        queries.append(q)
    assert [len(q[0]) for q in queries[:5]] == [1200, 0, 1, 64, 65]
    return dict(kfs=kfs, ref=ref, queries=queries, want=[ref.hits(q) for q in queries])


def test_raw_query_equals_reference_bit_for_bit(fe, raw_case):
    kfs, ref, queries, want = (raw_case[k] for k in ("kfs", "ref", "queries", "want"))
    db = V.KeyFrameDatabase(NW)
    try:
        for k, v in enumerate(kfs):
            db.add(1000 + k, k % 3, v)
        assert db.size() == ref.size() == (K, sum(len(v[0]) for v in kfs))
        for nq in (1, 3, 32):
            got = db.query(fe, queries[:nq])
            assert len(got) == nq
            for q in range(nq):
                assert_hits_equal(got[q], want[q], (nq, q))
        got = db.query(fe, queries)
    finally:
        db.close()
    # a query identical to a keyframe: L1-normalised, so the score is 1 (and both copies of the vector are found)
    h0 = {int(k): i for i, k in enumerate(got[0]["kf"])}
    assert got[0]["si"][h0[1007]] == np.float32(1.0) and got[0]["words"][h0[1007]] == 1200
    # ... and its common words straddle the 64-word passes of the kernel
    assert np.isin(queries[0][0][60:70], kfs[7][0]).all() and np.isin(queries[0][0][1150:], kfs[7][0]).all()
    # two keyframes with an equal first common word: slot (add) order decides; 1007 < 1298 < 1299 share the query's first word
    assert h0[1007] < h0[1000 + K - 2] < h0[1000 + K - 1]
    assert queries[0][0][0] == kfs[7][0][0] == kfs[K - 2][0][0] == kfs[K - 1][0][0]
    assert len(got[1]["kf"]) == 0 and len(got[2]["kf"]) >= 1 and 1003 in got[3]["kf"]
    # a pair whose only common word is the last word of both
    h4 = {int(k): i for i, k in enumerate(got[4]["kf"])}
    tail = 1000 + K - 3
    assert got[4]["words"][h4[tail]] == 1 and queries[4][0][-1] == kfs[K - 3][0][-1] == NW - 1
    assert np.intersect1d(queries[4][0], kfs[K - 3][0]).tolist() == [NW - 1]
    # teeth: on these inputs the order of the sum matters -- adding the same terms in descending word order changes the
    # double of at least a quarter of the hit pairs, so a kernel that reduced them in any other order would not pass
    changed = total = 0
    for q, w in zip(queries, want):
        for kf, s in zip(w["kf"], w["score"]):
            total += 1
            changed += R.l1_score_reversed(q, kfs[int(kf) - 1000]) != s
    print("hit pairs %d, changed by a reversed sum %d (%.0f %%)" % (total, changed, 100.0 * changed / total))
    assert total > 3000 and changed * 4 >= total


def _same(db, ref, fe, queries, what):
    assert db.size() == ref.size(), what
    for g, q in zip(db.query(fe, queries), queries):
        assert_hits_equal(g, ref.hits(q), what)


def test_mutations_growth_and_compaction(fe):
    """every keyframe holds word 0 and so does the first query: its hit list is the database in slot order"""
    nw = 2000
    rng = np.random.default_rng(77)

    def vec(n):
        ids, vals = R.random_bow(rng, nw, n, lo=1, hi=600)
        return np.insert(ids, 0, 0).astype(np.int32), np.insert(vals, 0, 0.01)
    queries = [vec(300), R.random_bow(rng, nw, 200, lo=1, hi=600)]
    db, ref = V.KeyFrameDatabase(nw, initial_entries=64), R.RefDatabase(nw)
    try:
        assert db.stats()["capacity"] == 64
        vs = {}
        for k in range(12):  # 12 x (40..130) entries into a pool of 64: it doubles several times
            vs[k] = vec(int(rng.integers(40, 130)))
            db.add(k, k % 2, vs[k])
            ref.add(k, k % 2, *vs[k])
        st = db.stats()
        assert st["growths"] >= 2 and st["capacity"] >= st["used"] == ref.size()[1] and st["compactions"] == 0
        _same(db, ref, fe, queries, "after the adds")
        for k in (0, 6, 11):  # first, middle, last
            db.erase(k)
            ref.erase(k)
            _same(db, ref, fe, queries, "erase %d" % k)
        db.erase(6)  # unknown now: nothing happens, as in the reference
        _same(db, ref, fe, queries, "second erase")
        db.add(6, 1, vs[0])  # an erased id comes back (with another vector) and goes last
        ref.add(6, 1, *vs[0])
        _same(db, ref, fe, queries, "re-add")
        assert db.query(fe, queries[:1])[0]["kf"][-1] == 6
        db.add(50, 0, (np.zeros(0, np.int32), np.zeros(0)))  # n = 0 is legal and never found
        ref.add(50, 0, [], [])
        _same(db, ref, fe, queries, "empty keyframe")
        db.clear_map(1)  # more than half of the entries die: the pool is compacted
        ref.clear_map(1)
        st = db.stats()
        assert st["compactions"] >= 1 and st["slots"] == db.size()[0] and st["used"] == db.size()[1]
        _same(db, ref, fe, queries, "clear_map")
        for k in (20, 21):  # adds behind a compaction land behind the survivors
            vs[k] = vec(90)
            db.add(k, 1, vs[k])
            ref.add(k, 1, *vs[k])
        _same(db, ref, fe, queries, "adds after the compaction")
        db.clear()
        ref.clear()
        assert db.size() == (0, 0)
        _same(db, ref, fe, queries, "clear")
        db.add(3, 0, vs[3])
        ref.add(3, 0, *vs[3])
        _same(db, ref, fe, queries, "add after clear")
    finally:
        db.close()


def test_argument_errors_leave_the_database_unchanged(fe):
    h = C.c_void_p()
    for scoring in (1, 2, 5, -1):
        assert V.lib().vslam_kfdb_create(0, 100, scoring, C.byref(h)) == V.ERR_UNSUPPORTED and not h.value
    with pytest.raises(V.VslamError) as e:
        V.KeyFrameDatabase(100, scoring=3)
    assert e.value.code == V.ERR_UNSUPPORTED
    db = V.KeyFrameDatabase(100)
    try:
        good = (np.array([1, 5, 99], np.int32), np.array([.5, .25, .25]))
        db.add(1, 0, good)
        for kf_id, ids in ((1, [2, 3]),        # duplicate keyframe
                           (2, [3, 3]), (2, [5, 4]),  # not strictly ascending
                           (2, [-1, 4]), (2, [4, 100])):  # out of range
            with pytest.raises(V.VslamError) as e:
                db.add(kf_id, 0, (np.array(ids, np.int32), np.array([.5, .5])))
            assert e.value.code == V.ERR_INVALID and db.size() == (1, 3)
        for bad in ([np.array([7, 7], np.int32)], [np.array([100], np.int32)], []):
            with pytest.raises(V.VslamError) as e:
                db.query(fe, [(b, np.ones(len(b))) for b in bad])
            assert e.value.code == V.ERR_INVALID
        with pytest.raises(V.VslamError) as e:
            db.query(fe, [good] * 33)
        assert e.value.code == V.ERR_INVALID and db.size() == (1, 3)
        got = db.query(fe, [good])[0]
        assert got["kf"].tolist() == [1] and got["words"].tolist() == [3] and got["score"][0] == 1.0
    finally:
        db.close()


def test_relocalisation_chain_on_real_descriptors(fe):
    """ComputeBoW -> KeyFrameDatabase -> candidates: eight frames of a moving scene, seven of them keyframes in two
    maps; the queries are the eighth frame and keyframe 2 itself."""
    voc = synth.make_vocabulary(10, 4)
    n_words = int(voc["word_id"].max()) + 1
    res = fe.compute_batch([synth.make_frame(640, 480, step=s) for s in range(8)])
    vv = V.Vocabulary(voc)
    try:
        vv.transform_slots_async(fe, 0, 8, 4)
        bows = [(b["bow_ids"].copy(), b["bow_vals"].copy()) for b in vv.transform_slots_wait([len(r[0]) for r in res])]
    finally:
        vv.close()
    assert all(len(b[0]) > 200 for b in bows)
    maps = [0, 0, 0, 1, 1, 0, 1]
    covis = {0: [1, 2], 1: [0, 2, 5], 2: [1, 0, 3], 3: [4, 6, 2], 4: [3, 6], 5: [1, 42], 6: [4, 3]}
    db, ref = V.KeyFrameDatabase(n_words), R.RefDatabase(n_words)
    try:
        for k in range(7):
            db.add(k, maps[k], bows[k])
            ref.add(k, maps[k], *bows[k])
        found = []
        for m, neigh in ((0, covis), (1, lambda k: covis[k])):  # neighbours as a dict and as a callable
            got = db.DetectRelocalizationCandidates(fe, bows[7], m, neigh)
            assert got == ref.DetectRelocalizationCandidates(bows[7], m, covis), m
            assert all(maps[k] == m for k in got)
            found += got
        assert found
        got = db.DetectNBestCandidates(fe, bows[7], 7, 0, [6], covis, 3)
        want = ref.DetectNBestCandidates(bows[7], 0, [6], covis, 3)
        assert got == (want[0], want[1]) and got[0] and 6 not in got[0] + got[1]
        # keyframe 2 against the database that holds it
        hits = db.query(fe, [bows[2]])[0]
        assert_hits_equal(hits, ref.hits(bows[2]), "self")
        assert hits["si"][hits["kf"].tolist().index(2)] == np.float32(1.0)
        got = db.DetectNBestCandidates(fe, bows[2], 2, 0, [], covis, 3)
        want = ref.DetectNBestCandidates(bows[2], 0, [], covis, 3)
        assert got == (want[0], want[1]) and got[0][0] == 2
        got = db.DetectNBestCandidates(fe, bows[2], 2, 0, [2, 1], covis, 3, bad_maps=[1])
        want = ref.DetectNBestCandidates(bows[2], 0, [2, 1], covis, 3, bad_maps=[1])
        assert got == (want[0], want[1]) and 2 not in got[0] and 1 not in got[0] and got[1] == []
        got = db.DetectRelocalizationCandidates(fe, bows[2], 0, covis)
        assert got == ref.DetectRelocalizationCandidates(bows[2], 0, covis) and got[0] == 2
        for k in ref.kfs.values():  # the scores the wrapper carries between queries are the reference's members
            assert np.float32(db.reloc_score.get(k.mnId, 0.0)) == k.mRelocScore
            assert np.float32(db.place_score.get(k.mnId, 0.0)) == k.mPlaceRecognitionScore
    finally:
        db.close()
