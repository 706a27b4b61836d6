"""Pure-Python restatement of the reference's KeyFrameDatabase for the tests: DBoW3's L1Scoring::score
(thirdparty/DBoW3/DBoW3/src/ScoringObject.cpp:23-68) and src/datastructures/keyframedatabase.cpp -- add (:21-27),
erase (:29-48), clear (:50-54), clearMap (:56-80), DetectNBestCandidates (:579-705) and DetectRelocalizationCandidates
(:707-811) -- with a real inverted file (one list per word) and the per-keyframe members the reference keeps.
Python floats are IEEE doubles; the reference's `float` variables are numpy.float32 here.

Deviations, as in DESIGN.md: mRelocScore starts at 0.0f (uninitialised in keyframe.cpp:20-38), and every query carries
a fresh query id (a counter), so the mn*Query(0) collision of a query with id 0 cannot happen."""
import numpy as np

F32 = np.float32


def l1_score(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68).  v = (strictly ascending word ids, values).  The reference walks both
    maps, skipping with lower_bound (:47-58) to the next word both hold; the words it stops at are the common ones in
    ascending order (found here by an intersection).  What decides the double it returns is the sum: the terms of the
    common words are added one after another, in ascending word order, into a double that starts at 0 (:32, :41)."""
    (i1, x1), (i2, x2) = v1, v2
    _, p1, p2 = np.intersect1d(i1, i2, assume_unique=True, return_indices=True)
    score = 0.0
    for vi, wi in zip(np.asarray(x1, np.float64)[p1].tolist(), np.asarray(x2, np.float64)[p2].tolist()):
        score += abs(vi - wi) - abs(vi) - abs(wi)  # :41, evaluated left to right
    return -score / 2.0  # :65


def l1_score_reversed(v1, v2):
    """The same terms added in DESCENDING word order: what a test uses to show that its data tell the orders apart."""
    (i1, x1), (i2, x2) = v1, v2
    _, p1, p2 = np.intersect1d(i1, i2, assume_unique=True, return_indices=True)
    score = 0.0
    for a, b in zip(p1[::-1], p2[::-1]):
        vi, wi = float(x1[a]), float(x2[b])
        score += abs(vi - wi) - abs(vi) - abs(wi)
    return -score / 2.0


class RefKeyFrame:
    def __init__(self, kf_id, map_id, ids, vals):
        self.mnId, self.map = kf_id, map_id
        self.mBowVec = (np.asarray(ids, np.int32).copy(), np.asarray(vals, np.float64).copy())
        self.mnRelocQuery = self.mnPlaceRecognitionQuery = None
        self.mnRelocWords = self.mnPlaceRecognitionWords = 0
        self.mRelocScore = F32(0.0)
        self.mPlaceRecognitionScore = F32(0.0)  # keyframe.cpp:20-38


class RefDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.kfs = {}  # the live KeyFrame objects by id
        self._query = 0

    # ---- keyframedatabase.cpp:21-80
    def add(self, kf_id, map_id, ids, vals):
        assert kf_id not in self.kfs
        kf = self.kfs[kf_id] = RefKeyFrame(kf_id, map_id, ids, vals)
        for w in kf.mBowVec[0]:
            self.mvInvertedFile[w].append(kf)  # push_back

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id, None)
        if kf is None:
            return
        for w in kf.mBowVec[0]:
            self.mvInvertedFile[w].remove(kf)  # the first (only) occurrence, order of the rest kept

    def clear(self):
        self.mvInvertedFile = [[] for _ in range(self.n_words)]
        self.kfs = {}

    def clear_map(self, map_id):
        for w in range(self.n_words):
            if self.mvInvertedFile[w]:
                self.mvInvertedFile[w] = [k for k in self.mvInvertedFile[w] if k.map != map_id]
        self.kfs = {i: k for i, k in self.kfs.items() if k.map != map_id}

    def size(self):
        return len(self.kfs), sum(len(k.mBowVec[0]) for k in self.kfs.values())

    # ---- the walk shared by both Detect functions, without exclusion: lKFsSharingWords and the word counts
    def walk(self, bow):
        """-> (keyframes in the order the walk first meets them, {kf: common words})"""
        order, words = [], {}
        for w in bow[0]:
            for kf in self.mvInvertedFile[w]:
                if kf not in words:
                    words[kf] = 0
                    order.append(kf)
                words[kf] += 1
        return order, words

    def hits(self, bow):
        """What vslam_kfdb_query_wait delivers for this query."""
        order, words = self.walk(bow)
        score = np.array([l1_score(bow, k.mBowVec) for k in order], np.float64)
        return dict(kf=np.array([k.mnId for k in order], np.int64), map=np.array([k.map for k in order], np.int32),
                    words=np.array([words[k] for k in order], np.int32), si=score.astype(np.float32), score=score)

    # ---- keyframedatabase.cpp:707-811
    def DetectRelocalizationCandidates(self, bow, map_id, neighbours):
        self._query += 1
        qid = ("F", self._query)
        lKFsSharingWords = []
        for w in bow[0]:  # :714-727
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != qid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = qid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = max(k.mnRelocWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))  # :740, int * float in float, truncated
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:  # :747-757
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch, bestAccScore = [], F32(0)
        for si, pKFi in lScoreAndMatch:  # :766-789
            bestScore, accScore, pBestKF = si, si, pKFi
            for nid in list(_neigh(neighbours, pKFi.mnId))[:10]:
                pKF2 = self.kfs.get(nid)
                if pKF2 is None or pKF2.mnRelocQuery != qid:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF, bestScore = pKF2, pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)  # :792
        added, out = set(), []
        for si, pKFi in lAccScoreAndMatch:  # :796-808
            if si > minScoreToRetain:
                if pKFi.map != map_id:
                    continue
                if pKFi not in added:
                    out.append(pKFi.mnId)
                    added.add(pKFi)
        return out

    # ---- keyframedatabase.cpp:579-705
    def DetectNBestCandidates(self, bow, map_id, connected, neighbours, n=3, bad_maps=()):
        self._query += 1
        qid = ("KF", self._query)
        spConnectedKF = set(connected)
        lKFsSharingWords = []
        for w in bow[0]:  # :590-610
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnPlaceRecognitionQuery != qid:
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi.mnId not in spConnectedKF:
                        pKFi.mnPlaceRecognitionQuery = qid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnPlaceRecognitionWords += 1
        if not lKFsSharingWords:
            return [], []
        maxCommonWords = max(k.mnPlaceRecognitionWords for k in lKFsSharingWords)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))  # :623
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:  # :630-641
            if pKFi.mnPlaceRecognitionWords > minCommonWords:
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mPlaceRecognitionScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return [], []
        lAccScoreAndMatch = []
        for si, pKFi in lScoreAndMatch:  # :650-675
            bestScore, accScore, pBestKF = si, si, pKFi
            for nid in list(_neigh(neighbours, pKFi.mnId))[:10]:
                pKF2 = self.kfs.get(nid)
                if pKF2 is None or pKF2.mnPlaceRecognitionQuery != qid:
                    continue
                accScore = F32(accScore + pKF2.mPlaceRecognitionScore)
                if pKF2.mPlaceRecognitionScore > bestScore:
                    pBestKF, bestScore = pKF2, pKF2.mPlaceRecognitionScore
            lAccScoreAndMatch.append((accScore, pBestKF))
        lAccScoreAndMatch.sort(key=lambda t: -float(t[0]))  # list::sort(compFirst): stable, descending (:677)
        vpLoopCand, vpMergeCand, spAlreadyAddedKF = [], [], set()
        i = 0
        while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < n or len(vpMergeCand) < n):  # :684-704
            pKFi = lAccScoreAndMatch[i][1]
            if pKFi not in spAlreadyAddedKF:
                if map_id == pKFi.map and len(vpLoopCand) < n:
                    vpLoopCand.append(pKFi.mnId)
                elif map_id != pKFi.map and len(vpMergeCand) < n and pKFi.map not in bad_maps:
                    vpMergeCand.append(pKFi.mnId)
                spAlreadyAddedKF.add(pKFi)
            i += 1
        return vpLoopCand, vpMergeCand


def _neigh(neighbours, kf_id):
    if callable(neighbours):
        return neighbours(kf_id)
    return (neighbours or {}).get(kf_id, ())


def random_bow(rng, n_words, n, normalised=True, lo=None, hi=None):
    """n distinct ascending word ids (inside [lo, hi) if given) with tf-idf-like positive values, L1-normalised."""
    lo, hi = (0 if lo is None else lo), (n_words if hi is None else hi)
    ids = np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False)).astype(np.int32)
    vals = rng.gamma(2.0, 1.0, size=n) * rng.uniform(0.5, 8.0, size=n)
    if normalised and n:
        vals = vals / np.sum(np.abs(vals))
    return ids, vals.astype(np.float64)
