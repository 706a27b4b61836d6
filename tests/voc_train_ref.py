"""TEST INFRASTRUCTURE: numpy restatement of DBoW3::Vocabulary::create (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp:157-571,
DescManip.cpp:25-73) with the draws of include/vslam_fe.h in place of rand().  It is the yardstick of vslam_voc_train
(device) and vslamh_voc_train (host twin): written from the reference's rules as a plain recursion, it shares no code
with either.

train(desc, doc_offsets, k, L, ...) returns the vocabulary as a dict in read_vocabulary_file's layout (DBoW3's node
order, which the recursion produces by itself), "stats" with the branch counters of vslam_voc_train_stats, "word_of"
(the word of every training feature) and "dist_sums" (per k-means node: every dist_sum of its seeding, as Python ints)."""
import math

import numpy as np

M64 = (1 << 64) - 1
POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)
RAND_MAX = 2147483647
ZERO_DRAW_LIMIT = 64
DEFAULT_MAX_ITER = 10000


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def child_key(parent, c):
    return mix(parent ^ (((c + 1) * 0x9E3779B97F4A7C15) & M64))


def draw(key, j, mask):
    return (mix(key ^ (((j + 1) * 0xD1B54A32D192ED03) & M64)) >> 33) & mask


def hamming(block, one):
    """DescManip::distance of every row of block (n x 32 uint8) to one descriptor"""
    return POP[block ^ one[None, :]].sum(axis=1, dtype=np.int64)


def mean_value(group):
    """DescManip::meanValue of a non-empty group (n x 32 uint8): bit set iff its count >= n / 2 + n % 2"""
    n = len(group)
    if n == 1:
        return group[0].copy()
    bits = np.unpackbits(group, axis=1).sum(axis=0, dtype=np.int64)
    return np.packbits(bits >= n // 2 + n % 2)


class _Trainer:
    def __init__(self, desc, k, L, seed, rand_mask, max_iter):
        self.desc, self.k, self.L, self.mask = desc, k, L, rand_mask
        self.max_iter = max_iter or DEFAULT_MAX_ITER
        self.parent, self.node_desc, self.children, self.level = [0], [np.zeros(32, np.uint8)], [[]], [0]
        self.st = dict(max_passes=0, total_passes=0, hit_max_iter=0, early_stops=0, draws=0, redraws=0, small_nodes=0,
                       single_leaves=0, empty_groups=0)
        self.dist_sums = []
        self.step(0, np.arange(len(desc)), 1, mix(seed & M64))

    def seed_clusters(self, feats, key):
        """initiateClustersKMpp (:409-491)"""
        n, j = len(feats), 0
        clusters = [feats[draw(key, j, self.mask) % n].copy()]
        j += 1
        min_d = hamming(feats, clusters[0])
        sums = []
        while len(clusters) < self.k:
            d = hamming(feats, clusters[-1])
            upd = (min_d > 0) & (d < min_d)
            min_d = np.where(upd, d, min_d)
            dist_sum = int(min_d.sum())
            sums.append((dist_sum, float(np.add.reduce(min_d.astype(np.float64)))))
            if dist_sum == 0:
                self.st["early_stops"] += 1
                break
            zeros = 0
            while True:
                r = draw(key, j, self.mask)
                j += 1
                if r != 0:
                    break
                self.st["redraws"] += 1
                zeros += 1
                if zeros == ZERO_DRAW_LIMIT:
                    r = 1
                    break
            cut_d = (float(r) / float(RAND_MAX)) * float(dist_sum)
            up = np.cumsum(min_d)
            hit = np.flatnonzero(up.astype(np.float64) >= cut_d)
            clusters.append(feats[int(hit[0]) if len(hit) else n - 1].copy())
        self.st["draws"] += j
        self.dist_sums.append(sums)
        return clusters

    def step(self, parent, idx, level, key):
        """HKmeansStep (:233-394); idx ascending"""
        n = len(idx)
        if n == 0:
            return
        feats = self.desc[idx]
        if n <= self.k:
            self.st["small_nodes"] += 1
            clusters, assoc = [f.copy() for f in feats], np.arange(n)
        else:
            clusters = self.seed_clusters(feats, key)
            assoc, last, passes = None, None, 0
            while True:
                if passes > 0:
                    for c in range(len(clusters)):
                        group = feats[assoc == c]
                        if len(group) == 0:
                            self.st["empty_groups"] += 1
                        else:
                            clusters[c] = mean_value(group)
                dist = np.stack([hamming(feats, c) for c in clusters], axis=1)
                assoc = np.argmin(dist, axis=1)  # the first minimum: strict < keeps the lowest cluster
                passes += 1
                if passes > 1 and np.array_equal(assoc, last):
                    break
                if passes >= self.max_iter:
                    self.st["hit_max_iter"] += 1
                    break
                last = assoc
            self.st["total_passes"] += passes
            self.st["max_passes"] = max(self.st["max_passes"], passes)
        ids = []
        for c in clusters:
            ids.append(len(self.parent))
            self.parent.append(parent)
            self.node_desc.append(c)
            self.children.append([])
            self.level.append(level)
            self.children[parent].append(ids[-1])
        if level >= self.L:
            return
        for c, nid in enumerate(ids):
            sub = idx[assoc == c]
            if len(sub) > 1:
                self.step(nid, sub, level + 1, child_key(key, c))
            elif len(sub) == 1:
                self.st["single_leaves"] += 1


def transform_words(voc, desc):
    """Vocabulary::transform(feature, word_id) (:880-...) for every row: strict <, the first child wins"""
    n = len(desc)
    node = np.zeros(n, np.int64)
    cs, cc, ci, nd = voc["child_start"], voc["child_count"], voc["child_ids"], voc["desc"]
    active = np.arange(n)
    while len(active):
        nxt = []
        cur = node[active]
        for p in np.unique(cur):
            sel = active[cur == p]
            ch = ci[cs[p]:cs[p] + cc[p]]
            dist = np.stack([hamming(desc[sel], nd[c]) for c in ch], axis=1)
            node[sel] = ch[np.argmin(dist, axis=1)]
            nxt.append(sel[cc[node[sel]] > 0])
        active = np.concatenate(nxt) if nxt else np.zeros(0, np.int64)
    return voc["word_id"][node].astype(np.int32)


def simulate_node_order(child_lists):
    """ids in the order of the HKmeansStep calls over a finished tree given as {node: [children]} in any labelling:
    a call numbers its children consecutively, then descends into every child that has children, in order"""
    new = {0: 0}
    nxt = [1]

    def visit(p):
        for c in child_lists[p]:
            new[c] = nxt[0]
            nxt[0] += 1
        for c in child_lists[p]:
            if child_lists[c]:
                visit(c)
    visit(0)
    return new


def train(desc, doc_offsets, k, L, weighting=0, scoring=0, seed=0, rand_mask=0x7fffffff, max_iter=0):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    off = np.asarray(doc_offsets, np.int64)
    t = _Trainer(desc, k, L, seed, rand_mask, max_iter)
    n = len(t.parent)
    cc = np.array([len(c) for c in t.children], np.int32)
    cs = np.concatenate([[0], np.cumsum(cc)[:-1]]).astype(np.int32)
    ci = np.array([c for ch in t.children for c in ch], np.int32)
    word_id = np.zeros(n, np.int32)
    leaves = [i for i in range(1, n) if cc[i] == 0]  # createWords: leaves in node-id order
    word_id[leaves] = np.arange(len(leaves))
    voc = dict(k=k, L=L, scoring=scoring, weighting=weighting, norm=2 if scoring == 1 else 0 if scoring == 5 else 1,
               n_words=len(leaves), child_start=cs, child_count=cc, child_ids=ci, desc=np.stack(t.node_desc),
               weight=np.zeros(n, np.float64), word_id=word_id)
    word_of = transform_words(voc, desc)
    if weighting in (1, 3):  # TF, BINARY
        voc["weight"][leaves] = 1.0
    else:  # setNodeWeights (:520-571)
        n_docs = len(off) - 1
        ni = np.zeros(len(leaves), np.int64)
        for d in range(n_docs):
            ni[np.unique(word_of[off[d]:off[d + 1]])] += 1
        for w, nid in enumerate(leaves):
            if ni[w] > 0:
                voc["weight"][nid] = math.log(float(n_docs) / float(ni[w]))
    st = dict(t.st)
    st.update(nodes=n, words=len(leaves), deepest_level=max(t.level))
    voc.update(stats=st, word_of=word_of, dist_sums=t.dist_sums, level=np.array(t.level, np.int32))
    return voc


TABLE_KEYS = ("child_start", "child_count", "child_ids", "desc", "word_id")
COUNTER_KEYS = ("nodes", "words", "deepest_level", "max_passes", "total_passes", "hit_max_iter", "early_stops", "draws",
                "redraws", "small_nodes", "single_leaves", "empty_groups")


def assert_same(got, want, what=""):
    """tables, word ids, weights (as uint64) and counters of a trained vocabulary equal the yardstick's"""
    for key in ("k", "L", "scoring", "weighting", "n_words"):
        assert int(got[key]) == int(want[key]), "%s: %s %r != %r" % (what, key, got[key], want[key])
    for key in TABLE_KEYS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs" % (what, key)
    wa = np.ascontiguousarray(got["weight"], np.float64).view(np.uint64)
    wb = np.ascontiguousarray(want["weight"], np.float64).view(np.uint64)
    assert np.array_equal(wa, wb), "%s: weights differ in %d nodes" % (what, int((wa != wb).sum()))
    for key in COUNTER_KEYS:
        assert int(got["stats"][key]) == int(want["stats"][key]), \
            "%s: counter %s %r != %r" % (what, key, got["stats"][key], want["stats"][key])
