/* vslam_voc_train_host.cpp -- the GPU-free half of Vocabulary::create / save (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp):
 *   - the parameter checks, the renumbering into DBoW3's node order with createWords (:496-515) and setNodeWeights
 *     (:520-571), shared by vslam_voc_train (vslam_voc_train.hip) and the twin;
 *   - vslamh_voc_train, the host twin: HKmeansStep (:233-394) as the plain recursion it is in the reference, one core,
 *     with the draws of include/vslam_fe.h in place of rand().  It serves the CPU tests, the demo and the timing
 *     baseline; the product library does not call it;
 *   - vslam_voc_file_save: Vocabulary::toStream(out, false) (:1292-1366).
 * Part of libvslam_fe.so and of libvslam_host.so. */
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "vslam_voc_train.h"

namespace vslam_vt {

int check_params(const vslam_voc_train_params* p, const int64_t* doc_offsets, int n_docs, vslam_voc_train_params* eff,
                 int64_t* n_features) {
    if (!p || !doc_offsets || !eff || !n_features) return vslam_voc_file_fail(VSLAM_ERR_INVALID, "invalid arguments");
    if (p->k < 2 || p->k > kMaxK || p->L < 1 || p->L > 10 || p->weighting < 0 || p->weighting > 3 || p->scoring < 0 ||
        p->scoring > 5 || p->max_iter < 0)
        return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary training: k must be 2..64, L 1..10, weighting 0..3, scoring 0..5, max_iter >= 0");
    if (p->rand_mask == 0 || p->rand_mask > 0x7fffffffu)
        return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary training: rand_mask must be 1..0x7fffffff");
    if (n_docs < 1 || doc_offsets[0] != 0) return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary training: doc_offsets must start at 0");
    for (int d = 0; d < n_docs; d++)
        if (doc_offsets[d + 1] < doc_offsets[d]) return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary training: doc_offsets decrease");
    if (doc_offsets[n_docs] < 1 || doc_offsets[n_docs] > VSLAM_VOC_MAX_FEATURES)
        return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary training: 1..2^24 features");
    *eff = *p;
    if (eff->max_iter == 0) eff->max_iter = kDefaultMaxIter;
    *n_features = doc_offsets[n_docs];
    return VSLAM_OK;
}

namespace {
/* ids in the order of the HKmeansStep calls: a call numbers its children, then descends into each child that has
 * children of its own, in cluster order */
void number_children(const std::vector<TreeNode>& tree, int p, std::vector<int32_t>& newid, int32_t& next) {
    for (int c : tree[p].children) newid[c] = next++;
    for (int c : tree[p].children)
        if (!tree[c].children.empty()) number_children(tree, c, newid, next);
}
}  // namespace

vslam_voc_file* finish_tree(const vslam_voc_train_params& p, const std::vector<TreeNode>& tree, vslam_voc_train_stats* st) {
    const size_t n = tree.size();
    std::vector<int32_t> newid(n, 0);
    int32_t next = 1;
    number_children(tree, 0, newid, next);
    std::vector<int32_t> old_of(n, 0);
    for (size_t i = 0; i < n; i++) old_of[newid[i]] = (int32_t)i;
    vslam_voc_file* f = new vslam_voc_file();
    f->k = p.k, f->L = p.L, f->scoring = p.scoring, f->weighting = p.weighting, f->format = 0;
    f->child_start.assign(n, 0);
    f->child_count.assign(n, 0);
    f->word_id.assign(n, 0);
    f->weight.assign(n, 0.0);
    f->desc.assign(n * 32, 0);
    f->child_ids.reserve(n - 1);
    int deepest = 0;
    for (size_t i = 0; i < n; i++) {
        const TreeNode& t = tree[old_of[i]];
        f->child_start[i] = (int32_t)f->child_ids.size();
        f->child_count[i] = (int32_t)t.children.size();
        for (int c : t.children) f->child_ids.push_back(newid[c]);
        memcpy(&f->desc[i * 32], t.desc, 32);
        deepest = std::max(deepest, t.level);
        if (i > 0 && t.children.empty()) f->word_id[i] = f->n_words++; /* createWords: leaves in node-id order */
    }
    if (st) st->nodes = (int32_t)n, st->words = f->n_words, st->deepest_level = deepest;
    return f;
}

void set_weights(vslam_voc_file& f, const int32_t* word_of_feature, const int64_t* doc_offsets, int n_docs) {
    const size_t n = f.child_start.size();
    std::vector<int32_t> node_of_word(f.n_words, 0);
    for (size_t i = 1; i < n; i++)
        if (f.child_count[i] == 0) node_of_word[f.word_id[i]] = (int32_t)i;
    if (f.weighting == 1 || f.weighting == 3) { /* TF, BINARY */
        for (int32_t nid : node_of_word) f.weight[nid] = 1.0;
        return;
    }
    std::vector<uint32_t> Ni(f.n_words, 0);
    std::vector<int32_t> counted(f.n_words, -1); /* last document that counted the word */
    for (int d = 0; d < n_docs; d++)
        for (int64_t i = doc_offsets[d]; i < doc_offsets[d + 1]; i++) {
            const int32_t w = word_of_feature[i];
            if (counted[w] != d) {
                counted[w] = d;
                Ni[w]++;
            }
        }
    for (int w = 0; w < f.n_words; w++)
        if (Ni[w] > 0) f.weight[node_of_word[w]] = log((double)(unsigned)n_docs / (double)Ni[w]);
}

}  // namespace vslam_vt

namespace {
using namespace vslam_vt;
typedef std::array<uint32_t, 8> Desc;

struct Twin {
    vslam_voc_train_params p;
    std::vector<Desc> feat;
    std::vector<TreeNode> tree;
    vslam_voc_train_stats st;

    /* initiateClustersKMpp (:409-491) */
    void seed(const std::vector<int>& idx, uint64_t key, std::vector<Desc>& clusters) {
        const size_t n = idx.size();
        uint32_t j = 0, redraws = 0;
        std::vector<uint32_t> min_d(n);
        clusters.push_back(feat[idx[vslamvoc_draw(key, j++, p.rand_mask) % n]]);
        for (size_t i = 0; i < n; i++) min_d[i] = hamming(feat[idx[i]].data(), clusters.back().data());
        while ((int)clusters.size() < p.k) {
            uint64_t sum = 0;
            for (size_t i = 0; i < n; i++) {
                if (min_d[i] > 0) {
                    const uint32_t d = hamming(feat[idx[i]].data(), clusters.back().data());
                    if (d < min_d[i]) min_d[i] = d;
                }
                sum += min_d[i];
            }
            if (sum == 0) {
                st.early_stops++;
                break;
            }
            const double cut_d = next_cut(key, &j, p.rand_mask, sum, &redraws);
            size_t pick = n - 1;
            uint64_t up = 0;
            for (size_t i = 0; i < n; i++) {
                up += min_d[i];
                if ((double)up >= cut_d) {
                    pick = i;
                    break;
                }
            }
            clusters.push_back(feat[idx[pick]]);
        }
        st.draws += j;
        st.redraws += redraws;
    }

    /* HKmeansStep (:233-394); idx ascending */
    void step(int parent, const std::vector<int>& idx, int level, uint64_t key) {
        const size_t n = idx.size();
        if (n == 0) return;
        std::vector<Desc> clusters;
        std::vector<int> assoc(n, 0);
        if ((int)n <= p.k) {
            st.small_nodes++;
            for (size_t i = 0; i < n; i++) clusters.push_back(feat[idx[i]]), assoc[i] = (int)i;
        } else {
            seed(idx, key, clusters);
            const int nc = (int)clusters.size();
            std::vector<int> last;
            std::vector<uint32_t> cnt(256);
            int passes = 0;
            for (;;) {
                if (passes > 0)
                    for (int c = 0; c < nc; c++) { /* DescManip::meanValue */
                        uint32_t size = 0;
                        std::fill(cnt.begin(), cnt.end(), 0u);
                        for (size_t i = 0; i < n; i++)
                            if (assoc[i] == c) {
                                size++;
                                for (int b = 0; b < 256; b++) cnt[b] += (feat[idx[i]][b >> 5] >> (b & 31)) & 1u;
                            }
                        if (size == 0) {
                            st.empty_groups++;
                            continue;
                        }
                        const uint32_t th = majority_threshold(size);
                        for (int w = 0; w < 8; w++) {
                            uint32_t v = 0;
                            for (int q = 0; q < 32; q++) v |= (uint32_t)(cnt[w * 32 + q] >= th) << q;
                            clusters[c][w] = v;
                        }
                    }
                for (size_t i = 0; i < n; i++) {
                    uint32_t best = hamming(feat[idx[i]].data(), clusters[0].data());
                    int ic = 0;
                    for (int c = 1; c < nc; c++) {
                        const uint32_t d = hamming(feat[idx[i]].data(), clusters[c].data());
                        if (d < best) best = d, ic = c;
                    }
                    assoc[i] = ic;
                }
                passes++;
                if (passes > 1 && assoc == last) break;
                if (passes >= p.max_iter) {
                    st.hit_max_iter++;
                    break;
                }
                last = assoc;
            }
            st.total_passes += passes;
            st.max_passes = std::max(st.max_passes, passes);
        }
        const int nc = (int)clusters.size();
        std::vector<int> ids(nc);
        for (int c = 0; c < nc; c++) {
            TreeNode t;
            t.parent = parent, t.level = level;
            memcpy(t.desc, clusters[c].data(), 32);
            ids[c] = (int)tree.size();
            tree[parent].children.push_back(ids[c]);
            tree.push_back(t);
        }
        if (level >= p.L) return;
        for (int c = 0; c < nc; c++) {
            std::vector<int> sub;
            for (size_t i = 0; i < n; i++)
                if (assoc[i] == c) sub.push_back(idx[i]);
            if (sub.size() > 1)
                step(ids[c], sub, level + 1, vslamvoc_child_key(key, c));
            else if (sub.size() == 1)
                st.single_leaves++;
        }
    }

    /* Vocabulary::transform(feature, word_id) (:880-...): strict <, first child wins */
    int32_t word_of(const vslam_voc_file& f, const Desc& d) const {
        int32_t id = 0;
        while (f.child_count[id] > 0) {
            const int32_t* ch = &f.child_ids[f.child_start[id]];
            uint32_t best = 0xffffffffu;
            int32_t bid = ch[0];
            for (int j = 0; j < f.child_count[id]; j++) {
                uint32_t nd[8];
                memcpy(nd, &f.desc[(size_t)ch[j] * 32], 32);
                const uint32_t dist = hamming(d.data(), nd);
                if (dist < best) best = dist, bid = ch[j];
            }
            id = bid;
        }
        return f.word_id[id];
    }
};

}  // namespace

extern "C" int vslamh_voc_train(const vslam_voc_train_params* params, const uint8_t* desc, const int64_t* doc_offsets,
                                int n_docs, vslam_voc_file** out, vslam_voc_train_stats* stats) {
    if (!out || !desc) return vslam_voc_file_fail(VSLAM_ERR_INVALID, "invalid arguments");
    *out = nullptr;
    Twin t;
    int64_t n = 0;
    const int rc = check_params(params, doc_offsets, n_docs, &t.p, &n);
    if (rc != VSLAM_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    memset(&t.st, 0, sizeof(t.st));
    t.feat.resize((size_t)n);
    memcpy(t.feat.data(), desc, (size_t)n * 32);
    t.tree.emplace_back();
    std::vector<int> all((size_t)n);
    std::iota(all.begin(), all.end(), 0);
    t.step(0, all, 1, vslamvoc_mix(t.p.seed));
    vslam_voc_file* f = finish_tree(t.p, t.tree, &t.st);
    if (t.p.weighting == 0 || t.p.weighting == 2) {
        std::vector<int32_t> word((size_t)n);
        for (int64_t i = 0; i < n; i++) word[i] = t.word_of(*f, t.feat[i]);
        set_weights(*f, word.data(), doc_offsets, n_docs);
    } else {
        set_weights(*f, nullptr, doc_offsets, n_docs);
    }
    t.st.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = t.st;
    *out = f;
    return VSLAM_OK;
}

extern "C" int vslam_voc_file_from_arrays(int branching, int depth_levels, int scoring, int weighting, int n_nodes,
                                          const int32_t* child_start, const int32_t* child_count, const int32_t* child_ids,
                                          int n_child_ids, const uint8_t* node_desc, const double* node_weight,
                                          const int32_t* node_word_id, vslam_voc_file** out) {
    if (!out || n_nodes < 2 || n_child_ids < 0 || !child_start || !child_count || !child_ids || !node_desc || !node_weight ||
        !node_word_id || depth_levels < 1 || weighting < 0 || weighting > 3 || scoring < 0 || scoring > 5)
        return vslam_voc_file_fail(VSLAM_ERR_INVALID, "invalid arguments");
    *out = nullptr;
    int n_words = 0;
    for (int i = 0; i < n_nodes; i++) {
        if (child_count[i] < 0 || child_start[i] < 0 || (long long)child_start[i] + child_count[i] > n_child_ids)
            return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary: child range out of bounds");
        for (int j = 0; j < child_count[i]; j++) {
            const int c = child_ids[child_start[i] + j];
            if (c <= i || c >= n_nodes)
                return vslam_voc_file_fail(VSLAM_ERR_INVALID, "vocabulary: child ids must be larger than their parent's and inside the node table");
        }
        if (i > 0 && child_count[i] == 0) n_words++;
    }
    vslam_voc_file* f = new vslam_voc_file();
    f->k = branching, f->L = depth_levels, f->scoring = scoring, f->weighting = weighting, f->format = 0, f->n_words = n_words;
    f->child_start.assign(child_start, child_start + n_nodes);
    f->child_count.assign(child_count, child_count + n_nodes);
    f->child_ids.assign(child_ids, child_ids + n_child_ids);
    f->desc.assign(node_desc, node_desc + (size_t)n_nodes * 32);
    f->weight.assign(node_weight, node_weight + n_nodes);
    f->word_id.assign(node_word_id, node_word_id + n_nodes);
    *out = f;
    return VSLAM_OK;
}

extern "C" int vslam_voc_file_save(const vslam_voc_file* v, const char* path) {
    if (!v || !path || v->child_start.empty()) return vslam_voc_file_fail(VSLAM_ERR_INVALID, "invalid arguments");
    std::vector<uint8_t> out;
    auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    auto put32 = [&](uint32_t x) { put(&x, 4); };
    const uint64_t magic = 88877711233ull;
    const uint8_t compressed = 0;
    const size_t n = v->child_start.size();
    put(&magic, 8);
    put(&compressed, 1);
    put32((uint32_t)n);
    put32((uint32_t)v->k), put32((uint32_t)v->L), put32((uint32_t)v->scoring), put32((uint32_t)v->weighting);
    std::vector<int32_t> stack(1, 0); /* toStream's walk: the children of the last pushed inner node first */
    while (!stack.empty()) {
        const int32_t pid = stack.back();
        stack.pop_back();
        for (int j = 0; j < v->child_count[pid]; j++) {
            const int32_t c = v->child_ids[v->child_start[pid] + j];
            put32((uint32_t)c), put32((uint32_t)pid);
            put(&v->weight[c], 8);
            put32(32), put32(1), put32(0); /* DescManip::toStream: cols, rows, type CV_8U */
            put(&v->desc[(size_t)c * 32], 32);
            if (v->child_count[c] > 0) stack.push_back(c);
        }
    }
    std::vector<int32_t> leaves;
    for (size_t i = 1; i < n; i++)
        if (v->child_count[i] == 0) leaves.push_back((int32_t)i);
    std::stable_sort(leaves.begin(), leaves.end(), [&](int32_t a, int32_t b) { return v->word_id[a] < v->word_id[b]; });
    put32((uint32_t)leaves.size());
    for (size_t w = 0; w < leaves.size(); w++) put32((uint32_t)w), put32((uint32_t)leaves[w]);
    FILE* fp = fopen(path, "wb");
    if (!fp) return vslam_voc_file_fail(VSLAM_ERR_INVALID, std::string("vocabulary file: cannot write ") + path);
    const bool ok = fwrite(out.data(), 1, out.size(), fp) == out.size();
    if (fclose(fp) != 0 || !ok) return vslam_voc_file_fail(VSLAM_ERR_INVALID, std::string("vocabulary file: short write to ") + path);
    return VSLAM_OK;
}
