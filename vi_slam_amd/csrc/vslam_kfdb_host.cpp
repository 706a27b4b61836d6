/* vslam_kfdb_host.cpp -- see include/vslam_fe.h: the host halves of ComputeBoW and of the KeyFrameDatabase queries. */
#include "../../include/vslam_fe.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

/* ------------------------------------------------------------------ ComputeBoW, host half
 * DBoW3::Vocabulary::transform (Vocabulary.cpp:754-826) after the per-feature tree walk: BowVector::addWeight /
 * addIfNotExist in feature order (std::map, double), the "divide by the number of words" step when the scoring
 * object does not normalise, BowVector::normalize (BowVector.cpp), FeatureVector::addFeature. */
extern "C" int vslam_bow_assemble(int weighting, int norm, const int32_t* word_id, const double* weight,
                                  const int32_t* node_id, int n, int32_t* bow_ids, double* bow_vals, int* n_bow,
                                  int32_t* fv_nodes, int32_t* fv_off, int32_t* fv_feat, int* n_fv) {
    if (n < 0 || (n && (!word_id || !weight || !node_id || !bow_ids || !bow_vals || !fv_nodes || !fv_off || !fv_feat)) ||
        !n_bow || !n_fv || weighting < 0 || weighting > 3 || norm < 0 || norm > 2)
        return -1;
    /* std::map semantics without the tree: a STABLE sort of the kept feature indices by word id (by node id) keeps
     * the feature order inside each key, so every word's weights are summed in exactly the order addWeight saw them */
    std::vector<int32_t> kept;
    kept.reserve(n);
    for (int i = 0; i < n; i++)
        if (weight[i] > 0) kept.push_back(i); /* not stopped */
    const bool tf = weighting == 0 || weighting == 1; /* TF_IDF, TF */
    std::vector<int32_t> byWord(kept);
    std::stable_sort(byWord.begin(), byWord.end(), [&](int32_t a, int32_t b) { return word_id[a] < word_id[b]; });
    int k = 0;
    for (size_t p = 0; p < byWord.size();) {
        const int32_t w = word_id[byWord[p]];
        double v = 0.0;
        bool first = true;
        size_t q = p;
        for (; q < byWord.size() && word_id[byWord[q]] == w; q++) {
            if (tf) v = first ? weight[byWord[q]] : v + weight[byWord[q]]; /* insert, then += */
            else if (first) v = weight[byWord[q]];                       /* addIfNotExist */
            first = false;
        }
        bow_ids[k] = w;
        bow_vals[k++] = v;
        p = q;
    }
    if (tf && k > 0 && norm == 0) {
        const double nd = (double)k;
        for (int i = 0; i < k; i++) bow_vals[i] /= nd;
    }
    if (norm) {
        double nv = 0.0;
        if (norm == 1) for (int i = 0; i < k; i++) nv += std::fabs(bow_vals[i]);
        else {
            for (int i = 0; i < k; i++) nv += bow_vals[i] * bow_vals[i];
            nv = std::sqrt(nv);
        }
        if (nv > 0.0) for (int i = 0; i < k; i++) bow_vals[i] /= nv;
    }
    *n_bow = k;
    std::vector<int32_t> byNode(kept);
    std::stable_sort(byNode.begin(), byNode.end(), [&](int32_t a, int32_t b) { return node_id[a] < node_id[b]; });
    int f = 0, off = 0;
    for (size_t p = 0; p < byNode.size();) {
        const int32_t nd = node_id[byNode[p]];
        fv_nodes[f] = nd;
        fv_off[f++] = off;
        for (; p < byNode.size() && node_id[byNode[p]] == nd; p++) fv_feat[off++] = byNode[p];
    }
    fv_off[f] = off;
    *n_fv = f;
    return 0;
}

/* ------------------------------------------------------------------ KeyFrameDatabase, selection stage
 * DetectRelocalizationCandidates (keyframedatabase.cpp:707-811) and DetectNBestCandidates (:579-705) from the hit list
 * on: the hits are lKFsSharingWords in the reference's order (vslam_kfdb_query_wait), words / si what the walk and
 * mpVoc->score leave in the KeyFrames, score_io the mRelocScore / mPlaceRecognitionScore members (read stale for
 * hits that are not scored by this query, written for those that are). */

namespace {
struct KfdbScored {
    float score;
    int hit;
};

/* :732-789 (:615-675): maxCommonWords, minCommonWords, the scores, the covisibility accumulation.  `listed[i]` == 0:
 * hit i never entered lKFsSharingWords (a connected keyframe, :600).  Returns lAccScoreAndMatch and bestAccScore. */
std::vector<KfdbScored> kfdb_accumulate(const int64_t* hit_kf, const int32_t* hit_words, const float* hit_si, int n_hits,
                                        const uint8_t* listed, float* score_io, vslam_kfdb_neighbours_fn neighbours_fn,
                                        void* user, float* bestAccScore) {
    std::vector<KfdbScored> acc;
    *bestAccScore = 0;
    int maxCommonWords = 0;
    for (int i = 0; i < n_hits; i++)
        if (listed[i] && hit_words[i] > maxCommonWords) maxCommonWords = hit_words[i];
    const int minCommonWords = (int)(maxCommonWords * 0.8f);
    std::vector<KfdbScored> scored; /* lScoreAndMatch */
    for (int i = 0; i < n_hits; i++)
        if (listed[i] && hit_words[i] > minCommonWords) {
            score_io[i] = hit_si[i];
            scored.push_back({hit_si[i], i});
        }
    if (scored.empty()) return acc;
    std::unordered_map<int64_t, int> byId; /* mn*Query == this query's id */
    for (int i = 0; i < n_hits; i++)
        if (listed[i]) byId.emplace(hit_kf[i], i);
    for (const KfdbScored& sc : scored) {
        int64_t neigh[10];
        int nn = neighbours_fn ? neighbours_fn(user, hit_kf[sc.hit], neigh) : 0;
        if (nn > 10) nn = 10;
        float bestScore = sc.score, accScore = bestScore;
        int best = sc.hit;
        for (int k = 0; k < nn; k++) {
            auto it = byId.find(neigh[k]);
            if (it == byId.end()) continue;
            const float s2 = score_io[it->second];
            accScore += s2;
            if (s2 > bestScore) {
                best = it->second;
                bestScore = s2;
            }
        }
        acc.push_back({accScore, best});
        if (accScore > *bestAccScore) *bestAccScore = accScore;
    }
    return acc;
}

bool kfdb_hits_ok(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words, const float* hit_si, int n_hits,
                  const float* score_io) {
    return n_hits >= 0 && (n_hits == 0 || (hit_kf && hit_map && hit_words && hit_si && score_io));
}
} /* namespace */

extern "C" int vslam_kfdb_select_relocalization(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words,
                                                const float* hit_si, int n_hits, float* score_io, int32_t map_id,
                                                vslam_kfdb_neighbours_fn neighbours_fn, void* user, int64_t* out_kf,
                                                int cap, int* n_out) {
    if (!kfdb_hits_ok(hit_kf, hit_map, hit_words, hit_si, n_hits, score_io) || !n_out || cap < 0 || (cap && !out_kf))
        return -1;
    *n_out = 0;
    if (n_hits == 0) return 0; /* :729 */
    const std::vector<uint8_t> listed((size_t)n_hits, 1);
    float bestAccScore;
    const std::vector<KfdbScored> acc =
        kfdb_accumulate(hit_kf, hit_words, hit_si, n_hits, listed.data(), score_io, neighbours_fn, user, &bestAccScore);
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::unordered_set<int> added; /* spAlreadyAddedKF */
    std::vector<int64_t> out;
    for (const KfdbScored& a : acc)
        if (a.score > minScoreToRetain) {
            if (hit_map[a.hit] != map_id) continue;
            if (added.insert(a.hit).second) out.push_back(hit_kf[a.hit]);
        }
    *n_out = (int)out.size();
    if ((int)out.size() > cap) return -4; /* VSLAM_ERR_CAPACITY; *n_out says how many there are */
    for (size_t i = 0; i < out.size(); i++) out_kf[i] = out[i];
    return 0;
}

extern "C" int vslam_kfdb_select_nbest(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words,
                                       const float* hit_si, int n_hits, float* score_io, int32_t query_map_id,
                                       const int64_t* connected_ids, int n_connected, int n_candidates,
                                       const int32_t* bad_maps, int n_bad_maps, vslam_kfdb_neighbours_fn neighbours_fn,
                                       void* user, int64_t* loop_kf, int* n_loop, int64_t* merge_kf, int* n_merge) {
    if (!kfdb_hits_ok(hit_kf, hit_map, hit_words, hit_si, n_hits, score_io) || n_connected < 0 ||
        (n_connected && !connected_ids) || n_bad_maps < 0 || (n_bad_maps && !bad_maps) || n_candidates < 0 || !n_loop ||
        !n_merge || (n_candidates && (!loop_kf || !merge_kf)))
        return -1;
    *n_loop = *n_merge = 0;
    const std::unordered_set<int64_t> connected(connected_ids, connected_ids + n_connected); /* spConnectedKF */
    std::vector<uint8_t> listed((size_t)n_hits);
    bool any = false;
    for (int i = 0; i < n_hits; i++) any |= (listed[i] = !connected.count(hit_kf[i])) != 0; /* :600 */
    if (!any) return 0; /* :612 */
    float bestAccScore;
    std::vector<KfdbScored> acc =
        kfdb_accumulate(hit_kf, hit_words, hit_si, n_hits, listed.data(), score_io, neighbours_fn, user, &bestAccScore);
    /* list::sort(compFirst) is a stable merge sort, descending */
    std::stable_sort(acc.begin(), acc.end(), [](const KfdbScored& a, const KfdbScored& b) { return a.score > b.score; });
    std::unordered_set<int> added; /* spAlreadyAddedKF */
    for (size_t i = 0; i < acc.size() && (*n_loop < n_candidates || *n_merge < n_candidates); i++) { /* :684-704 */
        const int h = acc[i].hit;
        if (added.count(h)) continue;
        const int32_t map = hit_map[h];
        if (query_map_id == map && *n_loop < n_candidates) loop_kf[(*n_loop)++] = hit_kf[h];
        else if (query_map_id != map && *n_merge < n_candidates &&
                 std::find(bad_maps, bad_maps + n_bad_maps, map) == bad_maps + n_bad_maps)
            merge_kf[(*n_merge)++] = hit_kf[h];
        added.insert(h);
    }
    return 0;
}
