/* vslam_ftbook.cpp -- vilib::FeatureTrackerGPU's bookkeeping (include/vslam_featuretracker.h): steps 02 and 03 of track() and
 * what they call, around the two kernels of vslam_featuretracker.hip.  feature_tracker_gpu.cpp:137-267,319-352,404-411,496-524;
 * feature_tracker_base.cpp:61-171. */
#include "../../include/vslam_featuretracker.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

struct vslam_ftbook {
    vslam_ft_params p;
    int n_cols = 0, n_rows = 0, cw = 0, ch = 0, cells = 0, max_ftr = 0;
    int next_id = 0, tracked = 0, detected = 0;
    struct Track {
        vslam_ft_track_info i;
        int first_level;
        float first_score;
    };
    std::vector<Track> tracks;
    std::vector<int> avail; /* available_indices_: decreasing, taken from the back */
    std::vector<vslam_ft_feature> feats;
    void add_feature(const Track& t) { feats.push_back(vslam_ft_feature{t.i.cur_pos[0], t.i.cur_pos[1], t.first_score, t.first_level, t.i.track_id}); }
};

extern "C" int vslam_ftbook_create(const vslam_ft_params* p, int n_cols, int n_rows, int cell_w, int cell_h, vslam_ftbook** out) {
    if (!p || !out || n_cols < 1 || n_rows < 1 || cell_w < 1 || cell_h < 1 || p->use_best_n_features < -1 ||
        p->min_tracks_to_detect_new_features < 0)
        return -1;
    *out = nullptr;
    const long long cells = (long long)n_cols * n_rows;
    /* feature_tracker_gpu.cpp:404-411 */
    const long long max_ftr = ((long long)p->min_tracks_to_detect_new_features - 1) + ((p->use_best_n_features == -1 ? cells : p->use_best_n_features) - 1);
    if (max_ftr < 1 || max_ftr > (1 << 20)) return -1;
    vslam_ftbook* b = new vslam_ftbook();
    b->p = *p;
    b->n_cols = n_cols;
    b->n_rows = n_rows;
    b->cw = cell_w;
    b->ch = cell_h;
    b->cells = (int)cells;
    b->max_ftr = (int)max_ftr;
    for (int i = 0; i < b->max_ftr; i++) b->avail.push_back(b->max_ftr - i - 1); /* initBufferIds */
    *out = b;
    return 0;
}

extern "C" void vslam_ftbook_destroy(vslam_ftbook* b) { delete b; }
extern "C" int vslam_ftbook_capacity(const vslam_ftbook* b) { return b ? b->max_ftr : -1; }

extern "C" int vslam_ftbook_results(vslam_ftbook* b, const float* res, int n) {
    if (!b || n != (int)b->tracks.size() || (n && !res)) return -1;
    b->feats.clear();
    b->tracked = 0;
    std::vector<vslam_ftbook::Track> keep; /* removeTracks: the survivors in their order */
    keep.reserve(b->tracks.size());
    for (int i = 0; i < n; i++) {
        vslam_ftbook::Track& t = b->tracks[i];
        const float x = res[4 * i];
        if (std::isnan(x)) {
            b->avail.push_back(t.i.buffer_id);
            continue;
        }
        t.i.life++;
        t.i.cur_pos[0] = x;
        t.i.cur_pos[1] = res[4 * i + 1];
        t.i.cur_disparity = res[4 * i + 2];
        b->tracked++;
        b->add_feature(t);
        keep.push_back(t);
    }
    b->tracks.swap(keep);
    b->detected = 0;
    return 0;
}

extern "C" int vslam_ftbook_need_detect(const vslam_ftbook* b) { return b ? (b->tracked < b->p.min_tracks_to_detect_new_features ? 1 : 0) : -1; }

extern "C" int vslam_ftbook_detect(vslam_ftbook* b, const float* pos, const float* score, const int32_t* level, int* n_detected) {
    if (!b || !pos || !score || !level) return -1;
    b->detected = 0;
    std::vector<uint8_t> occ((size_t)b->cells, 0); /* OccupancyGrid2D::reset */
    if (b->p.reset_before_detection) {
        b->tracked = 0;
        for (const vslam_ftbook::Track& t : b->tracks) b->avail.push_back(t.i.buffer_id);
        b->tracks.clear();
        b->feats.clear();
    } else {
        for (const vslam_ft_feature& f : b->feats) { /* setOccupied(int x, int y): the position truncated */
            const double fx = (double)f.x, fy = (double)f.y;
            if (!(fx > -1.0 && fy > -1.0 && fx < (double)b->n_cols * b->cw && fy < (double)b->n_rows * b->ch)) continue; /* the reference asserts */
            const int x = (int)fx, y = (int)fy;
            occ[(size_t)(y / b->ch) * b->n_cols + x / b->cw] = 1;
        }
    }
    std::vector<int> order((size_t)b->cells);
    for (int i = 0; i < b->cells; i++) order[i] = i;
    int limit = b->cells;
    if (b->p.use_best_n_features != -1) { /* :242-247; the reference's std::sort leaves ties open: the lower cell first */
        std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return score[a] > score[c]; });
        limit = std::max(0, b->p.use_best_n_features - b->tracked);
    }
    for (int k = 0; k < b->cells && b->detected < limit && !b->avail.empty(); k++) {
        const int c = order[k];
        if (occ[c] || !(score[c] > 0.0f)) continue;
        vslam_ftbook::Track t;
        memset(&t, 0, sizeof(t));
        t.i.first_pos[0] = t.i.cur_pos[0] = pos[2 * c];
        t.i.first_pos[1] = t.i.cur_pos[1] = pos[2 * c + 1];
        t.i.track_id = b->next_id++;
        t.i.buffer_id = b->avail.back();
        b->avail.pop_back();
        t.first_level = level[c];
        t.first_score = score[c];
        b->tracks.push_back(t);
        b->add_feature(t);
        b->detected++;
    }
    if (n_detected) *n_detected = b->detected;
    return 0;
}

extern "C" int vslam_ftbook_update_count(const vslam_ftbook* b) {
    return b ? (b->p.klt_template_is_first_observation ? b->detected : b->detected + b->tracked) : -1;
}

extern "C" int vslam_ftbook_features(const vslam_ftbook* b, vslam_ft_feature* out, int cap, int* n) {
    if (!b || cap < 0 || (cap && !out)) return -1;
    if (n) *n = (int)b->feats.size();
    for (int i = 0; i < cap && i < (int)b->feats.size(); i++) out[i] = b->feats[i];
    return 0;
}

extern "C" int vslam_ftbook_tracks(const vslam_ftbook* b, vslam_ft_track_info* out, int cap, int* n) {
    if (!b || cap < 0 || (cap && !out)) return -1;
    if (n) *n = (int)b->tracks.size();
    for (int i = 0; i < cap && i < (int)b->tracks.size(); i++) out[i] = b->tracks[i].i;
    return 0;
}

extern "C" int vslam_ftbook_disparity(const vslam_ftbook* b, double pivot_ratio, double* out) {
    if (!b || !out || !(pivot_ratio >= 0.0)) return -1;
    std::vector<float> d; /* tracks with life >= 1; new tracks sit at the end of the list */
    for (const vslam_ftbook::Track& t : b->tracks) {
        if (t.i.life <= 0) break;
        d.push_back(t.i.cur_disparity);
    }
    *out = 0.0;
    if (d.empty()) return 0;
    const size_t pivot = std::min((size_t)(pivot_ratio * (double)d.size()), d.size() - 1);
    std::nth_element(d.begin(), d.begin() + pivot, d.end());
    *out = (double)d[pivot];
    return 0;
}

extern "C" int vslam_ftbook_reset(vslam_ftbook* b) {
    if (!b) return -1;
    for (const vslam_ftbook::Track& t : b->tracks) b->avail.push_back(t.i.buffer_id);
    b->tracks.clear();
    b->tracked = b->detected = 0;
    return 0;
}

extern "C" int vslam_ftbook_set_best_n(vslam_ftbook* b, int n) {
    if (!b || n < -1) return -1;
    b->p.use_best_n_features = n;
    return 0;
}

extern "C" int vslam_ftbook_set_min_tracks(vslam_ftbook* b, int n) {
    if (!b || n < 0) return -1;
    b->p.min_tracks_to_detect_new_features = n;
    return 0;
}

/* Point::getNewId is one counter for every camera of a FrameBundle: a tracker over several books reads it from one book
 * after step 03 and hands it to the next before */
extern "C" int vslam_ftbook_next_id(const vslam_ftbook* b) { return b ? b->next_id : -1; }
extern "C" int vslam_ftbook_set_next_id(vslam_ftbook* b, int id) {
    if (!b || id < 0) return -1;
    b->next_id = id;
    return 0;
}
