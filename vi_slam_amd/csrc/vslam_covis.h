/* vslam_covis.h -- private: the host shadow of the observation graph (vslam_covis_host.cpp), shared by the device
 * mirror (vslam_covis.hip) and the GPU-free twin in libvslam_host.so.  Plain C++: nothing of HIP.
 *
 * Three word arrays are kept in the layout the kernels read, so that an upload is a copy of ranges:
 *   ktab   4 words per keyframe slot   { rank by order_key among the live slots, map, flags, 0 }
 *   korder 1 word per rank             { slot }
 *   ptab   4 words per point slot      { first record in the pool, records, nObs, flags }
 *   pool   2 words per record          { keyframe slot, level as KeyFrameCulling reads it (min of the sides present) }
 * A point's records lie in one segment of the pool whose capacity is a power of two (4 at first); the order inside a
 * segment carries no meaning (erase moves the last record into the hole).  What only the host needs -- the indices, the
 * level of each side, the stereo flag -- lies beside the pool in `extra`. */
#ifndef VSLAM_COVIS_H
#define VSLAM_COVIS_H
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vslam_fe.h"

#define COVIS_ALIVE 1
#define COVIS_BAD 2
#define COVIS_CHUNK_WORDS 64   /* the grain of dirty tracking: 256 bytes */
#define COVIS_FIRST_SEGMENT 4  /* records */
#define COVIS_DEFAULT_ENTRIES 4096
#define COVIS_LDS_SLOTS 8192   /* live keyframes up to which the kernels keep the histogram in LDS (32 KB) */
#define COVIS_TH_WEIGHT 15     /* keyframe.cpp:392 */

struct CovisRange {
    uint32_t off, n; /* words */
};

/* a word array with a dirty bit per chunk */
struct CovisArray {
    std::vector<int32_t> w;
    std::vector<uint8_t> dirty;
    std::vector<uint32_t> dirty_list;
    bool all = true; /* everything below `w.size()` goes up: after growth and compaction */
    void touch(size_t word) {
        const size_t c = word / COVIS_CHUNK_WORDS;
        if (c >= dirty.size()) dirty.resize(c + 1, 0);
        if (!dirty[c]) {
            dirty[c] = 1;
            dirty_list.push_back((uint32_t)c);
        }
    }
    void touch(size_t word, size_t n) {
        for (size_t c = word / COVIS_CHUNK_WORDS; n && c <= (word + n - 1) / COVIS_CHUNK_WORDS; c++) touch(c * COVIS_CHUNK_WORDS);
    }
    /* the ranges to upload, of `used` words, merged and ascending; clears the marks */
    void take(size_t used, std::vector<CovisRange>& out);
};

struct CovisExtra { /* host-only half of a record */
    int32_t idxL, idxR;
    int8_t lvlL, lvlR, stereo, pad_;
};

struct CovisStore {
    /* keyframes */
    std::vector<int64_t> kf_id;
    std::vector<uint64_t> kf_key;
    std::vector<int32_t> kf_refs; /* records that name the slot */
    std::vector<int32_t> kf_free;
    std::unordered_map<int64_t, int32_t> kf_slot;
    std::unordered_map<uint64_t, int32_t> key_slot;
    std::vector<int32_t> ktab, korder;
    bool ranks_stale = true; /* a keyframe came or went: refresh_ranks recomputes rank and korder */
    bool k_upload = true;    /* the device copy of both tables is out of date: they go up whole */
    /* points */
    std::vector<int64_t> mp_id;
    std::vector<uint32_t> seg_cap;
    std::vector<int32_t> mp_free;
    std::unordered_map<int64_t, int32_t> mp_slot;
    CovisArray ptab, pool;
    std::vector<CovisExtra> extra;
    size_t cap = 0, used = 0, dead = 0, n_records = 0; /* pool records: allocated, handed out, in abandoned segments, live */
    unsigned long long n_grow = 0, n_compact = 0;
    mutable std::string err;

    explicit CovisStore(size_t initial_entries = 0);
    int add_keyframe(int64_t kf, int32_t map, uint64_t key);
    int add_keyframes(int n, const int64_t* kf, const int32_t* map, const uint64_t* key);
    int set_keyframe_bad(int64_t kf);
    int set_keyframe_map(int64_t kf, int32_t map);
    int erase_keyframe(int64_t kf);
    int add_point(int64_t mp);
    int add_observation(int64_t mp, int64_t kf, int32_t idx, int is_right, int level, int stereo);
    int erase_observation(int64_t mp, int64_t kf, int* became_bad);
    int clear_point(int64_t mp);
    int erase_point(int64_t mp);
    int clear_map(int32_t map);
    int clear();
    int get_point(int64_t mp, int cap_obs, int* n_obs, int* bad, vslam_covis_obs* obs, int* n_rec) const;
    void refresh_ranks(); /* before a query: ktab ranks and korder, if keyframes changed */
    int n_live_keyframes() const { return (int)kf_slot.size(); }

    /* the queries from the shadow (the host twins).  Lists of job j start at the sum of the earlier jobs' counts. */
    int connections(int n_jobs, const vslam_covis_job* jobs, vslam_covis_result* res, std::vector<int64_t>& counter_kf,
                    std::vector<int32_t>& counter_n, std::vector<int64_t>& ordered_kf, std::vector<int32_t>& ordered_w);
    int culling(int n_jobs, const vslam_covis_cull_job* jobs, int th_obs, vslam_covis_cull_result* res);

private:
    int fail(const char* what) {
        err = what;
        return VSLAM_ERR_INVALID;
    }
    void drop_segment(int32_t p);
    void drop_records(int32_t p);
    int reserve_record(int32_t p);
    void compact();
    void set_ptab(int32_t p, int word, int32_t v) {
        ptab.w[(size_t)p * 4 + word] = v;
        ptab.touch((size_t)p * 4 + word);
    }
};

int covis_jobs_ok(int n_jobs, const vslam_covis_job* jobs, std::string& err);
int covis_cull_jobs_ok(int n_jobs, const vslam_covis_cull_job* jobs, int th_obs, std::string& err);

#endif
