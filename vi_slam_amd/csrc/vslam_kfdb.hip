/* vslam_kfdb.hip -- KeyFrameDatabase (src/datastructures/keyframedatabase.cpp) in HBM: the BowVectors of the keyframes
 * in one pooled pair of device arrays, and ONE kernel that does, for every (query, keyframe) pair at once, what the
 * reference's walk over its inverted file plus DBoW3's L1Scoring::score (thirdparty/DBoW3/DBoW3/src/ScoringObject.cpp:
 * 23-68) do: the number of common words (mnRelocWords / mnPlaceRecognitionWords), the smallest common word (it decides
 * where the keyframe enters lKFsSharingWords) and the score.
 *
 * The inverted file itself is not stored.  A keyframe's position in every inverted list of the reference is its
 * position in `add` order (list::push_back in add, order-preserving erase: keyframedatabase.cpp:21-80), so the slot
 * number stands for it: the reference meets the keyframes sharing words with a query in the order (smallest common
 * word, slot).  What follows the hit list -- exclusion of connected keyframes, minCommonWords, covisibility
 * accumulation, the candidate lists -- is order-dependent work on a few hundred items and lives on the host:
 * vslam_kfdb_select_* (vslam_kfdb_host.cpp).
 */
#include <unordered_map>

#include "vslam_ctx.h"
#include "vslam_kernels.h"

struct KfdbSlot { /* one keyframe, in add order; mirrored to the device as it is */
    uint32_t off; /* first entry in the pool */
    int32_t len;
    int32_t alive;
    int32_t map;
};

struct KfdbQueryArgs {
    const int32_t* poolIds;
    const double* poolVals;
    const KfdbSlot* slots;
    int32_t nSlots;
    const int32_t *qIds, *qOff; /* the queries' BowVectors back to back; qOff[nq + 1] */
    const double* qVals;
    double* score;  /* [nq][nSlots] */
    int32_t* words; /* [nq][nSlots]: 0 = not a hit */
    int32_t* first; /* [nq][nSlots]: smallest common word id */
};

#define KFDB_WAVES 4 /* pairs per workgroup */

/* One wave per (query, slot) pair.  The lanes take 64 consecutive query words per pass and look each up in the
 * keyframe's ascending ids (binary search); the terms of the matched lanes are then added ONE AFTER ANOTHER in lane
 * order -- ascending word id -- into one double, because that is what L1Scoring::score does (`score += ...` along both
 * maps) and a tree reduction of the same terms rounds differently in most pairs.  Each term is
 * (fabs(vi - wi) - fabs(vi)) - fabs(wi): no multiplication, nothing to contract. */
__global__ void __launch_bounds__(64 * KFDB_WAVES) k_kfdb_query(KfdbQueryArgs A) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6), q = blockIdx.y;
    if (s >= A.nSlots) return; /* whole wave */
    const KfdbSlot sl = A.slots[s];
    const int q0 = A.qOff[q], qn = A.qOff[q + 1] - q0;
    double acc = 0.0;
    int words = 0, first = -1;
    if (sl.alive && sl.len > 0) {
        const int32_t* kid = A.poolIds + sl.off;
        const double* kval = A.poolVals + sl.off;
        for (int base = 0; base < qn; base += 64) {
            const int j = base + lane;
            bool hit = false;
            double term = 0.0;
            int id = 0;
            if (j < qn) {
                id = A.qIds[q0 + j];
                int lo = 0, hi = sl.len; /* lower_bound */
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (kid[mid] < id) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < sl.len && kid[lo] == id) {
                    hit = true;
                    const double vi = A.qVals[q0 + j], wi = kval[lo];
                    term = (fabs(vi - wi) - fabs(vi)) - fabs(wi); /* ScoringObject.cpp:41 */
                }
            }
            unsigned long long m = __ballot(hit);
            if (m) {
                if (first < 0) first = __shfl(id, __ffsll((long long)m) - 1);
                words += __popcll(m);
                while (m) { /* wave-uniform: every lane keeps the same running sum */
                    acc += __shfl(term, __ffsll((long long)m) - 1);
                    m &= m - 1;
                }
            }
        }
    }
    if (lane == 0) {
        const size_t o = (size_t)q * A.nSlots + s;
        A.score[o] = -acc / 2.0; /* ScoringObject.cpp:65 */
        A.words[o] = words;
        A.first[o] = first;
    }
}

#define KFDB_DEFAULT_ENTRIES 4096
#define KFDB_MAX_ENTRIES ((size_t)1 << 31)

struct vslam_kfdb {
    int device = 0, nWords = 0;
    std::mutex mu;
    vslam_dbuf<int32_t> d_ids; /* the pool: cap entries each */
    vslam_dbuf<double> d_vals;
    size_t cap = 0, used = 0, dead = 0; /* pool entries: allocated, handed out, belonging to erased keyframes */
    std::vector<KfdbSlot> slots;
    std::vector<int64_t> kf; /* keyframe id of every slot */
    std::unordered_map<int64_t, int> live; /* keyframe id -> slot */
    vslam_dbuf<KfdbSlot> d_slots;
    bool table_dirty = true;
    unsigned long long n_grow = 0, n_compact = 0;
    /* the query in flight / delivered last: results lie in q_fe's pinned staging, the slot table as it was */
    vslam_event ev;
    vslam_fe* q_fe = nullptr;
    int q_n = 0;
    std::vector<KfdbSlot> q_slots;
    std::vector<int64_t> q_kf;
    size_t q_o_score = 0, q_o_words = 0, q_o_first = 0;
};

/* nothing of the pool or the slot table changes under a query kernel that may still read it */
static int kfdb_settle(vslam_kfdb* db) {
    if (db->q_fe) HIPCHK(hipEventSynchronize(db->ev));
    return VSLAM_OK;
}

/* move the pool's entries [from, from + n) to `to` of a new pair of arrays */
static int kfdb_move(const vslam_kfdb* db, int32_t* ids, double* vals, size_t to, size_t from, size_t n) {
    if (!n) return VSLAM_OK;
    HIPCHK(hipMemcpy(ids + to, db->d_ids + from, n * 4, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(vals + to, db->d_vals + from, n * 8, hipMemcpyDeviceToDevice));
    return VSLAM_OK;
}

static int kfdb_grow(vslam_kfdb* db, size_t need) {
    size_t cap = db->cap;
    while (cap < need) cap *= 2;
    if (cap > KFDB_MAX_ENTRIES) {
        g_err = "KeyFrameDatabase: more than 2^31 pool entries";
        return VSLAM_ERR_CAPACITY;
    }
    vslam_dbuf<int32_t> ids; /* built aside and swapped in on success; the old pair goes with these */
    vslam_dbuf<double> vals;
    int rc = ids.alloc(cap);
    if (!rc) rc = vals.alloc(cap);
    if (!rc) rc = kfdb_move(db, ids, vals, 0, 0, db->used);
    if (rc) return rc;
    db->d_ids.swap(ids);
    db->d_vals.swap(vals);
    db->cap = cap;
    db->n_grow++;
    return VSLAM_OK;
}

/* Drop the erased keyframes' entries and slots, keeping the order of the rest: runs of neighbouring live slots are
 * neighbours in the pool too and move as one copy. */
static int kfdb_compact(vslam_kfdb* db) {
    if (db->dead * 2 <= db->used) return VSLAM_OK;
    vslam_dbuf<int32_t> ids; /* as in kfdb_grow */
    vslam_dbuf<double> vals;
    int rc = ids.alloc(db->cap);
    if (!rc) rc = vals.alloc(db->cap);
    if (rc) return rc;
    std::vector<KfdbSlot> slots;
    std::vector<int64_t> kf;
    size_t to = 0, run_from = 0, run_n = 0;
    for (size_t s = 0; s < db->slots.size() && !rc; s++) {
        const KfdbSlot& sl = db->slots[s];
        if (!sl.alive) continue;
        if (run_n && run_from + run_n != sl.off) {
            rc = kfdb_move(db, ids, vals, to, run_from, run_n);
            to += run_n;
            run_n = 0;
        }
        if (!run_n) run_from = sl.off;
        KfdbSlot ns = sl;
        ns.off = (uint32_t)(to + run_n);
        run_n += (size_t)sl.len;
        slots.push_back(ns);
        kf.push_back(db->kf[s]);
    }
    if (!rc) rc = kfdb_move(db, ids, vals, to, run_from, run_n);
    if (rc) return rc;
    db->d_ids.swap(ids);
    db->d_vals.swap(vals);
    db->slots.swap(slots);
    db->kf.swap(kf);
    db->live.clear();
    for (size_t s = 0; s < db->slots.size(); s++) db->live[db->kf[s]] = (int)s;
    db->used -= db->dead;
    db->dead = 0;
    db->table_dirty = true;
    db->n_compact++;
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_create_ex(int device, int n_words, int scoring, int initial_entries, vslam_kfdb** out) {
    if (!out || n_words < 1 || initial_entries < 0) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    if (scoring != 0) {
        g_err = "KeyFrameDatabase: only L1_NORM scoring (0) is implemented";
        return VSLAM_ERR_UNSUPPORTED;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_err = "no usable HIP device (this library has no CPU fallback)";
        return VSLAM_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    vslam_kfdb* db = new vslam_kfdb();
    db->device = device;
    db->nWords = n_words;
    db->cap = initial_entries ? (size_t)initial_entries : KFDB_DEFAULT_ENTRIES;
    int rc = db->d_ids.alloc(db->cap);
    if (!rc) rc = db->d_vals.alloc(db->cap);
    if (!rc) rc = db->ev.ensure(hipEventDisableTiming);
    if (rc) {
        delete db;
        return rc;
    }
    *out = db;
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_create(int device, int n_words, int scoring, vslam_kfdb** out) {
    return vslam_kfdb_create_ex(device, n_words, scoring, 0, out);
}

extern "C" void vslam_kfdb_destroy(vslam_kfdb* db) {
    if (!db) return;
    hipSetDevice(db->device);
    if (db->q_fe) hipEventSynchronize(db->ev);
    delete db;
}

/* a BowVector as vslam_bow_assemble leaves it: strictly ascending ids inside the vocabulary */
static bool kfdb_bow_ok(const int32_t* ids, const double* vals, int n, int n_words) {
    if (n < 0 || (n && (!ids || !vals))) return false;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= n_words || (i && ids[i] <= ids[i - 1])) return false;
    return true;
}

extern "C" int vslam_kfdb_add(vslam_kfdb* db, int64_t kf_id, int32_t map_id, const int32_t* bow_ids,
                              const double* bow_vals, int n) {
    if (!db) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    if (!kfdb_bow_ok(bow_ids, bow_vals, n, db->nWords)) {
        g_err = "KeyFrameDatabase::add: word ids must be strictly ascending and inside the vocabulary";
        return VSLAM_ERR_INVALID;
    }
    if (db->live.count(kf_id)) {
        g_err = "KeyFrameDatabase::add: the keyframe is in the database already";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(db->device));
    int rc = kfdb_settle(db);
    if (rc) return rc;
    if (db->used + (size_t)n > db->cap && (rc = kfdb_grow(db, db->used + (size_t)n))) return rc;
    if (n) {
        HIPCHK(hipMemcpy(db->d_ids + db->used, bow_ids, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db->d_vals + db->used, bow_vals, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    KfdbSlot sl;
    sl.off = (uint32_t)db->used;
    sl.len = n;
    sl.alive = 1;
    sl.map = map_id;
    db->live[kf_id] = (int)db->slots.size();
    db->slots.push_back(sl);
    db->kf.push_back(kf_id);
    db->used += (size_t)n;
    db->table_dirty = true;
    return VSLAM_OK;
}

static void kfdb_kill(vslam_kfdb* db, int s) {
    db->slots[s].alive = 0;
    db->dead += (size_t)db->slots[s].len;
    db->live.erase(db->kf[s]);
    db->table_dirty = true;
}

extern "C" int vslam_kfdb_erase(vslam_kfdb* db, int64_t kf_id) {
    if (!db) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    auto it = db->live.find(kf_id);
    if (it == db->live.end()) return VSLAM_OK; /* the reference's erase finds nothing to remove either */
    HIPCHK(hipSetDevice(db->device));
    int rc = kfdb_settle(db);
    if (rc) return rc;
    kfdb_kill(db, it->second);
    return kfdb_compact(db);
}

extern "C" int vslam_kfdb_clear(vslam_kfdb* db) {
    if (!db) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    HIPCHK(hipSetDevice(db->device));
    int rc = kfdb_settle(db);
    if (rc) return rc;
    db->slots.clear();
    db->kf.clear();
    db->live.clear();
    db->used = db->dead = 0;
    db->table_dirty = true;
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_clear_map(vslam_kfdb* db, int32_t map_id) {
    if (!db) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    HIPCHK(hipSetDevice(db->device));
    int rc = kfdb_settle(db);
    if (rc) return rc;
    for (size_t s = 0; s < db->slots.size(); s++)
        if (db->slots[s].alive && db->slots[s].map == map_id) kfdb_kill(db, (int)s);
    return kfdb_compact(db);
}

extern "C" int vslam_kfdb_size(vslam_kfdb* db, int* n_keyframes, long long* n_entries) {
    if (!db) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(db->mu);
    if (n_keyframes) *n_keyframes = (int)db->live.size();
    if (n_entries) *n_entries = (long long)(db->used - db->dead);
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_stats(vslam_kfdb* db, long long* capacity, long long* used, int* n_slots, int* n_growths,
                                int* n_compactions) {
    if (!db) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(db->mu);
    if (capacity) *capacity = (long long)db->cap;
    if (used) *used = (long long)db->used;
    if (n_slots) *n_slots = (int)db->slots.size();
    if (n_growths) *n_growths = (int)db->n_grow;
    if (n_compactions) *n_compactions = (int)db->n_compact;
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_query_async(vslam_kfdb* db, vslam_fe* fe, int nq, const int32_t* const* bow_ids,
                                      const double* const* bow_vals, const int* n) {
    if (!db || !fe || nq < 1 || nq > 32 || !bow_ids || !bow_vals || !n || fe->p.device != db->device) {
        g_err = "invalid arguments (1..32 queries; the database must live on the context's device)";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    size_t total = 0;
    for (int q = 0; q < nq; q++) {
        if (!kfdb_bow_ok(bow_ids[q], bow_vals[q], n[q], db->nWords)) {
            g_err = "KeyFrameDatabase query: word ids must be strictly ascending and inside the vocabulary";
            return VSLAM_ERR_INVALID;
        }
        total += (size_t)n[q];
    }
    HIPCHK(hipSetDevice(db->device));
    int rc = kfdb_settle(db); /* the staging of a query that was never waited for is reused below */
    if (rc) return rc;
    db->q_fe = nullptr;
    const size_t S = db->slots.size();
    const auto [o_vals, o_ids, o_off, o_score, o_words, o_first, bytes] = vslam::layout(
        16, {total * 8, total * 4, (size_t)(nq + 1) * 4, (size_t)nq * S * 8, (size_t)nq * S * 4, (size_t)nq * S * 4});
    if ((rc = fe->kfdb.ensure(bytes))) return rc;
    uint8_t *h = fe->kfdb.h, *d = fe->kfdb.d;
    int32_t* off = (int32_t*)(h + o_off);
    size_t at = 0;
    for (int q = 0; q < nq; q++) {
        off[q] = (int32_t)at;
        if (n[q]) {
            memcpy((double*)(h + o_vals) + at, bow_vals[q], (size_t)n[q] * 8);
            memcpy((int32_t*)(h + o_ids) + at, bow_ids[q], (size_t)n[q] * 4);
        }
        at += (size_t)n[q];
    }
    off[nq] = (int32_t)at;
    if (S && db->table_dirty) {
        if (db->d_slots.count() < S && (rc = db->d_slots.alloc(std::max(S * 2, (size_t)256)))) return rc;
        HIPCHK(hipMemcpy(db->d_slots, db->slots.data(), S * sizeof(KfdbSlot), hipMemcpyHostToDevice));
        db->table_dirty = false;
    }
    hipStream_t st = fe->stream;
    if (S) {
        fe->kfdb.up(st, 0, o_score);
        KfdbQueryArgs A;
        A.poolIds = db->d_ids;
        A.poolVals = db->d_vals;
        A.slots = db->d_slots;
        A.nSlots = (int32_t)S;
        A.qVals = (const double*)(d + o_vals);
        A.qIds = (const int32_t*)(d + o_ids);
        A.qOff = (const int32_t*)(d + o_off);
        A.score = (double*)(d + o_score);
        A.words = (int32_t*)(d + o_words);
        A.first = (int32_t*)(d + o_first);
        hipLaunchKernelGGL(k_kfdb_query, dim3((unsigned)((S + KFDB_WAVES - 1) / KFDB_WAVES), (unsigned)nq),
                           dim3(64 * KFDB_WAVES), 0, st, A);
        fe->kfdb.down(st, o_score, bytes - o_score);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(db->ev, st));
    db->q_fe = fe;
    db->q_n = nq;
    db->q_slots = db->slots;
    db->q_kf = db->kf;
    db->q_o_score = o_score;
    db->q_o_words = o_words;
    db->q_o_first = o_first;
    return VSLAM_OK;
}

extern "C" int vslam_kfdb_query_wait(vslam_kfdb* db, vslam_fe* fe, int q, int cap, int64_t* hit_kf, int32_t* hit_map,
                                     int32_t* hit_words, float* hit_si, double* hit_score, int* n_hits) {
    if (!db || !fe || !n_hits || cap < 0) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->q_fe != fe || q < 0 || q >= db->q_n) {
        g_err = "KeyFrameDatabase: no such query enqueued on this context";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(db->device));
    HIPCHK(hipEventSynchronize(db->ev));
    const size_t S = db->q_slots.size();
    const uint8_t* h = fe->kfdb.h;
    const double* score = (const double*)(h + db->q_o_score) + (size_t)q * S;
    const int32_t* words = (const int32_t*)(h + db->q_o_words) + (size_t)q * S;
    const int32_t* first = (const int32_t*)(h + db->q_o_first) + (size_t)q * S;
    /* lKFsSharingWords: the walk over the query's words meets a keyframe at its smallest common word, and inside a
     * word's list in add order */
    std::vector<int> order;
    for (size_t s = 0; s < S; s++)
        if (db->q_slots[s].alive && words[s] > 0) order.push_back((int)s);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    *n_hits = (int)order.size();
    if ((int)order.size() > cap) {
        g_err = "KeyFrameDatabase: hit list larger than the caller's arrays";
        return VSLAM_ERR_CAPACITY;
    }
    for (size_t i = 0; i < order.size(); i++) {
        const int s = order[i];
        if (hit_kf) hit_kf[i] = db->q_kf[s];
        if (hit_map) hit_map[i] = db->q_slots[s].map;
        if (hit_words) hit_words[i] = words[s];
        if (hit_si) hit_si[i] = (float)score[s]; /* float si = mpVoc->score(...) */
        if (hit_score) hit_score[i] = score[s];
    }
    return VSLAM_OK;
}
