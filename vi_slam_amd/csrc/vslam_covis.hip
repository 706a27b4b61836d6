/* vslam_covis.hip -- the observation graph in HBM and the covisibility counts over it: KeyFrame::UpdateConnections
 * (keyframe.cpp:351-444), the vote of Tracking::UpdateLocalKeyFrames (tracking.cpp:3309-3376), KeyFrame::TrackedMapPoints
 * (:320-339) and the counting loop of LocalMapping::KeyFrameCulling (localmapping.cpp:990-1052).  The shadow and its
 * bookkeeping are vslam_covis_host.cpp; here are the device arrays, the upload of what changed, and the kernels.
 *
 * One enqueue: the dirty ranges of the shadow are copied into the staging block behind a descriptor list, the block goes
 * up in one copy, k_covis_apply scatters the ranges into the four device arrays, and ONE workgroup per job answers the
 * query; one range of results comes down.  All integer work: the histogram is filled by integer atomicAdd (the sums do
 * not depend on the order), every output position comes from a ballot / popcount prefix along ascending order_key or
 * from a rank sort. */
#include "vslam_covis.h"
#include "vslam_ctx.h"

#define COVIS_WG 256   /* k_covis_apply */
#define COVIS_QWG 1024 /* the query kernels: a thread per listed MapPoint walks dependent loads, so a job wants many of them */
#define COVIS_DESC_WORDS 4096 /* words one workgroup of k_covis_apply copies */

struct CovisJobDev { /* 32 bytes */
    int32_t mode, map, self, min_obs, n, list_off, out_off, error;
};
struct CovisResDev { /* 32 bytes */
    int32_t error, n_counter, n_ordered, n_max, slot_max, n_tracked, n_mps, n_redundant;
};

struct CovisApplyArgs {
    const int4* desc; /* { array, first word there, first word of the payload, words } */
    const int32_t* payload;
    int32_t* dst[4];
};

__global__ void __launch_bounds__(COVIS_WG) k_covis_apply(CovisApplyArgs A) {
    const int4 d = A.desc[blockIdx.x];
    int32_t* dst = A.dst[d.x] + (uint32_t)d.y;
    const int32_t* src = A.payload + (uint32_t)d.z;
    for (int i = threadIdx.x; i < d.w; i += COVIS_WG) dst[i] = src[i];
}

struct CovisQueryArgs {
    const int4* ktab;
    const int32_t* korder;
    const int4* ptab;
    const int2* pool;
    int32_t R; /* live keyframes = ranks */
    int32_t th_obs;
    const CovisJobDev* jobs;
    const int32_t* lists;  /* point slots; < 0: skipped */
    const int32_t* levels; /* culling */
    int32_t* scratch;      /* [jobs][R], zeroed: the histogram above COVIS_LDS_SLOTS */
    CovisResDev* res;
    int32_t *cslot, *ccount, *oslot, *ow;
};

/* One workgroup per job.  The histogram runs over RANKS (a keyframe's place in ascending order_key), so that reading it
 * front to back is the walk over std::map<KeyFrame*, int>. */
template <bool LDS>
__global__ void __launch_bounds__(COVIS_QWG) k_covis_connections(CovisQueryArgs A) {
    __shared__ int32_t s_hist[LDS ? COVIS_LDS_SLOTS : 1];
    __shared__ int s_tracked, s_base, s_nord, s_wsum[COVIS_QWG / 64];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovisJobDev J = A.jobs[blockIdx.x];
    if (J.error) {
        if (tid == 0) A.res[blockIdx.x] = CovisResDev{J.error, 0, 0, 0, -1, 0, 0, 0};
        return;
    }
    const int R = A.R;
    int32_t* hist = LDS ? s_hist : A.scratch + (size_t)blockIdx.x * (size_t)R;
    if (LDS)
        for (int r = tid; r < R; r += COVIS_QWG) s_hist[r] = 0;
    if (tid == 0) {
        s_tracked = 0;
        s_base = 0;
        s_nord = 0;
        s_best = 0ull;
    }
    __syncthreads();
    const bool conn = J.mode == VSLAM_COVIS_CONNECTIONS;
    int tracked = 0;
    for (int i = tid; i < J.n; i += COVIS_QWG) {
        const int p = A.lists[J.list_off + i];
        if (p < 0) continue; /* keyframe.cpp:367 */
        const int4 P = A.ptab[p];
        if (P.w & COVIS_BAD) continue;                          /* :370 */
        tracked += J.min_obs > 0 ? (P.z >= J.min_obs ? 1 : 0) : 1; /* :329-333 */
        for (int r = 0; r < P.y; r++) {
            const int k = A.pool[(uint32_t)P.x + (uint32_t)r].x;
            const int4 K = A.ktab[k];
            if (conn && (k == J.self || (K.z & COVIS_BAD) || K.y != J.map)) continue; /* :377 */
            atomicAdd(&hist[K.x], 1);
        }
    }
    if (tracked) atomicAdd(&s_tracked, tracked);
    __syncthreads();
    /* ascending order_key: 1024 ranks per round, kept entries packed by ballot prefixes */
    unsigned long long best = 0ull;
    for (int base = 0; base < R; base += COVIS_QWG) {
        const int r = base + tid;
        int c = 0, k = -1;
        bool keep = false;
        if (r < R) {
            c = LDS ? hist[r] : __hip_atomic_load(&hist[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c > 0) {
                k = A.korder[r];
                keep = conn || !(A.ktab[k].z & COVIS_BAD); /* tracking.cpp:3365 */
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wsum[wave] = __popcll(m);
        __syncthreads();
        int at = s_base + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) at += s_wsum[w];
        if (keep) {
            A.cslot[J.out_off + at] = k;
            A.ccount[J.out_off + at] = c;
            /* :402 `>` along ascending keys: the greatest count, and of those the smallest rank */
            const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (0xffffffffu - (uint32_t)r);
            best = key > best ? key : best;
        }
        __syncthreads();
        if (tid == 0) {
            int add = 0;
            for (int w = 0; w < COVIS_QWG / 64; w++) add += s_wsum[w];
            s_base += add;
        }
        __syncthreads();
    }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    const int nC = s_base;
    const int n_max = (int)(s_best >> 32);
    const int slot_max = nC ? A.korder[0xffffffffu - (uint32_t)(s_best & 0xffffffffull)] : -1;
    if (conn && nC) {
        /* mvpOrderedConnectedKeyFrames: descending (count, order_key) of the entries with count >= 15, by rank sort */
        for (int i = tid; i < nC; i += COVIS_QWG) {
            const int ci = A.ccount[J.out_off + i];
            if (ci < COVIS_TH_WEIGHT) continue;
            int pos = 0;
            for (int j = 0; j < nC; j++) {
                const int cj = A.ccount[J.out_off + j];
                pos += (cj >= COVIS_TH_WEIGHT && (cj > ci || (cj == ci && j > i))) ? 1 : 0;
            }
            A.oslot[J.out_off + pos] = A.cslot[J.out_off + i];
            A.ow[J.out_off + pos] = ci;
            atomicAdd(&s_nord, 1);
        }
        __syncthreads();
    }
    if (tid == 0) {
        int n_ord = s_nord;
        if (conn && nC && !n_ord) { /* :414-418 */
            A.oslot[J.out_off] = slot_max;
            A.ow[J.out_off] = n_max;
            n_ord = 1;
        }
        A.res[blockIdx.x] = CovisResDev{0, nC, n_ord, n_max, slot_max, s_tracked, 0, 0};
    }
}

/* One workgroup per keyframe of the culling loop, one thread per feature */
__global__ void __launch_bounds__(COVIS_QWG) k_covis_culling(CovisQueryArgs A) {
    __shared__ int s_mps, s_red;
    const int tid = threadIdx.x;
    const CovisJobDev J = A.jobs[blockIdx.x];
    if (J.error) {
        if (tid == 0) A.res[blockIdx.x] = CovisResDev{J.error, 0, 0, 0, -1, 0, 0, 0};
        return;
    }
    if (tid == 0) s_mps = s_red = 0;
    __syncthreads();
    int mps = 0, red = 0;
    for (int i = tid; i < J.n; i += COVIS_QWG) {
        const int p = A.lists[J.list_off + i];
        if (p < 0) continue; /* localmapping.cpp:999, :1003-1007 */
        const int4 P = A.ptab[p];
        if (P.w & COVIS_BAD) continue; /* :1001 */
        mps++;
        if (P.z <= A.th_obs) continue; /* :1010 */
        const int level = A.levels[J.list_off + i];
        int n = 0;
        for (int r = 0; r < P.y; r++) {
            const int2 o = A.pool[(uint32_t)P.x + (uint32_t)r];
            n += (o.x != J.self && o.y <= level + 1) ? 1 : 0; /* :1020, :1038 */
        }
        red += n > A.th_obs ? 1 : 0; /* :1045 */
    }
    if (mps) atomicAdd(&s_mps, mps);
    if (red) atomicAdd(&s_red, red);
    __syncthreads();
    if (tid == 0) A.res[blockIdx.x] = CovisResDev{0, 0, 0, 0, -1, 0, s_mps, s_red};
}

enum { COVIS_OP_CONNECTIONS = 1, COVIS_OP_CULLING = 2 };

struct vslam_covis {
    int device = 0;
    std::mutex mu;
    CovisStore s;
    vslam_dbuf<int32_t> d_ktab, d_korder, d_ptab, d_pool;
    vslam_staging st; /* descriptors | payload | jobs | lists | levels || histogram scratch || results | four list arrays */
    vslam_pending op;
    vslam_span_timer<2> t; /* before k_covis_apply | between | behind the query kernel */
    long long up_bytes = 0;
    vslam_event ev;
    vslam_fe* q_fe = nullptr;
    /* the query in flight / delivered last */
    std::vector<int64_t> q_kf; /* keyframe id of every slot, as it was */
    std::vector<int32_t> q_out_off;
    std::vector<CovisResDev> q_res;
    bool q_delivered = false;
    size_t o_res = 0, o_cslot = 0, o_ccount = 0, o_oslot = 0, o_ow = 0;
    explicit vslam_covis(size_t n) : s(n) {}
};

/* the kfdb_settle rule: nothing a kernel may still read, and no pinned range a copy may still read, changes under it */
static int covis_settle(vslam_covis* c) {
    if (c->op.in_flight()) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipEventSynchronize(c->ev));
    }
    return VSLAM_OK;
}

extern "C" int vslam_covis_create(int device, int initial_entries, vslam_covis** out) {
    if (!out || initial_entries < 0) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_err = "no usable HIP device (this library has no CPU fallback)";
        return VSLAM_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    vslam_covis* c = new vslam_covis((size_t)initial_entries);
    c->device = device;
    if (int rc = c->ev.ensure(hipEventDisableTiming)) {
        delete c;
        return rc;
    }
    *out = c;
    return VSLAM_OK;
}

extern "C" void vslam_covis_destroy(vslam_covis* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->op.in_flight()) hipEventSynchronize(c->ev);
    delete c;
}

extern "C" int vslam_covis_limits(int* max_jobs, int* max_list, int* lds_slots) {
    if (max_jobs) *max_jobs = VSLAM_COVIS_MAX_JOBS;
    if (max_list) *max_list = VSLAM_COVIS_MAX_LIST;
    if (lds_slots) *lds_slots = COVIS_LDS_SLOTS;
    return VSLAM_OK;
}

/* a mutator: settle, then the shadow's own function */
#define COVIS_MUTATOR(call)                       \
    if (!c) {                                     \
        g_err = "invalid arguments";              \
        return VSLAM_ERR_INVALID;                 \
    }                                             \
    std::lock_guard<std::mutex> lk(c->mu);        \
    if (int rc = covis_settle(c)) return rc;      \
    const int rc_ = c->s.call;                    \
    if (rc_) g_err = c->s.err;                    \
    return rc_

extern "C" int vslam_covis_add_keyframe(vslam_covis* c, int64_t kf_id, int32_t map_id, uint64_t order_key) {
    COVIS_MUTATOR(add_keyframe(kf_id, map_id, order_key));
}
extern "C" int vslam_covis_add_keyframes(vslam_covis* c, int n, const int64_t* kf_ids, const int32_t* map_ids,
                                         const uint64_t* order_keys) {
    COVIS_MUTATOR(add_keyframes(n, kf_ids, map_ids, order_keys));
}
extern "C" int vslam_covis_set_keyframe_bad(vslam_covis* c, int64_t kf_id) { COVIS_MUTATOR(set_keyframe_bad(kf_id)); }
extern "C" int vslam_covis_set_keyframe_map(vslam_covis* c, int64_t kf_id, int32_t map_id) {
    COVIS_MUTATOR(set_keyframe_map(kf_id, map_id));
}
extern "C" int vslam_covis_erase_keyframe(vslam_covis* c, int64_t kf_id) { COVIS_MUTATOR(erase_keyframe(kf_id)); }
extern "C" int vslam_covis_add_point(vslam_covis* c, int64_t mp_id) { COVIS_MUTATOR(add_point(mp_id)); }
extern "C" int vslam_covis_add_observation(vslam_covis* c, int64_t mp_id, int64_t kf_id, int32_t idx, int is_right, int level,
                                           int stereo) {
    COVIS_MUTATOR(add_observation(mp_id, kf_id, idx, is_right, level, stereo));
}
extern "C" int vslam_covis_erase_observation(vslam_covis* c, int64_t mp_id, int64_t kf_id, int* became_bad) {
    COVIS_MUTATOR(erase_observation(mp_id, kf_id, became_bad));
}
extern "C" int vslam_covis_clear_point(vslam_covis* c, int64_t mp_id) { COVIS_MUTATOR(clear_point(mp_id)); }
extern "C" int vslam_covis_erase_point(vslam_covis* c, int64_t mp_id) { COVIS_MUTATOR(erase_point(mp_id)); }
extern "C" int vslam_covis_clear_map(vslam_covis* c, int32_t map_id) { COVIS_MUTATOR(clear_map(map_id)); }
extern "C" int vslam_covis_clear(vslam_covis* c) { COVIS_MUTATOR(clear()); }

extern "C" int vslam_covis_size(vslam_covis* c, int* n_keyframes, int* n_points, long long* n_observations) {
    if (!c) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_keyframes) *n_keyframes = (int)c->s.kf_slot.size();
    if (n_points) *n_points = (int)c->s.mp_slot.size();
    if (n_observations) *n_observations = (long long)c->s.n_records;
    return VSLAM_OK;
}

extern "C" int vslam_covis_stats(vslam_covis* c, long long* capacity, long long* used, int* n_growths, int* n_compactions) {
    if (!c) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (capacity) *capacity = (long long)c->s.cap;
    if (used) *used = (long long)c->s.used;
    if (n_growths) *n_growths = (int)c->s.n_grow;
    if (n_compactions) *n_compactions = (int)c->s.n_compact;
    return VSLAM_OK;
}

extern "C" int vslam_covis_get_point(vslam_covis* c, int64_t mp_id, int cap, int* n_obs, int* bad, vslam_covis_obs* obs,
                                     int* n_records) {
    if (!c) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    const int rc = c->s.get_point(mp_id, cap, n_obs, bad, obs, n_records);
    if (rc) g_err = c->s.err;
    return rc;
}

/* ------------------------------------------------------------------ one enqueue */
struct CovisJobHost { /* what the two job types have in common */
    int32_t mode, map, min_obs, n;
    int64_t self;
    bool need_self;
    const int64_t* ids;
    const int32_t* levels;
};

static int covis_enqueue(vslam_covis* c, vslam_fe* fe, int kind, const std::vector<CovisJobHost>& jobs, int th_obs) {
    CovisStore& s = c->s;
    const int nj = (int)jobs.size();
    HIPCHK(hipSetDevice(c->device));
    s.refresh_ranks();
    const size_t R = s.korder.size();
    const bool lds = R <= COVIS_LDS_SLOTS;
    /* the device arrays: grown ones are filled whole */
    int rc;
    if (c->d_ptab.count() < s.ptab.w.size()) {
        if ((rc = c->d_ptab.alloc(std::max(s.ptab.w.size() * 2, (size_t)4096)))) return rc;
        s.ptab.all = true;
    }
    if (c->d_pool.count() < s.cap * 2) {
        if ((rc = c->d_pool.alloc(s.cap * 2))) return rc;
        s.pool.all = true;
    }
    if (c->d_ktab.count() < s.ktab.size() && (rc = c->d_ktab.alloc(std::max(s.ktab.size() * 2, (size_t)1024)))) return rc;
    if (c->d_korder.count() < R && (rc = c->d_korder.alloc(std::max(R * 2, (size_t)256)))) return rc;
    /* what changed, as ranges of the four arrays; an enqueue that fails behind this point sends everything next time */
    struct Resend {
        CovisStore& s;
        bool done = false;
        ~Resend() {
            if (!done) s.k_upload = s.ptab.all = s.pool.all = true;
        }
    } resend{s};
    std::vector<CovisRange> rg[4];
    const int32_t* src[4] = {s.ktab.data(), s.korder.data(), s.ptab.w.data(), s.pool.w.data()};
    const size_t room[4] = {c->d_ktab.count(), c->d_korder.count(), c->d_ptab.count(), c->d_pool.count()};
    if (s.k_upload) {
        if (!s.ktab.empty()) rg[0].push_back({0u, (uint32_t)s.ktab.size()});
        if (R) rg[1].push_back({0u, (uint32_t)R});
        s.k_upload = false;
    }
    s.ptab.take(s.ptab.w.size(), rg[2]);
    s.pool.take(s.used * 2, rg[3]);
    size_t n_desc = 0, n_words = 0;
    for (int a = 0; a < 4; a++)
        for (const CovisRange& r : rg[a]) {
            if ((size_t)r.off + r.n > room[a]) {
                g_err = "covis: an upload range lies outside its device array";
                return VSLAM_ERR_HIP;
            }
            n_desc += (r.n + COVIS_DESC_WORDS - 1) / COVIS_DESC_WORDS;
            n_words += r.n;
        }
    size_t n_list = 0;
    for (const CovisJobHost& J : jobs) n_list += (size_t)J.n;
    /* the jobs: ids to point slots, errors, and an upper bound of every counter */
    std::vector<CovisJobDev> jd((size_t)nj);
    std::vector<int32_t> slots(n_list);
    size_t at = 0, out_total = 0;
    for (int j = 0; j < nj; j++) {
        const CovisJobHost& J = jobs[(size_t)j];
        CovisJobDev D{J.mode, J.map, -1, J.min_obs, J.n, (int32_t)at, (int32_t)out_total, 0};
        if (J.need_self) {
            auto ki = s.kf_slot.find(J.self);
            if (ki == s.kf_slot.end()) D.error |= 2;
            else D.self = ki->second;
        }
        size_t records = 0;
        for (int i = 0; i < J.n; i++) {
            int32_t p = -1;
            if (J.ids[i] != -1) {
                auto pi = s.mp_slot.find(J.ids[i]);
                if (pi == s.mp_slot.end()) D.error |= 1;
                else {
                    p = pi->second;
                    records += (size_t)s.ptab.w[(size_t)p * 4 + 1];
                }
            }
            slots[at + (size_t)i] = p;
        }
        at += (size_t)J.n;
        if (kind == COVIS_OP_CONNECTIONS && !D.error) out_total += std::min(records, R);
        jd[(size_t)j] = D;
    }
    const bool cull = kind == COVIS_OP_CULLING;
    const auto [o_desc, o_pay, o_jobs, o_lists, o_levels, o_scratch, o_res, o_cslot, o_ccount, o_oslot, o_ow, bytes] =
        vslam::layout(16, {n_desc * 16, n_words * 4, (size_t)nj * sizeof(CovisJobDev), n_list * 4, cull ? n_list * 4 : 0,
                           (!cull && !lds) ? (size_t)nj * R * 4 : 0, (size_t)nj * sizeof(CovisResDev), out_total * 4,
                           out_total * 4, out_total * 4, out_total * 4});
    if ((rc = c->st.ensure(bytes))) return rc;
    if ((rc = c->t.arm(fe->profiling))) return rc;
    uint8_t *h = c->st.h, *d = c->st.d;
    int32_t* desc = (int32_t*)(h + o_desc);
    int32_t* pay = (int32_t*)(h + o_pay);
    size_t nd = 0, pw = 0;
    for (int a = 0; a < 4; a++)
        for (const CovisRange& r : rg[a]) {
            memcpy(pay + pw, src[a] + r.off, (size_t)r.n * 4);
            for (uint32_t o = 0; o < r.n; o += COVIS_DESC_WORDS) {
                desc[nd * 4 + 0] = a;
                desc[nd * 4 + 1] = (int32_t)(r.off + o);
                desc[nd * 4 + 2] = (int32_t)(pw + o);
                desc[nd * 4 + 3] = (int32_t)std::min((uint32_t)COVIS_DESC_WORDS, r.n - o);
                nd++;
            }
            pw += r.n;
        }
    memcpy(h + o_jobs, jd.data(), (size_t)nj * sizeof(CovisJobDev));
    if (n_list) memcpy(h + o_lists, slots.data(), n_list * 4);
    if (cull) {
        size_t l = 0;
        for (const CovisJobHost& J : jobs) {
            if (J.n) memcpy((int32_t*)(h + o_levels) + l, J.levels, (size_t)J.n * 4);
            l += (size_t)J.n;
        }
    }
    hipStream_t st = fe->stream;
    c->st.up(st, 0, o_scratch);
    if (!cull && !lds) HIPCHK(hipMemsetAsync(d + o_scratch, 0, (size_t)nj * R * 4, st));
    c->t.mark(0, st);
    if (n_desc) {
        CovisApplyArgs P;
        P.desc = (const int4*)(d + o_desc);
        P.payload = (const int32_t*)(d + o_pay);
        P.dst[0] = c->d_ktab;
        P.dst[1] = c->d_korder;
        P.dst[2] = c->d_ptab;
        P.dst[3] = c->d_pool;
        hipLaunchKernelGGL(k_covis_apply, dim3((unsigned)n_desc), dim3(COVIS_WG), 0, st, P);
    }
    c->t.mark(1, st);
    CovisQueryArgs A;
    A.ktab = (const int4*)c->d_ktab.get();
    A.korder = c->d_korder;
    A.ptab = (const int4*)c->d_ptab.get();
    A.pool = (const int2*)c->d_pool.get();
    A.R = (int32_t)R;
    A.th_obs = th_obs;
    A.jobs = (const CovisJobDev*)(d + o_jobs);
    A.lists = (const int32_t*)(d + o_lists);
    A.levels = (const int32_t*)(d + o_levels);
    A.scratch = (int32_t*)(d + o_scratch);
    A.res = (CovisResDev*)(d + o_res);
    A.cslot = (int32_t*)(d + o_cslot);
    A.ccount = (int32_t*)(d + o_ccount);
    A.oslot = (int32_t*)(d + o_oslot);
    A.ow = (int32_t*)(d + o_ow);
    if (cull) hipLaunchKernelGGL(k_covis_culling, dim3((unsigned)nj), dim3(COVIS_QWG), 0, st, A);
    else if (lds) hipLaunchKernelGGL(k_covis_connections<true>, dim3((unsigned)nj), dim3(COVIS_QWG), 0, st, A);
    else hipLaunchKernelGGL(k_covis_connections<false>, dim3((unsigned)nj), dim3(COVIS_QWG), 0, st, A);
    c->t.mark(2, st);
    HIPCHK(hipGetLastError());
    c->st.down(st, o_res, bytes - o_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev, st));
    if (fe->profiling) c->up_bytes += (long long)o_scratch;
    c->q_fe = fe;
    c->q_kf = s.kf_id;
    c->q_out_off.resize((size_t)nj);
    for (int j = 0; j < nj; j++) c->q_out_off[(size_t)j] = jd[(size_t)j].out_off;
    c->q_delivered = false;
    c->o_res = o_res;
    c->o_cslot = o_cslot;
    c->o_ccount = o_ccount;
    c->o_oslot = o_oslot;
    c->o_ow = o_ow;
    c->op.jobs = nj;
    c->op.set(false, kind);
    resend.done = true;
    return VSLAM_OK;
}

static int covis_begin(vslam_covis* c, vslam_fe* fe) {
    if (!c || !fe || fe->p.device != c->device) {
        g_err = "invalid arguments (the mirror must live on the context's device)";
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

/* the wait of both queries: the device results of the jobs */
static int covis_wait(vslam_covis* c, vslam_fe* fe, int kind) {
    if (int rc = c->op.ready(kind, "the other covisibility query is enqueued on this mirror")) return rc;
    if (c->q_fe != fe) {
        g_err = "covis: the query was enqueued on another context";
        return VSLAM_ERR_INVALID;
    }
    c->op.take();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev));
    if (int rc = c->t.collect()) return rc;
    const CovisResDev* r = (const CovisResDev*)(c->st.h + c->o_res);
    c->q_res.assign(r, r + c->op.jobs);
    c->q_delivered = kind == COVIS_OP_CONNECTIONS;
    return VSLAM_OK;
}

extern "C" int vslam_covis_connections_async(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_job* jobs) {
    if (int rc = covis_begin(c, fe)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = c->op.begin("a covisibility query is already in flight on this mirror")) return rc;
    if (int rc = covis_jobs_ok(n_jobs, jobs, g_err)) return rc;
    std::vector<CovisJobHost> J((size_t)n_jobs);
    for (int j = 0; j < n_jobs; j++)
        J[(size_t)j] = CovisJobHost{jobs[j].mode, jobs[j].map_id, jobs[j].min_obs, jobs[j].n, jobs[j].self_kf,
                                    jobs[j].mode == VSLAM_COVIS_CONNECTIONS, jobs[j].mp_ids, nullptr};
    return covis_enqueue(c, fe, COVIS_OP_CONNECTIONS, J, 0);
}

extern "C" int vslam_covis_connections_wait(vslam_covis* c, vslam_fe* fe, vslam_covis_result* results) {
    if (!c || !fe || !results) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = covis_wait(c, fe, COVIS_OP_CONNECTIONS)) return rc;
    for (size_t j = 0; j < c->q_res.size(); j++) {
        const CovisResDev& r = c->q_res[j];
        results[j] = vslam_covis_result{r.error, r.n_counter, r.n_ordered, r.n_max,
                                        r.slot_max >= 0 ? c->q_kf[(size_t)r.slot_max] : -1, r.n_tracked, 0};
    }
    return VSLAM_OK;
}

extern "C" int vslam_covis_connections(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_job* jobs,
                                       vslam_covis_result* results) {
    if (!results) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const int rc = vslam_covis_connections_async(c, fe, n_jobs, jobs);
    return rc ? rc : vslam_covis_connections_wait(c, fe, results);
}

extern "C" int vslam_covis_connections_lists(vslam_covis* c, int job, int64_t* counter_kf, int32_t* counter_n,
                                             int64_t* ordered_kf, int32_t* ordered_w) {
    if (!c) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->q_delivered || c->op.in_flight() || job < 0 || job >= (int)c->q_res.size()) {
        g_err = "covis: no such job in a delivered connections query";
        return VSLAM_ERR_INVALID;
    }
    const CovisResDev& r = c->q_res[(size_t)job];
    const size_t o = (size_t)c->q_out_off[(size_t)job];
    const uint8_t* h = c->st.h;
    const int32_t *cs = (const int32_t*)(h + c->o_cslot) + o, *cc = (const int32_t*)(h + c->o_ccount) + o;
    const int32_t *os = (const int32_t*)(h + c->o_oslot) + o, *ow = (const int32_t*)(h + c->o_ow) + o;
    for (int i = 0; i < r.n_counter; i++) {
        if (counter_kf) counter_kf[i] = c->q_kf[(size_t)cs[i]];
        if (counter_n) counter_n[i] = cc[i];
    }
    for (int i = 0; i < r.n_ordered; i++) {
        if (ordered_kf) ordered_kf[i] = c->q_kf[(size_t)os[i]];
        if (ordered_w) ordered_w[i] = ow[i];
    }
    return VSLAM_OK;
}

extern "C" int vslam_covis_culling_async(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_cull_job* jobs, int th_obs) {
    if (int rc = covis_begin(c, fe)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = c->op.begin("a covisibility query is already in flight on this mirror")) return rc;
    if (int rc = covis_cull_jobs_ok(n_jobs, jobs, th_obs, g_err)) return rc;
    std::vector<CovisJobHost> J((size_t)n_jobs);
    for (int j = 0; j < n_jobs; j++) J[(size_t)j] = CovisJobHost{0, 0, 0, jobs[j].n, jobs[j].kf_id, true, jobs[j].mp_ids, jobs[j].levels};
    return covis_enqueue(c, fe, COVIS_OP_CULLING, J, th_obs);
}

extern "C" int vslam_covis_culling_wait(vslam_covis* c, vslam_fe* fe, vslam_covis_cull_result* results) {
    if (!c || !fe || !results) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = covis_wait(c, fe, COVIS_OP_CULLING)) return rc;
    for (size_t j = 0; j < c->q_res.size(); j++)
        results[j] = vslam_covis_cull_result{c->q_res[j].error, c->q_res[j].n_mps, c->q_res[j].n_redundant, 0};
    return VSLAM_OK;
}

extern "C" int vslam_covis_culling(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_cull_job* jobs, int th_obs,
                                   vslam_covis_cull_result* results) {
    if (!results) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const int rc = vslam_covis_culling_async(c, fe, n_jobs, jobs, th_obs);
    return rc ? rc : vslam_covis_culling_wait(c, fe, results);
}

extern "C" int vslam_covis_get_profile(vslam_covis* c, double* apply_ms, double* query_ms, long long* upload_bytes, long* passes) {
    if (!c) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    c->t.read({apply_ms, query_ms}, passes);
    if (upload_bytes) *upload_bytes = c->up_bytes;
    return VSLAM_OK;
}
