/* vslam_init_kernel.hip -- FMatcher::SearchForInitialization (fmatcher.cpp:983-1098) entirely on the GPU.
 *
 * The reference loop is sequential over the octave-0 keypoints of frame 1 (a later query may steal an
 * earlier query's match, and a candidate whose current owner is at least as close is skipped).  Only that
 * skip/steal bookkeeping is order-dependent; the expensive part -- which frame-2 keypoints lie in a query's
 * window and how far their descriptors are -- is not.  Two kernels:
 *
 *   k_si_topm   (parallel, one wave per query, all pairs at once): every window candidate gets
 *               key = min(dist,255) << 24 | gridcell << 12 | slot, i.e. (distance, position in
 *               Frame::GetFeaturesInArea's output: grid cell column-major, ascending index inside a cell,
 *               frame.cpp:712-741).  The M smallest keys of each query are written in ascending order.
 *   k_si_replay (one wave per pair, queries in index order): the first two list entries that are not skipped
 *               (vMatchedDistance[i2] <= dist, fmatcher.cpp:1022) are bestDist/bestIdx2 and bestDist2 --
 *               "first wins" on equal distance is the key order, bestDist2 is the multiset second minimum.
 *               A list is a sorted prefix of all candidates, so this is exact whenever two survivors are found
 *               (or the list is not full, or the last list entry already decides the ratio test); otherwise
 *               the wave re-scans that query's window in full (rare; forced in tests with a tiny M).
 *               Acceptance (TH_LOW, ratio test in float), stealing, the 30-bin rotation histogram and
 *               ComputeThreeMaxima follow the reference literally.
 *
 * Distances are clamped to 255 inside the key (the only other value is 256): an accepted best and every
 * owner's distance are <= TH_LOW = 50, so the clamp can only matter through the ratio test against a second
 * of exactly 256, and nnratio * 255 > 50 for every nnratio >= 0.2 -- the host wrapper refuses smaller ratios.
 */
#include "vslam_kernels.h"
#include "vslam_wave.h"
#include "vslam_matchdev.h"

#define SI_TH_LOW 50
#define SI_QPB_MAX 32 /* queries per k_si_topm workgroup: run-time (4 waves x 2..8), see vk_search_init */

struct SiCand { /* one octave-0 keypoint of frame 2 */
    float x, y, angle;
    uint16_t cell; /* gridX * 64 + gridY (gridY < 48) */
    uint16_t idx;  /* index in frame 2 */
};
struct SiCandL { /* the same in k_si_topm's LDS list, which is sorted by grid column: the position c in the
                   keypoint-ordered list (what the keys and k_si_replay refer to) instead of the angle */
    float x, y;
    uint32_t c;
    uint16_t cell;
    uint16_t idx;
};
struct SiQuery { /* one octave-0 keypoint of frame 1 */
    float px, py, angle; /* vbPrevMatched position, keypoint angle */
    uint32_t idx;
};

/* per-pair scratch in HBM: [c1, c2, pad, pad] | SiCand[max_c2] | SiQuery[max_c2] | topm[max_c2][M] */
__host__ __device__ inline size_t si_pair_bytes(int max_c2, int M) {
    return 16 + (size_t)max_c2 * (sizeof(SiCand) + sizeof(SiQuery) + 4 * (size_t)M);
}

/* ------------------------------------------------------------------------------------------------
 * phase A: grid (chunks of SI_QPB queries, pairs), 256 threads.  Every workgroup compacts the octave-0
 * keypoints of both frames in index order (block scan per 256), keeps frame 2's in LDS, and ranks the window
 * candidates of its own queries.  Chunk 0 also publishes the compacted candidate list and the counts.
 * ---------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256)
k_si_topm(InitJobs jobs, int cap, SiBounds bnd, int window, int max_c2, int M, uint8_t* scratch, int SI_QPB) {
    extern __shared__ __align__(16) uint8_t sism[];
    SiCandL* cand = (SiCandL*)sism;                  /* max_c2, sorted by grid column */
    uint32_t* wkeys = (uint32_t*)(cand + max_c2);    /* 4 waves x max_c2: window keys of the current query */
    SiCandL* tmpc = (SiCandL*)wkeys;                 /* ... and, before that, the list in keypoint order */
    __shared__ SiQuery s_q[SI_QPB_MAX];
    __shared__ int s_wcnt[4];
    __shared__ int s_col[SI_GRID_COLS + 1]; /* candidates per grid column, then the columns' first positions */
    __shared__ int s_fill[SI_GRID_COLS];
    if (threadIdx.x <= SI_GRID_COLS) s_col[threadIdx.x] = 0;
    if (threadIdx.x < SI_GRID_COLS) s_fill[threadIdx.x] = 0;
    __syncthreads();
    const InitJob jb = jobs.job[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = min(*jb.cnt1, cap), n2 = min(*jb.cnt2, cap);
    uint8_t* sp = scratch + (size_t)blockIdx.y * si_pair_bytes(max_c2, M);
    int32_t* hdr = (int32_t*)sp;
    SiCand* gcand = (SiCand*)(sp + 16);
    SiQuery* gqry = (SiQuery*)(gcand + max_c2);
    uint32_t* topm = (uint32_t*)(gqry + max_c2);
    const int q0 = blockIdx.x * SI_QPB;

    const SiGridInv inv = si_grid_inv(bnd); /* Frame grid of frame 2 */

    int c2 = 0;
    for (int b = 0; b < n2; b += 256) {
        const int i = b + tid;
        bool take = false;
        vslam_kp k;
        int cell = -1;
        if (i < n2) {
            k = jb.k2[i];
            if (k.octave == 0) {
                /* keypoints outside the grid are rejected here, before anything is packed into the u16 cell or the
                 * 12-bit key field */
                cell = si_grid_cell(k.x, k.y, bnd, inv);
                take = cell >= 0;
            }
        }
        const unsigned long long m = __ballot(take);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int pos = c2 + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) pos += s_wcnt[w];
        if (take && pos < max_c2) {
            SiCand cd;
            cd.x = k.x;
            cd.y = k.y;
            cd.angle = k.angle;
            cd.cell = (uint16_t)cell;
            cd.idx = (uint16_t)i;
            if (blockIdx.x == 0) gcand[pos] = cd;
            SiCandL cl;
            cl.x = k.x;
            cl.y = k.y;
            cl.c = (uint32_t)pos;
            cl.cell = cd.cell;
            cl.idx = cd.idx;
            tmpc[pos] = cl;
            atomicAdd(&s_col[cell >> 6], 1);
        }
        c2 += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    const int c2_raw = c2;
    c2 = min(c2, max_c2);
    /* sort the list by grid column (order inside a column is irrelevant: keys are unique), so that a query only visits
     * the columns of its window -- a sixth of the list at window 100 on a KITTI frame -- instead of testing all of it */
    if (wave == 0) {
        const int v = s_col[lane];
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        s_col[lane] = inc - v;
        if (lane == 63) s_col[SI_GRID_COLS] = inc;
    }
    __syncthreads();
    for (int i = tid; i < c2; i += 256) {
        const SiCandL e = tmpc[i];
        const int gx = e.cell >> 6;
        cand[s_col[gx] + atomicAdd(&s_fill[gx], 1)] = e;
    }
    __syncthreads();
    int c1 = 0;
    for (int b = 0; b < n1; b += 256) {
        const int i = b + tid;
        vslam_kp k;
        bool take = false;
        if (i < n1) {
            k = jb.k1[i];
            take = k.octave == 0; /* level1 > 0 -> continue, fmatcher.cpp:999-1001 */
        }
        const unsigned long long m = __ballot(take);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int pos = c1 + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) pos += s_wcnt[w];
        if (take && pos >= q0 && pos < q0 + SI_QPB && pos < max_c2) {
            SiQuery q;
            q.px = jb.prev ? jb.prev[2 * i] : k.x;
            q.py = jb.prev ? jb.prev[2 * i + 1] : k.y;
            q.angle = k.angle;
            q.idx = (uint32_t)i;
            s_q[pos - q0] = q;
            gqry[pos] = q;
        }
        c1 += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    const int c1_raw = c1;
    c1 = min(c1, max_c2);
    if (blockIdx.x == 0 && tid == 0) {
        hdr[0] = c1;
        hdr[1] = c2;
        /* more octave-0 keypoints than the LDS-resident lists hold (keypoints of a foreign extractor configuration):
         * the result would be silently truncated, so k_si_replay reports the pair as failed instead */
        hdr[2] = (c1_raw > max_c2 || c2_raw > max_c2) ? 1 : 0;
    }

    const float r = (float)window;
    uint32_t* wk = wkeys + (size_t)wave * max_c2;
    for (int t = q0 + wave; t < min(c1, q0 + SI_QPB); t += 4) {
        const SiQuery qq = s_q[t - q0];
        const SiWindow win = si_window_b(qq.px, qq.py, r, bnd, inv);
        uint32_t mine = 0xFFFFFFFFu; /* lane j < M ends up with the j-th smallest key */
        if (!win.empty) {
            const uint4 da = ((const uint4*)jb.d1)[(size_t)qq.idx * 2];
            const uint4 db = ((const uint4*)jb.d1)[(size_t)qq.idx * 2 + 1];
            int nk = 0; /* window candidates, compacted (their order is irrelevant: keys are unique) */
            const int lo = s_col[win.minX], hi = s_col[win.maxX + 1]; /* 0 <= minX <= maxX <= 63 for a non-empty window */
            for (int cb = lo; cb < hi; cb += 64) {
                const int c = cb + lane;
                bool in = false;
                uint32_t key = 0;
                if (c < hi) {
                    const SiCandL cd = cand[c];
                    if (si_in_window(cd, win, qq.px, qq.py, r)) {
                        const uint4 ta = ((const uint4*)jb.d2)[(size_t)cd.idx * 2];
                        const uint4 tb = ((const uint4*)jb.d2)[(size_t)cd.idx * 2 + 1];
                        const uint32_t dist = si_hamming(da, db, ta, tb);
                        key = si_key(dist, cd.cell, cd.c);
                        in = true;
                    }
                }
                const unsigned long long m = __ballot(in);
                if (in) wk[nk + __popcll(m & ((1ull << lane) - 1ull))] = key;
                nk += __popcll(m);
            }
            /* M rounds of "smallest key not yet taken" (keys are unique; same wave, LDS is in order) */
            uint32_t lower = 0;
            for (int j = 0; j < M; j++) {
                uint32_t lm = 0xFFFFFFFFu;
                for (int e = lane; e < nk; e += 64) {
                    const uint32_t kv = wk[e];
                    if (kv >= lower) lm = min(lm, kv);
                }
                const uint32_t g = wave_min_u32(lm);
                if (g == 0xFFFFFFFFu) break;
                if (lane == j) mine = g;
                lower = g + 1u;
            }
        }
        if (lane < M) topm[(size_t)t * M + lane] = mine;
    }
}

/* vMatchedDistance as the replay keeps it: per frame-2 slot up to four (writer + 1) << 8 | distance entries (0xFFFFFFFF =
 * empty; writer field 0 = merged entries of queries that everybody still pending comes after).  A query sees the
 * acceptances of EARLIER queries only -- later queries may have committed before it (see k_si_replay). */
__device__ __forceinline__ uint32_t sir_od_eff(const uint4 L, uint32_t q) {
    uint32_t od = 0x7FFFFFFFu;
    if ((L.x >> 8) <= q) od = min(od, L.x & 0xFFu);
    if ((L.y >> 8) <= q) od = min(od, L.y & 0xFFu);
    if ((L.z >> 8) <= q) od = min(od, L.z & 0xFFu);
    if ((L.w >> 8) <= q) od = min(od, L.w & 0xFFu);
    return od;
}

/* Full re-scan of one query's window (the reference loop body, fmatcher.cpp:1003-1035) by ONE wave: used when the query's
 * sorted prefix ran out.  Returns the best key; *second_out = bestDist2 (0x7FFFFFFF if none). */
__device__ uint32_t si_full_scan(const InitJob& jb, const SiCand* gcand, const uint4* slotlog, int c2, int lane,
                                 const SiQuery& qq, uint32_t qpos, float r, const SiBounds& bnd, const SiGridInv& inv,
                                 uint32_t* second_out) {
    const SiWindow win = si_window_b(qq.px, qq.py, r, bnd, inv);
    uint32_t bestKey = 0xFFFFFFFFu, second = 0x7FFFFFFFu; /* per lane: best key, smallest other distance */
    if (!win.empty) {
        const uint4 da = ((const uint4*)jb.d1)[(size_t)qq.idx * 2];
        const uint4 db = ((const uint4*)jb.d1)[(size_t)qq.idx * 2 + 1];
        for (int c = lane; c < c2; c += 64) {
            const SiCand cd = gcand[c];
            if (!si_in_window(cd, win, qq.px, qq.py, r)) continue;
            const uint4 ta = ((const uint4*)jb.d2)[(size_t)cd.idx * 2];
            const uint4 tb = ((const uint4*)jb.d2)[(size_t)cd.idx * 2 + 1];
            const uint32_t dist = min(si_hamming(da, db, ta, tb), 255u);
            if (sir_od_eff(slotlog[c], qpos) <= dist) continue; /* vMatchedDistance[i2] <= dist, fmatcher.cpp:1022 */
            const uint32_t key = si_key(dist, cd.cell, (uint32_t)c);
            if (key < bestKey) {
                if (bestKey != 0xFFFFFFFFu) second = min(second, si_key_dist(bestKey));
                bestKey = key;
            } else {
                second = min(second, dist);
            }
        }
    }
    const uint32_t gBest = wave_min_u32(bestKey);
    /* second minimum over the multiset: lanes that do not hold the winner contribute their own best */
    uint32_t contrib = second;
    if (bestKey != gBest && bestKey != 0xFFFFFFFFu) contrib = min(contrib, si_key_dist(bestKey));
    *second_out = wave_min_u32(contrib);
    return gBest;
}

/* append (writer q, distance d) to a slot's entries; `merge`: the writer is the smallest pending query, so every entry
 * present comes from an earlier query and is visible to everybody still pending -- they collapse into one.  Returns
 * false if the slot is full and merging is not allowed. */
__device__ __forceinline__ bool sir_slot_append(uint4* slotlog, uint32_t slot, uint32_t q, uint32_t d, bool merge) {
    uint4 L = slotlog[slot];
    const uint32_t e = ((q + 1u) << 8) | d;
    if (L.x == 0xFFFFFFFFu) L.x = e;
    else if (L.y == 0xFFFFFFFFu) L.y = e;
    else if (L.z == 0xFFFFFFFFu) L.z = e;
    else if (L.w == 0xFFFFFFFFu) L.w = e;
    else if (merge) {
        const uint32_t dm = min(min(L.x & 0xFFu, L.y & 0xFFu), min(L.z & 0xFFu, L.w & 0xFFu));
        L = make_uint4(dm, e, 0xFFFFFFFFu, 0xFFFFFFFFu);
    } else {
        return false;
    }
    slotlog[slot] = L;
    return true;
}

/* ------------------------------------------------------------------------------------------------
 * phase B: one workgroup per pair; the sequential loop of fmatcher.cpp:1003-1049 decided in a few rounds.
 *
 * The loop carries ONE piece of state, vMatchedDistance, and a query's decision is a function of its FIRST TWO
 * candidates (in key order) that are not skipped (vMatchedDistance[i2] <= dist, :1022); skipped ones never come back,
 * the array only decreases.  So a query's decision is final as soon as no EARLIER undecided query can still accept one
 * of those two slots -- and an undecided query can only ever accept a slot that is in its sorted prefix, not skipped,
 * with a distance <= TH_LOW (:1037).  Every round, all undecided queries at once:
 *   1. each evaluates the loop body against the acceptances of the queries BEFORE it (the per-slot entries carry their
 *      writer, so an acceptance committed early by a later query is invisible to it) and publishes its index at every
 *      slot it might still accept (atomicMin);
 *   2. a query whose best and second-best slots show no smaller index commits: appends its acceptance to the slot's
 *      entries and to the log.  The smallest undecided query always commits, so the rounds end; on consecutive KITTI-like
 *      frames 217 (436) queries take 4-6 rounds (tests/tools/replay_sim.py), where committing only the prefix in front of
 *      the first dependent query of a 64-query window (round 3's first version) took 30 (48) and one query per step 217.
 * Two rare cases wait until they are the smallest undecided query: a query whose sorted prefix ran out and that needs the
 * re-scan of its whole window (its second-best lies beyond the list) -- and while an undecided query could accept a slot
 * BEYOND its list (full list, last listed distance <= TH_LOW), nothing behind it commits.
 * Ownership ("last acceptor wins", which is what the reference's steal/undo amounts to), vnMatches12 and the rotation
 * histogram are rebuilt from the log in parallel afterwards.
 * ---------------------------------------------------------------------------------------------- */
#ifndef SIR_NT
#define SIR_NT 256
#endif
#define SIR_PEND 1u
#define SIR_ACC 2u
#define SIR_SCAN 4u
template <int MAXM> /* unrolled length of a query's sorted prefix: 8 (the default M) or SI_MAX_M */
__global__ void __launch_bounds__(SIR_NT)
k_si_replay(InitJobs jobs, int cap, SiBounds bnd, int window, float nnratio, int checkOri,
            int32_t* matches_out /* [pair][cap] */, float* prev_out /* [pair][2*cap] */,
            int32_t* nmatch_out /* [pair] */, int max_c2, int M, const uint8_t* scratch, int* fallbacks, int keys_lds_bytes) {
    extern __shared__ __align__(16) uint8_t sism[];
    const InitJob jb = jobs.job[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n1 = min(*jb.cnt1, cap);
    const uint8_t* sp = scratch + (size_t)blockIdx.x * si_pair_bytes(max_c2, M);
    const int32_t* hdr = (const int32_t*)sp;
    const SiCand* gcand = (const SiCand*)(sp + 16);
    const SiQuery* gqry = (const SiQuery*)(gcand + max_c2);
    const uint32_t* topm = (const uint32_t*)(gqry + max_c2);
    const int c1 = hdr[0], c2 = hdr[1];
    /* LDS: slotlog | lister[2] | kfirst | ksecond | alog | m12 | qstate | rotBin */
    uint4* slotlog = (uint4*)sism;                                /* vMatchedDistance with writers, max_c2 */
    int32_t* lister0 = (int32_t*)(slotlog + max_c2);              /* smallest undecided query that may still accept the slot */
    int32_t* lister1 = lister0 + max_c2;                          /* (two buffers: one is reset while the other is in use) */
    uint32_t* kfirst = (uint32_t*)(lister1 + max_c2);             /* this round's best / second-best key of a query */
    uint32_t* ksecond = kfirst + max_c2;
    uint32_t* alog = ksecond + max_c2;                            /* accepted (query position << 12 | slot), any order */
    int32_t* m12 = (int32_t*)(alog + max_c2);                     /* vnMatches12, cap */
    uint8_t* qstate = (uint8_t*)(m12 + cap);                      /* SIR_* flags per query, max_c2 */
    uint8_t* rotBin = qstate + max_c2;                            /* bin of an accepted query, 255 = none; cap */
    /* the queries' sorted prefixes are read once per round: kept in LDS when they fit what the host set aside */
    uint32_t* keys_lds = (uint32_t*)(sism + (((size_t)max_c2 * 37 + (size_t)cap * 5 + 15) & ~(size_t)15));
    const bool keys_in_lds = (size_t)c1 * M * 4 <= (size_t)keys_lds_bytes;
    const uint32_t* keysrc = keys_in_lds ? keys_lds : topm;
    if (keys_in_lds)
        for (int i = tid; i < c1 * M; i += SIR_NT) keys_lds[i] = topm[i];
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    __shared__ int s_minpend[2], s_minwild[2], s_scanq, s_nlog, s_cnt;

    int32_t* mo = matches_out + (size_t)blockIdx.x * cap;
    float* po = prev_out + (size_t)blockIdx.x * cap * 2;
    const SiGridInv inv = si_grid_inv(bnd);
    const float r = (float)window;

    for (int c = tid; c < c2; c += SIR_NT) {
        slotlog[c] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        lister0[c] = 0x7FFFFFFF;
        lister1[c] = 0x7FFFFFFF;
    }
    for (int q = tid; q < c1; q += SIR_NT) qstate[q] = (uint8_t)SIR_PEND;
    for (int i = tid; i < n1; i += SIR_NT) {
        m12[i] = -1;
        rotBin[i] = 255;
    }
    if (tid < VSLAM_HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) {
        s_minpend[0] = s_minpend[1] = 0x7FFFFFFF;
        s_minwild[0] = s_minwild[1] = 0x7FFFFFFF;
        s_scanq = -1;
        s_nlog = 0;
        s_cnt = 0;
    }
    __syncthreads();

    int nfb = 0, nrounds = 0;
    for (int par = 0;; par ^= 1) {
        int32_t* lister = par ? lister1 : lister0;
        if (tid == 0) s_scanq = -1; /* everybody has read last round's value (it is only set in part 2, behind a barrier) */
        /* ---- 1: the reference's loop body (fmatcher.cpp:1003-1039) for every undecided query, as the queries before it left the state */
        for (int q = tid; q < c1; q += SIR_NT) {
            if (!(qstate[q] & SIR_PEND)) continue;
            uint32_t key[MAXM];
#pragma unroll
            for (int j = 0; j < MAXM; j++) key[j] = j < M ? keysrc[(size_t)q * M + j] : 0xFFFFFFFFu;
            int nvalid = 0;
            uint32_t gBest = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu, klast = 0u;
#pragma unroll
            for (int j = 0; j < MAXM; j++) {
                if (j < M && key[j] != 0xFFFFFFFFu) {
                    nvalid++;
                    klast = key[j];
                    const uint32_t slot = si_key_index(key[j]), d = si_key_dist(key[j]);
                    if (!(sir_od_eff(slotlog[slot], (uint32_t)q) <= d)) { /* not skipped */
                        if (d <= SI_TH_LOW) atomicMin(&lister[slot], q); /* may still accept this slot */
                        if (gBest == 0xFFFFFFFFu) gBest = key[j];
                        else if (k2 == 0xFFFFFFFFu) k2 = key[j];
                    }
                }
            }
            const bool full = nvalid == M;
            const uint32_t dlast = si_key_dist(klast);
            const bool wild = full && dlast <= SI_TH_LOW; /* could accept a slot beyond its list once the list is used up */
            bool accept = false, scan = false;
            if (gBest == 0xFFFFFFFFu) {
                scan = wild; /* else: vIndices2 empty, everything skipped, or nothing within TH_LOW beyond the list */
            } else if (si_key_dist(gBest) <= SI_TH_LOW) {
                uint32_t bestDist2 = k2 == 0xFFFFFFFFu ? 0x7FFFFFFFu : si_key_dist(k2);
                if (k2 == 0xFFFFFFFFu && full) {
                    /* the second survivor lies beyond the list: it is at least as far as the last entry */
                    if ((float)(int)si_key_dist(gBest) < __fmul_rn((float)(int)dlast, nnratio)) bestDist2 = dlast; /* accepted whatever the true second is */
                    else scan = true;
                }
                if (!scan) accept = (float)(int)si_key_dist(gBest) < __fmul_rn((float)(int)bestDist2, nnratio);
            }
            kfirst[q] = gBest;
            ksecond[q] = k2;
            qstate[q] = (uint8_t)(SIR_PEND | (accept ? SIR_ACC : 0u) | (scan ? SIR_SCAN : 0u));
            atomicMin(&s_minpend[par], q);
            if (wild) atomicMin(&s_minwild[par], q);
        }
        __syncthreads();
        const int minp = s_minpend[par], minw = s_minwild[par];
        if (minp == 0x7FFFFFFF) break; /* nothing undecided (block-uniform) */
        nrounds++;
        /* ---- 2: commit what no earlier undecided query can change; reset the other round's buffers */
        {
            int32_t* other = par ? lister0 : lister1;
            for (int c = tid; c < c2; c += SIR_NT) other[c] = 0x7FFFFFFF;
            if (tid == 0) {
                s_minpend[par ^ 1] = 0x7FFFFFFF;
                s_minwild[par ^ 1] = 0x7FFFFFFF;
            }
        }
        for (int q = tid; q < c1; q += SIR_NT) {
            const uint32_t fl = qstate[q];
            if (!(fl & SIR_PEND)) continue;
            if (fl & SIR_SCAN) {
                if (q == minp) s_scanq = q; /* everything in front of it is decided: re-scan below */
                continue;
            }
            const uint32_t k1 = kfirst[q], k2 = ksecond[q];
            bool blocked = q > minw;
            if (k1 != 0xFFFFFFFFu && lister[si_key_index(k1)] < q) blocked = true;
            if (k2 != 0xFFFFFFFFu && lister[si_key_index(k2)] < q) blocked = true;
            if (blocked) continue;
            if (fl & SIR_ACC) {
                if (!sir_slot_append(slotlog, si_key_index(k1), (uint32_t)q, si_key_dist(k1), q == minp)) continue; /* slot full: wait to be first */
                alog[atomicAdd(&s_nlog, 1)] = ((uint32_t)q << 12) | si_key_index(k1);
            }
            qstate[q] = 0;
        }
        __syncthreads();
        /* ---- 3 (rare): the smallest undecided query's sorted prefix ran out -- re-scan its whole window, one wave
         * (fmatcher.cpp:1003-1035 literally); it sees the acceptances of the queries before it only */
        const int sq = s_scanq;
        if (sq >= 0) { /* block-uniform */
            if (tid < 64) {
                uint32_t d2;
                const uint32_t gb = si_full_scan(jb, gcand, slotlog, c2, lane, gqry[sq], (uint32_t)sq, r, bnd, inv, &d2);
                if (tid == 0) {
                    if (gb != 0xFFFFFFFFu && si_key_dist(gb) <= SI_TH_LOW && (float)(int)si_key_dist(gb) < __fmul_rn((float)(int)d2, nnratio)) {
                        sir_slot_append(slotlog, si_key_index(gb), (uint32_t)sq, si_key_dist(gb), true);
                        alog[atomicAdd(&s_nlog, 1)] = ((uint32_t)sq << 12) | si_key_index(gb);
                    }
                    qstate[sq] = 0;
                }
            }
            nfb++;
            __syncthreads();
        }
    }
    __syncthreads();
    const int nlog = s_nlog;
    if (fallbacks && tid == 0) { /* [0] re-scans (vslam_dbg_search_init_fallbacks), [1..3] rounds, queries, pairs */
        if (nfb) atomicAdd(fallbacks, nfb);
        atomicAdd(fallbacks + 1, nrounds);
        atomicAdd(fallbacks + 2, c1);
        atomicAdd(fallbacks + 3, 1);
    }
    /* ownership: the last acceptor of a slot (in query order) keeps it (fmatcher.cpp:1041-1049 undoes the previous owner) */
    int32_t* ownerQ = lister0;
    for (int c = tid; c < c2; c += SIR_NT) ownerQ[c] = -1;
    __syncthreads();
    for (int e = tid; e < nlog; e += SIR_NT) atomicMax(&ownerQ[alog[e] & 0xFFFu], (int)(alog[e] >> 12));
    __syncthreads();
    for (int e = tid; e < nlog; e += SIR_NT) {
        const uint32_t le = alog[e];
        const SiQuery q = gqry[le >> 12];
        const SiCand cd = gcand[le & 0xFFFu];
        if (ownerQ[le & 0xFFFu] == (int)(le >> 12)) m12[q.idx] = cd.idx;
        if (checkOri) {
            const int bin = vslam_md::rot_bin(q.angle, cd.angle, VSLAM_HISTO_LENGTH);
            rotBin[q.idx] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1); /* rotHist[bin].push_back(i1): never removed, even if stolen later */
        }
    }
    __syncthreads();
    /* nmatches is counted from vnMatches12 at the end: the reference's running count equals it */
    if (checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
        for (int i = tid; i < n1; i += SIR_NT) {
            const int b = rotBin[i];
            if (b != 255 && !vslam_md::keeps_bin(mx, b)) m12[i] = -1;
        }
        __syncthreads();
    }
    int cnt = 0;
    /* four keypoints per thread and pass: their (dependent) global loads are in flight together */
    for (int i0 = tid; i0 < n1; i0 += 4 * SIR_NT) {
        int m[4];
        float2 o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * SIR_NT;
            m[u] = i < n1 ? m12[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * SIR_NT;
            o[u] = make_float2(0.0f, 0.0f);
            if (i < n1) {
                /* vbPrevMatched update (fmatcher.cpp:1093-1095) */
                if (m[u] >= 0) o[u] = make_float2(jb.k2[m[u]].x, jb.k2[m[u]].y);
                else if (jb.prev) o[u] = make_float2(jb.prev[2 * i], jb.prev[2 * i + 1]);
                else o[u] = make_float2(jb.k1[i].x, jb.k1[i].y);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * SIR_NT;
            if (i < n1) {
                mo[i] = m[u];
                po[2 * i] = o[u].x;
                po[2 * i + 1] = o[u].y;
                cnt += m[u] >= 0;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) nmatch_out[blockIdx.x] = hdr[2] ? -1 : s_cnt; /* -1: capacity overflow (vslam_search_init_dev_wait) */
}

size_t vk_search_init_scratch_bytes(int npairs, int max_c2, int M) { return (size_t)npairs * si_pair_bytes(max_c2, M); }

static size_t si_topm_lds(int max_c2) { return (size_t)max_c2 * (sizeof(SiCand) + 4 * 4); }
/* state (37 bytes per octave-0 keypoint, 5 per keypoint) + the sorted prefixes of up to max_c2 queries if that stays within 64 KB */
static size_t si_replay_keys_lds(int max_c2, int M) {
    const size_t want = (size_t)max_c2 * M * 4;
    return want <= (64u << 10) ? want : 0;
}
static size_t si_replay_lds(int cap, int max_c2, int M = 0) {
    return (((size_t)max_c2 * 37 + (size_t)cap * 5 + 15) & ~(size_t)15) + si_replay_keys_lds(max_c2, M) + 16;
}

size_t vk_search_init_lds(int cap, int max_c2) { return std::max(si_topm_lds(max_c2), si_replay_lds(cap, max_c2)); } /* without the optional key cache */

int vk_search_init_set_max_lds(size_t bytes) {
    int rc = (int)hipFuncSetAttribute((const void*)k_si_topm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_si_replay<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    return (int)hipFuncSetAttribute((const void*)k_si_replay<SI_MAX_M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

void vk_search_init(hipStream_t st, const InitJobs& jobs, int npairs, int cap, const SiBounds& bounds, int window,
                    float nnratio, int checkOri, int32_t* matches_out, float* prev_out, int32_t* nmatch_out,
                    int max_c2, int M, uint8_t* scratch, int* fallbacks, const vslam_tuning& T) {
    if (npairs <= 0) return;
    /* queries per workgroup: every workgroup first rebuilds the pair's candidate list and finds its queries (a scan of
     * both frames' keypoints), so fewer, longer workgroups repeat less of that; VSLAM_SI_QPB = 8 | 16 | 32 for A/B runs */
    const int qv = T.si_queries_per_block;
    const int qpb = (qv == 8 || qv == 16 || qv == 32) ? qv : 16;
    const int chunks = (max_c2 + qpb - 1) / qpb;
    hipLaunchKernelGGL(k_si_topm, dim3(chunks, npairs), dim3(256), si_topm_lds(max_c2), st, jobs, cap, bounds,
                       window, max_c2, M, scratch, qpb);
    /* the key cache only if the whole allocation stays within what vk_search_init_set_max_lds allowed (150 KB) */
    int keys_lds = (int)si_replay_keys_lds(max_c2, M);
    if (si_replay_lds(cap, max_c2, M) > (150u << 10)) keys_lds = 0;
    const size_t rlds = keys_lds ? si_replay_lds(cap, max_c2, M) : si_replay_lds(cap, max_c2);
    if (M <= 8)
        hipLaunchKernelGGL(k_si_replay<8>, dim3(npairs), dim3(SIR_NT), rlds, st, jobs, cap, bounds,
                           window, nnratio, checkOri, matches_out, prev_out, nmatch_out, max_c2, M, scratch, fallbacks, keys_lds);
    else
        hipLaunchKernelGGL(k_si_replay<SI_MAX_M>, dim3(npairs), dim3(SIR_NT), rlds, st, jobs, cap, bounds,
                           window, nnratio, checkOri, matches_out, prev_out, nmatch_out, max_c2, M, scratch, fallbacks, keys_lds);
}

