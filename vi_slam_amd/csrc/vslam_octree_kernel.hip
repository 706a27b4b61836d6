/* vslam_octree_kernel.hip -- FExtractor::DistributeOctTree (fextractor.cpp:530-754) on the GPU.
 *
 * One workgroup (256, 512 or 1024 threads: vk_octree) per (image slot, pyramid level).  The reference algorithm is a sequential
 * walk over a std::list, but every pass of it splits a whole generation of nodes, and the only
 * order-dependent facts are (a) the relative order of the keys inside a node (DivideNode keeps it),
 * (b) the order of the list and (c) the "largest node first, stop at N" rule.  All three are prefix sums:
 *
 *  - a split needs only the per-child key COUNT of every expandable node; the relative order of the keys inside a
 *    node only matters for the final "first key with the maximal response" = arg-max on (response, ~position);
 *  - children are push_front'ed in creation order and survivors keep their relative order, so after a
 *    pass   list = reverse(children in creation order) ++ survivors.  Nodes are stored IN LIST ORDER and
 *    rebuilt each pass from two scans (children created before me / survivors before me);
 *  - phase 2 (fextractor.cpp:664-729) sorts the expandable nodes by (size, node address) and stops once
 *    lNodes.size() >= N: rank by counting, prefix sum of (children-1) in that order, cut where the
 *    running list size reaches N.  Heap addresses are not reproducible; the tie-break is "created later
 *    first" == smaller list index first (same rule as the CPU oracle and vslam_host.cpp).
 *
 * Integer arithmetic only, except the initial bucket index (int)(x / hX) which is an IEEE float division
 * exactly as in the reference (fextractor.cpp:560).
 */
#include "vslam_kernels.h"

#include <mutex>

#ifndef O4BATCH
#define O4BATCH 8 /* k_octree_v4: keys per thread and batch of the key walk (loads in flight per lane) */
#endif
typedef unsigned long long u64;

struct ONode { /* 16 bytes, one entry of the list */
    int16_t x0, y0, x1, y1;
    uint32_t begin; /* path code of the node (k_octree_v4) */
    uint32_t cf;    /* count << 1 | noMore */
};
#define ND_NOMORE(nd) ((nd).cf & 1u)

/* packed per-quadrant counters: quadrants 0..2 in three 21-bit fields of a u64 (up to 2M keys per level);
 * quadrant 3 is what remains of the node */
#define FB 21
#define FMASK ((1ull << FB) - 1)
__device__ __forceinline__ unsigned long long onehot(int q) { return q < 3 ? 1ull << (FB * q) : 0ull; }
__device__ __forceinline__ uint32_t fld(unsigned long long v, int q) { return (uint32_t)((v >> (FB * q)) & FMASK); }
/* number of non-empty children given the packed counts of quadrants 0..2 and the node's key count */
__device__ __forceinline__ uint32_t nchildren(unsigned long long c, uint32_t count) {
    const uint32_t c0 = fld(c, 0), c1 = fld(c, 1), c2 = fld(c, 2);
    return (c0 != 0) + (c1 != 0) + (c2 != 0) + (count - c0 - c1 - c2 != 0);
}

template <typename T, int NT>
__device__ __forceinline__ T block_excl_scan(T v, T* s_wave, T* total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    T woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
        const T x = s_wave[k];
        if (k < wv) woff += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

/* ------------------------------------------------------------------------------------------------
 * k_octree_v4: the distribution with ONE key walk, no walk per pass, and no limit on how finely keys cluster.
 *
 * DivideNode's boundaries depend on the node alone (midpoints, fextractor.cpp:474-475), never on the keys, so the
 * quadtree below an initial node is a fixed implicit tree; and because x and y are halved separately, a key's path to
 * depth D (one 2-bit quadrant per depth) is two table look-ups, path = xs[x] | ys[y] (vslam::build_oct_lut).
 *   walk    every key is read ONCE from the FAST cells' segments (position in cell order = the reference's key order);
 *           its leaf of depth D ("fine cell", nIni * 4^D of them) gets two LDS atomics: the cell's key count, and the
 *           cell's best key, a max on response << 20 | ~position (28 bits).  The key is also stored in key order.
 *           -> one prefix sum over the fine counts, in place.  A node of depth d <= D IS the contiguous run of the
 *           4^(D-d) fine cells under its path, in the prefix array and in the best keys.
 *   passes  the reference's list logic (list order, "largest first until N", creation ranks); the child counts a pass
 *           needs are four differences of the prefix array, per NODE, not per key.  A node DEEPER than the grid (keys
 *           closer together than a fine cell: real images do that on the sparse top levels, where every node is split
 *           down to single keys) lies inside one fine cell.  The first pass that meets one sorts the keys by fine cell
 *           (a second walk, over the stored keys: rank from a returning atomic, sorted[PS[cell] + rank]); the node's
 *           few keys are then enumerated from its cell's run and tested against the node's path by walking the
 *           halvings -- exact at any depth, no fallback kernel.  Most problems never sort.
 *   select  "best response, first key wins" (fextractor.cpp:732-751): four lanes per final node reduce the best keys of
 *           its cells to the winner's position, and the winners are gathered from the keys in key order; a problem
 *           that sorted reduces the node's run of the sorted keys instead (response, then original position).
 * One workgroup per (slot, level): the quadtree stays a narrow kernel that hides behind the grid-filling ones.
 * History (git): v3 kept an owner table instead of sorted keys (gather + count + owner fill + select walks, fine cell by D
 * dependent halvings per key: 52 / 89 / 251 us for the level-0 problem at KITTI N=1000 / 2000 / 1080p N=4000) and
 * handed problems whose keys cluster below the grid to the walk-per-pass code in k_assign_out -- which the reference's
 * own test images (hut_stereo 752x480) triggered on 5-30 % of their (slot, level) problems.
 * ---------------------------------------------------------------------------------------------- */
#define ND4_DEPTH(nd) ((int)((nd).cf >> 28))
#define ND4_COUNT(nd) (((nd).cf & 0x0FFFFFFFu) >> 1)

__device__ __forceinline__ uint32_t oct_key_path(uint32_t key, float hX, int nIni, int Hh, int depth) {
    const int x = key & 0xFFF, y = (key >> 12) & 0xFFF;
    int b = (int)__fdiv_rn((float)x, hX); /* initial node, fextractor.cpp:557-561 */
    b = min(b, nIni - 1);
    int x0 = (int)__fmul_rn(hX, (float)b), x1 = (int)__fmul_rn(hX, (float)(b + 1)), y0 = 0, y1 = Hh;
    uint32_t code = 0;
    for (int d = 0; d < depth; d++) { /* DivideNode: halfX = ceil((UR.x - UL.x) / 2); kp.x < n1.UR.x, kp.y < n1.BR.y */
        const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
        const int qx = x < mx ? 0 : 1, qy = y < my ? 0 : 1;
        code = (code << 2) | (uint32_t)qx | ((uint32_t)qy << 1);
        if (qx) x0 = mx; else x1 = mx;
        if (qy) y0 = my; else y1 = my;
    }
    return ((uint32_t)b << (2 * depth)) | code;
}

/* inclusive scan over a 64-cell tile, lane = cell */
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if ((int)(threadIdx.x & 63) >= o) v += t;
    }
    return v;
}

/* packed child counts of a node at or below the grid depth D: its keys are among the few of ONE fine cell's sorted run */
__device__ __forceinline__ u64 deep_child_counts(const uint2* sorted, const uint32_t* PS, uint32_t path, int depth, int D,
                                                 float hX, int nIni, int Hh) {
    u64 c = 0ull;
    const uint32_t f = path >> (2 * (depth - D));
    for (uint32_t j = PS[f]; j < PS[f + 1]; j++) {
        const uint32_t kp = oct_key_path(sorted[j].x, hX, nIni, Hh, depth + 1);
        if ((kp >> 2) == path) c += onehot((int)(kp & 3u));
    }
    return c;
}

/* the key that wins a fine cell, as one 32-bit LDS atomicMax: response, then the EARLIEST position in key order (n < 2^20) */
#define OCT_BEST(key, pos) ((((key) >> 24) << 20) | (0xFFFFFu - (uint32_t)(pos)))
#define OCT_BEST_POS(b) (0xFFFFFu - ((b) & 0xFFFFFu))

template <int OTV> /* OTV: threads of the workgroup (256 / 512 / 1024, vk_octree) */
__global__ void __launch_bounds__(OTV)
k_octree_v4(const uint8_t* __restrict__ cand_region, size_t cand_stride, int ncells, OctParams P, uint32_t* keys_a,
            uint2* sorted_a, size_t pts_stride, uint32_t* sel_xyr, int32_t* sel_cnt, int32_t* err_flag,
            int32_t* deep_flags) {
    extern __shared__ __align__(16) uint8_t osm[];
    const int MAXN = P.maxNodes;
    ONode* cur = (ONode*)osm;
    ONode* nxt = cur + MAXN;
    uint32_t* Kq = (uint32_t*)(nxt + MAXN);   /* phase 2: sort key of every node (8 bytes per node reserved, 4 used) */
    u64* Cnt = (u64*)(nxt + MAXN) + MAXN;     /* packed per-quadrant key counts of a node */
    uint16_t* cb = (uint16_t*)(Cnt + MAXN);   /* list index of a processed node's FIRST created child */
    uint16_t* newIdx = cb + MAXN;             /* unused, kept in the layout (vk_octree_lds_bytes) */
    uint16_t* prank = newIdx + MAXN;          /* processing rank of an expandable node */
    uint16_t* ordv = prank + MAXN;            /* node at processing rank r */
    __shared__ uint32_t s_w32[OTV / 64];
    __shared__ int s_size, s_M, s_nexp, s_cut, s_deep;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int level = blockIdx.y, slot = blockIdx.x;
    const int N = P.N[level];
    const uint32_t* hdr = (const uint32_t*)(cand_region + (size_t)slot * cand_stride);
    const CellOut* cout = (const CellOut*)(hdr + 2);
    const uint32_t* cand = (const uint32_t*)(cout + ncells);
    uint32_t* pa = keys_a + (size_t)slot * pts_stride;    /* the level's keys in key order */
    uint2* sorted = sorted_a + (size_t)slot * pts_stride; /* {key, position in key order}, sorted by fine cell: built on demand */
    uint32_t* out = sel_xyr + (size_t)slot * P.selStride + P.selOff[level];
    int32_t* ocnt = sel_cnt + slot * VSLAM_MAX_LEVELS + level;
    if (tid == 0) {
        deep_flags[slot * VSLAM_MAX_LEVELS + level] = 0;
        s_deep = 0;
    }
#ifdef VSLAM_OCT_STAMPS
    int dbgn3 = 0;
    unsigned long long* DBG3 = (unsigned long long*)P.dbg;
#ifndef VSLAM_OCT_STAMP_LEVEL
#define VSLAM_OCT_STAMP_LEVEL 0 /* the level of slot 0 whose workgroup is stamped */
#endif
#define STAMP3() do { if (DBG3 && tid == 0 && level == VSLAM_OCT_STAMP_LEVEL && slot == 0 && dbgn3 < 60) DBG3[dbgn3++] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define STAMP3() do { } while (0)
#endif
    STAMP3();

    /* ---- 0. this level's candidates in cell order (vToDistributeKeys, fextractor.cpp:809-817): a key's position in
     * that order is its rank in the reference's key order.  One binary search in the cells' offsets (LDS) for a lane's
     * first position, then it walks on cell by cell. */
    const int c0 = P.cellFirst[level], c1 = P.cellFirst[level + 1];
    uint32_t off0 = 0;
    if (c0 > 0) { /* keys of the levels in front of this one (level 0: none, no scan) */
        uint32_t before = 0;
        for (int c = tid; c < c0; c += OTV) before += cout[c].count;
        uint32_t tot;
        block_excl_scan<uint32_t, OTV>(before, s_w32, &tot);
        off0 = tot;
    }
    const int ncl = c1 - c0, K = (ncl + OTV - 1) / OTV;
    uint32_t mine = 0;
    for (int k = 0; k < K; k++) {
        const int c = c0 + tid * K + k;
        if (c < c1) mine += cout[c].count;
    }
    uint32_t ntot;
    uint32_t woff = block_excl_scan<uint32_t, OTV>(mine, s_w32, &ntot);
    const int n = (int)ntot;
    if (off0 + ntot > (uint32_t)P.ptsCap || n >= (1 << 20) || hdr[1] != 0) {
        if (tid == 0) {
            atomicOr(err_flag, 1);
            *ocnt = 0;
        }
        return;
    }
    pa += off0;
    sorted += off0;
    /* cell offsets (+ sentinel) and the cells' segment bases, borrowed from the node arrays (2 * ncl + 1 words; the host
     * sizes MAXN >= ncl / 4, i.e. 14 * MAXN words of node arrays): the walk needs ONE global round trip (the keys) */
    uint32_t* coff = (uint32_t*)nxt;
    uint32_t* cbas = coff + ncl + 1;
    for (int k = 0; k < K; k++) {
        const int c = c0 + tid * K + k;
        if (c < c1) {
            const CellOut co = cout[c];
            coff[c - c0] = woff;
            cbas[c - c0] = co.base;
            woff += co.count;
        }
    }
    if (tid == 0) coff[ncl] = ntot;
    if (n == 0) {
        if (tid == 0) *ocnt = 0;
        return;
    }
    const int nIni = P.nIni[level];
    const float hX = P.hX[level];
    const int Hh = P.H[level];
    const int D = P.fineD[level];
    const int cells = nIni << (2 * D);
    uint32_t* PS = (uint32_t*)(osm + P.fineLdsOff); /* key counts of the fine cells, then (in place) their exclusive prefix sums */
    uint32_t* Bst = PS + cells + 1;                 /* OCT_BEST of every fine cell; counters of the sort where it is built */
    const uint32_t* __restrict__ xs = P.lut + P.lutOff[level];
    const uint32_t* __restrict__ ys = xs + P.lutW[level];
    for (int i = tid; i <= cells; i += OTV) PS[i] = Bst[i] = 0u;
    /* the path tables are cold (another XCD's L2 or HBM) the first time a workgroup touches them: start pulling their
     * lines now, the key loads below hide the round trip */
    uint32_t warm = 0u;
    if (tid * 16 < P.lutW[level] + Hh + 1) warm = xs[tid * 16]; /* consumed (by nothing) behind the walk */
    __syncthreads();

    /* ---- 1. the ONE walk over the keys: every key is read once, counted into its fine cell, offered as the cell's best
     * key, and kept in key order (pa) for the gather of the winners and for the sort of a problem that splits below the
     * grid.  Positions are dealt to WAVES in contiguous chunks of EW (a multiple of 64) and to the lanes of a wave
     * interleaved: lane l holds positions wbeg + 64 k + l, so that a wave's loads (mostly one FAST cell segment after the
     * other) and its stores are coalesced */
    {
        const int KW = (n + OTV - 1) / OTV, EW = KW * 64; /* keys per lane, positions per wave */
        const int p0 = wv * EW + lane;
        int c = 0;
        if (p0 < n) {
            int lo = 0, hi = ncl - 1; /* last cell with coff <= p0 (empty cells share an offset: the last one holds it) */
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (coff[mid] <= (uint32_t)p0) lo = mid;
                else hi = mid - 1;
            }
            c = lo;
        }
        uint32_t cbase = p0 < n ? cbas[c] : 0u, cfirst = p0 < n ? coff[c] : 0u, cnext = p0 < n ? coff[c + 1] : 0u;
        for (int kb = 0; kb < KW; kb += O4BATCH) { /* O4BATCH loads in flight, then the table look-ups, then the atomics */
            uint32_t kk[O4BATCH], ff[O4BATCH];
#pragma unroll
            for (int j = 0; j < O4BATCH; j++) {
                const int i = p0 + 64 * (kb + j);
                kk[j] = 0u;
                if (kb + j < KW && i < n) {
                    while ((uint32_t)i >= cnext) { /* on to the cell that holds position i */
                        c++;
                        cfirst = cnext;
                        cnext = coff[c + 1];
                        cbase = cbas[c];
                    }
                    kk[j] = cand[cbase + ((uint32_t)i - cfirst)];
                }
            }
#pragma unroll
            for (int j = 0; j < O4BATCH; j++)
                ff[j] = (kb + j < KW && p0 + 64 * (kb + j) < n) ? xs[kk[j] & 0xFFF] | ys[(kk[j] >> 12) & 0xFFF] : 0u;
#pragma unroll
            for (int j = 0; j < O4BATCH; j++) {
                const int i = p0 + 64 * (kb + j);
                if (kb + j < KW && i < n) {
                    atomicAdd(&PS[ff[j]], 1u);
                    atomicMax(&Bst[ff[j]], OCT_BEST(kk[j], i));
                    pa[i] = kk[j];
                }
            }
        }
    }
    asm volatile("" ::"v"(warm));
    __syncthreads(); /* coff (in the node arrays) is free again; the counters and the best keys are complete */
    STAMP3();
    {   /* exclusive prefix sums of the fine counts, in place */
        const int ntile = (cells + 63) >> 6, tpw = (ntile + OTV / 64 - 1) / (OTV / 64); /* tiles per wave */
        const int t1 = min((wv + 1) * tpw, ntile);
        uint32_t carry = 0;
        for (int t = wv * tpw; t < t1; t++) {
            const int c = t * 64 + lane;
            const uint32_t h = c < cells ? PS[c] : 0u;
            const uint32_t inc = wave_incl_add(h);
            if (c < cells) PS[c] = carry + inc - h;
            carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if (lane == 0) s_w32[wv] = carry;
        __syncthreads();
        uint32_t wo = 0;
        for (int k = 0; k < wv; k++) wo += s_w32[k];
        if (wo)
            for (int t = wv * tpw; t < t1; t++) {
                const int c = t * 64 + lane;
                if (c < cells) PS[c] += wo;
            }
        if (tid == 0) PS[cells] = (uint32_t)n;
    }
    __syncthreads();
    STAMP3();

    /* initial nodes; ONode.begin = path code of the node (root << 2 depth | quadrants), depth in cf[31:28] */
    if (tid == 0) {
        int li = 0;
        for (int b = 0; b < nIni; b++) {
            const uint32_t cb0 = PS[(b + 1) << (2 * D)] - PS[b << (2 * D)];
            if (cb0) { /* empty initial nodes are erased (fextractor.cpp:572-573) */
                ONode nd;
                nd.x0 = (int16_t)(int)__fmul_rn(hX, (float)b);
                nd.x1 = (int16_t)(int)__fmul_rn(hX, (float)(b + 1));
                nd.y0 = 0;
                nd.y1 = (int16_t)Hh;
                nd.begin = (uint32_t)b;
                nd.cf = (cb0 << 1) | (cb0 == 1 ? 1u : 0u);
                cur[li++] = nd;
            }
        }
        s_size = li;
    }
    __syncthreads(); /* also: the keys in key order (global memory, this CU's stores) are complete for the whole workgroup */
    STAMP3();

    /* ---- 3. split passes: the reference's list logic; the children's key counts come from the prefix sums */
    int phase = 1;
    bool haveSorted = false; /* uniform: the keys sorted by fine cell exist (only a problem that splits below the grid builds them) */
    const int KN = (MAXN + OTV - 1) / OTV;
    for (int iter = 0; iter < P.maxIter; iter++) {
        const int size0 = s_size;
        /* A. children's key counts of every expandable node; phase 2 also needs every node's sort key */
        for (int k = 0; k < KN; k++) {
            const int v = tid * KN + k;
            if (v < size0) {
                const ONode nd = cur[v];
                u64 c = 0ull;
                uint32_t kq = 0u;
                if (!ND_NOMORE(nd)) {
                    const int depth = ND4_DEPTH(nd);
                    const uint32_t path = nd.begin;
                    if (depth < D) {
                        const uint32_t cb0 = path << (2 * (D - depth)), q4 = 1u << (2 * (D - depth - 1));
                        const uint32_t p0 = PS[cb0], p1 = PS[cb0 + q4], p2 = PS[cb0 + 2 * q4], p3 = PS[cb0 + 3 * q4];
                        c = (u64)(p1 - p0) | ((u64)(p2 - p1) << FB) | ((u64)(p3 - p2) << (2 * FB));
                    } else { /* finer than the grid: the node's keys are among the few of ONE fine cell */
                        s_deep = 1; /* benign race: all writers store 1, all readers wait for the barrier below */
                        if (haveSorted) c = deep_child_counts(sorted, PS, path, depth, D, hX, nIni, Hh);
                    }
                    /* descending (count, "created later" == smaller list index): one unsigned compare */
                    kq = (ND4_COUNT(nd) << 12) | (uint32_t)(4095 - v);
                }
                Cnt[v] = c;
                Kq[v] = kq;
            }
        }
        /* pad the sort keys to a multiple of four (the rank loop reads them four at a time) */
        if (tid < 4 && size0 + tid < ((size0 + 3) & ~3)) Kq[size0 + tid] = 0u;
        __syncthreads();
        if (s_deep && !haveSorted) {
            /* The first pass that meets a node below the grid sorts the keys by fine cell: {key, position} at
             * sorted[PS[cell] + rank], the rank from a returning LDS atomic on counters that take the place of the cells'
             * best keys (the select then reads the sorted runs instead).  Order inside a cell: whatever the atomics give;
             * the select decides by original position, which travels with the key.  s_deep only ever goes from 0 to 1 and
             * is written in front of the barrier above: the decision is uniform. */
            for (int i = tid; i < cells; i += OTV) Bst[i] = 0u;
            __syncthreads();
            for (int base = tid; base < n; base += O4BATCH * OTV) {
                uint32_t kk[O4BATCH], ff[O4BATCH];
#pragma unroll
                for (int j = 0; j < O4BATCH; j++) kk[j] = base + j * OTV < n ? pa[base + j * OTV] : 0u;
#pragma unroll
                for (int j = 0; j < O4BATCH; j++) ff[j] = base + j * OTV < n ? xs[kk[j] & 0xFFF] | ys[(kk[j] >> 12) & 0xFFF] : 0u;
#pragma unroll
                for (int j = 0; j < O4BATCH; j++) {
                    const int i = base + j * OTV;
                    if (i < n) sorted[PS[ff[j]] + atomicAdd(&Bst[ff[j]], 1u)] = make_uint2(kk[j], (uint32_t)i);
                }
            }
            haveSorted = true;
            __syncthreads();
            for (int k = 0; k < KN; k++) { /* the counts that step A left open */
                const int v = tid * KN + k;
                if (v < size0) {
                    const ONode nd = cur[v];
                    if (!ND_NOMORE(nd) && ND4_DEPTH(nd) >= D)
                        Cnt[v] = deep_child_counts(sorted, PS, nd.begin, ND4_DEPTH(nd), D, hX, nIni, Hh);
                }
            }
            __syncthreads();
        }
        /* D1. processing rank of every expandable node */
        uint32_t nexp_mine = 0;
        for (int k = 0; k < KN; k++) {
            const int v = tid * KN + k;
            if (v < size0 && !ND_NOMORE(cur[v])) nexp_mine++;
        }
        uint32_t nexp;
        uint32_t rbase = block_excl_scan<uint32_t, OTV>(nexp_mine, s_w32, &nexp);
        if (nexp == 0) break; /* nothing expandable: lNodes.size() == prevSize -> finish */
        if (phase == 1) {
            for (int k = 0; k < KN; k++) {
                const int v = tid * KN + k;
                if (v < size0 && !ND_NOMORE(cur[v])) {
                    prank[v] = (uint16_t)rbase;
                    ordv[rbase] = (uint16_t)v;
                    rbase++;
                }
            }
        } else {
            /* rank = number of nodes with a larger sort key (nodes that cannot be split have key 0) */
            const uint4* K4 = (const uint4*)Kq;
            const int n4 = (size0 + 3) >> 2;
            for (int k = 0; k < KN; k++) {
                const int v = tid * KN + k;
                if (v < size0 && !ND_NOMORE(cur[v])) {
                    const uint32_t kv = Kq[v];
                    uint32_t r = 0;
#pragma unroll 4
                    for (int u = 0; u < n4; u++) {
                        const uint4 q = K4[u];
                        r += (q.x > kv) + (q.y > kv) + (q.z > kv) + (q.w > kv);
                    }
                    prank[v] = (uint16_t)r;
                    ordv[r] = (uint16_t)v;
                }
            }
        }
        __syncthreads();
        /* D2. in processing order: children created before me, running list size -> cut */
        const int KE = ((int)nexp + OTV - 1) / OTV;
        uint32_t chl = 0;
        for (int k = 0; k < KE; k++) {
            const int r = tid * KE + k;
            if (r < (int)nexp) {
                const int v = ordv[r];
                chl += nchildren(Cnt[v], ND4_COUNT(cur[v]));
            }
        }
        uint32_t chtot;
        uint32_t chbase = block_excl_scan<uint32_t, OTV>(chl, s_w32, &chtot);
        if (tid == 0) s_cut = (int)nexp; /* number of processed parents */
        __syncthreads();
        {
            /* parent r is processed iff size0 + sum_{r'<r}(nch-1) < N (phase 2); phase 1: all */
            uint32_t cb_run = chbase;
            for (int k = 0; k < KE; k++) {
                const int r = tid * KE + k;
                if (r < (int)nexp) {
                    const int v = ordv[r];
                    const uint32_t nch = nchildren(Cnt[v], ND4_COUNT(cur[v]));
                    if (phase == 2 && size0 + (int)cb_run - r >= N) atomicMin(&s_cut, r);
                    cb[v] = (uint16_t)cb_run; /* children created before this parent (creation rank base) */
                    cb_run += nch;
                }
            }
        }
        __syncthreads();
        const int ncut = s_cut;
        if (tid == 0) {
            int M;
            if (ncut >= (int)nexp) M = (int)chtot;
            else M = cb[ordv[ncut]];
            s_M = M;
            s_size = size0 + M - ncut;
            s_nexp = 0;
        }
        __syncthreads();
        const int M = s_M;
        /* D3. survivors keep their relative order behind the children (created in reverse) */
        uint32_t sv = 0;
        for (int k = 0; k < KN; k++) {
            const int v = tid * KN + k;
            if (v < size0) {
                const bool processed = !ND_NOMORE(cur[v]) && prank[v] < ncut;
                if (!processed) sv++;
            }
        }
        uint32_t svtot;
        uint32_t svbase = block_excl_scan<uint32_t, OTV>(sv, s_w32, &svtot);
        int nexp_children = 0;
        for (int k = 0; k < KN; k++) {
            const int v = tid * KN + k;
            if (v >= size0) continue;
            const ONode nd = cur[v];
            const bool processed = !ND_NOMORE(nd) && prank[v] < ncut;
            if (!processed) {
                nxt[M + svbase] = nd;
                svbase++;
            } else {
                const u64 c = Cnt[v];
                const int mx = nd.x0 + ((nd.x1 - nd.x0 + 1) >> 1), my = nd.y0 + ((nd.y1 - nd.y0 + 1) >> 1);
                const uint32_t depth1 = (uint32_t)ND4_DEPTH(nd) + 1u;
                int kq = 0;
                const int first = M - 1 - (int)cb[v]; /* list index of the first created child */
                const uint32_t c3 = ND4_COUNT(nd) - fld(c, 0) - fld(c, 1) - fld(c, 2);
                for (int q = 0; q < 4; q++) {
                    const uint32_t cq = q < 3 ? fld(c, q) : c3;
                    if (!cq) continue;
                    ONode ch;
                    ch.x0 = (q & 1) ? (int16_t)mx : nd.x0;
                    ch.x1 = (q & 1) ? nd.x1 : (int16_t)mx;
                    ch.y0 = (q & 2) ? (int16_t)my : nd.y0;
                    ch.y1 = (q & 2) ? nd.y1 : (int16_t)my;
                    ch.begin = (nd.begin << 2) | (uint32_t)q;
                    ch.cf = (depth1 << 28) | (cq << 1) | (cq == 1 ? 1u : 0u);
                    nxt[first - kq] = ch;
                    if (cq > 1) nexp_children++;
                    kq++;
                }
            }
        }
        if (nexp_children) atomicAdd(&s_nexp, nexp_children);
        __syncthreads();
        { ONode* t = cur; cur = nxt; nxt = t; }
        /* F. loop control (fextractor.cpp:658-729) */
        const int size = s_size, nToExpand = s_nexp;
        __syncthreads();
        STAMP3(); /* one stamp per split pass */
        if (size >= N || size == size0) break;
        if (phase == 1 && size + nToExpand * 3 > N) phase = 2;
    }

    STAMP3();
    /* ---- 4. best response per node, first in key order wins (fextractor.cpp:732-751).  A node of depth d <= D is a run of
     * 4^(D-d) fine cells: four lanes reduce the cells' best keys (walk 1) to the winner's position, then all winners are
     * gathered from the keys in key order with independent loads.  A problem that went below the grid has the sorted
     * keys instead: four lanes per node reduce its run of them on (response, ~position). */
    const int size = s_size;
    if (!haveSorted) {
        /* A node of depth d reduces 4^(D-d) cells with four lanes: one or four cells for the nodes of a list that reached
         * its quota, but 4^D for an initial node that was never split (a list that ended early: few nodes, each a long
         * serial run of LDS reads, at most cells / 4 per lane in all).  Not dealt wider: such lists belong to the sparse
         * top levels, whose workgroups finish long before level 0's. */
        uint32_t* win = (uint32_t*)nxt; /* the list that is not current: position of every node's winner */
        for (int v0 = 0; v0 < size; v0 += OTV / 4) {
            const int v = v0 + (tid >> 2), sub = tid & 3;
            uint32_t best = 0u;
            if (v < size) {
                const ONode nd = cur[v];
                const int sh = 2 * (D - ND4_DEPTH(nd)); /* no node is deeper than the grid here */
                const uint32_t lo = nd.begin << sh, hi = (nd.begin + 1u) << sh;
                for (uint32_t j = lo + (uint32_t)sub; j < hi; j += 4) best = max(best, Bst[j]);
            }
            best = max(best, (uint32_t)__shfl_xor((int)best, 1, 64)); /* the node's four lanes are neighbours in the wave */
            best = max(best, (uint32_t)__shfl_xor((int)best, 2, 64));
            if (v < size && sub == 0) win[v] = OCT_BEST_POS(best); /* every listed node holds at least one key */
        }
        __syncthreads();
        for (int v = tid; v < size; v += OTV) out[v] = pa[win[v]];
    } else {
        for (int v0 = 0; v0 < size; v0 += OTV / 4) {
            const int v = v0 + (tid >> 2), sub = tid & 3;
            u64 best = 0ull;
            uint32_t bkey = 0u;
            if (v < size) {
                const ONode nd = cur[v];
                const int depth = ND4_DEPTH(nd);
                const uint32_t path = nd.begin;
                if (depth <= D) {
                    const uint32_t lo = PS[path << (2 * (D - depth))], hi = PS[(path + 1u) << (2 * (D - depth))];
                    for (uint32_t j0 = lo + (uint32_t)sub; j0 < hi; j0 += 16) { /* four loads in flight per lane */
                        uint2 r[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) r[u] = j0 + 4 * u < hi ? sorted[j0 + 4 * u] : make_uint2(0u, 0xFFFFFFFFu);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const u64 a = ((u64)(r[u].x >> 24) << 32) | (u64)(0xFFFFFFFFu - r[u].y);
                            if (j0 + 4 * u < hi && a >= best) { /* >=: a key of response 0 at position 0xFFFFFFFF cannot exist, so 'best == 0' means none yet */
                                best = a;
                                bkey = r[u].x;
                            }
                        }
                    }
                } else { /* a node inside one fine cell: test the cell's keys against the node's path */
                    const uint32_t f = path >> (2 * (depth - D));
                    for (uint32_t j = PS[f] + (uint32_t)sub; j < PS[f + 1]; j += 4) {
                        const uint2 r = sorted[j];
                        if (oct_key_path(r.x, hX, nIni, Hh, depth) == path) {
                            const u64 a = ((u64)(r.x >> 24) << 32) | (u64)(0xFFFFFFFFu - r.y);
                            if (a >= best) {
                                best = a;
                                bkey = r.x;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < 4; o <<= 1) { /* the node's four lanes are neighbours in the wave */
                const u64 ob = __shfl_xor(best, o, 64);
                const uint32_t ok = __shfl_xor(bkey, o, 64);
                if (ob > best) {
                    best = ob;
                    bkey = ok;
                }
            }
            if (v < size && sub == 0) out[v] = bkey; /* every listed node holds at least one key */
        }
    }
#ifdef VSLAM_OCT_STAMPS
    __syncthreads();
    STAMP3();
    if (DBG3 && tid == 0 && level == VSLAM_OCT_STAMP_LEVEL && slot == 0) DBG3[63] = dbgn3;
#endif
    if (tid == 0) {
        *ocnt = size;
        if (s_deep) deep_flags[slot * VSLAM_MAX_LEVELS + level] = 1;
    }
}

/* ------------------------------------------------------------------------------------------------
 * output order of a slot (fextractor.cpp:1071-1129): level-major; a keypoint whose scaled x lies in
 * [lap0, lap1] takes the next free index from the tail, the others from the head.  One workgroup per
 * slot; writes the SelKp list the orientation/descriptor kernel consumes and the slot's counts.
 * ---------------------------------------------------------------------------------------------- */
#define AO_T 256 /* a small workgroup finds a free CU slot quickly next to the other streams' kernels */
__global__ void __launch_bounds__(AO_T)
k_assign_out(OctParams P, PyramidGeom g, uint32_t* sel_xyr, int32_t* sel_cnt,
             int lap0, int lap1, SelKp* sel, int32_t* slot_counts /* [slot][4]: n, mono, deep-level mask, 0 */, int cap,
             int32_t* err_flag, const int32_t* deep_flags) {
    __shared__ uint32_t s_w32[AO_T / 64];
    __shared__ int s_lvl_off[VSLAM_MAX_LEVELS + 1];
    const int tid = threadIdx.x, slot = blockIdx.x;
    const int L = g.nlevels;
    uint32_t redo_mask = 0; /* levels of this slot on which k_octree_v4 split nodes finer than its grid (vslam_fe_octree_stats) */
    if (deep_flags && tid == 0)
        for (int lv = 0; lv < L; lv++) redo_mask |= deep_flags[slot * VSLAM_MAX_LEVELS + lv] ? 1u << lv : 0u;
    if (tid == 0) {
        int acc = 0;
        for (int l = 0; l < L; l++) {
            s_lvl_off[l] = acc;
            acc += sel_cnt[slot * VSLAM_MAX_LEVELS + l];
        }
        s_lvl_off[L] = acc;
    }
    __syncthreads();
    const int nk = s_lvl_off[L];
    if (nk > cap) {
        if (tid == 0) {
            atomicOr(err_flag, 2);
            slot_counts[slot * 4] = 0;
            slot_counts[slot * 4 + 1] = 0;
            slot_counts[slot * 4 + 2] = (int32_t)redo_mask;
        }
        return;
    }
    const int Cc = (nk + AO_T - 1) / AO_T;
    const int i0 = min(tid * Cc, nk), i1 = min(i0 + Cc, nk);
    const uint32_t* base = sel_xyr + (size_t)slot * P.selStride;
    uint32_t lapc = 0;
    int l = 0;
    for (int i = i0; i < i1; i++) {
        while (i >= s_lvl_off[l + 1]) l++;
        const uint32_t p = base[P.selOff[l] + (i - s_lvl_off[l])];
        float px = (float)((int)(p & 0xFFF) + VSLAM_BORDER);
        if (l) px = __fmul_rn(px, g.lv[l].scale);
        lapc += (px >= (float)lap0 && px <= (float)lap1) ? 1u : 0u;
    }
    uint32_t laptot;
    uint32_t lapbefore = block_excl_scan<uint32_t, AO_T>(lapc, s_w32, &laptot);
    l = 0;
    for (int i = i0; i < i1; i++) {
        while (i >= s_lvl_off[l + 1]) l++;
        const uint32_t p = base[P.selOff[l] + (i - s_lvl_off[l])];
        const int lx = (int)(p & 0xFFF) + VSLAM_BORDER, ly = (int)((p >> 12) & 0xFFF) + VSLAM_BORDER;
        float px = (float)lx;
        if (l) px = __fmul_rn(px, g.lv[l].scale);
        const bool inlap = px >= (float)lap0 && px <= (float)lap1;
        SelKp k;
        k.x = (uint16_t)lx;
        k.y = (uint16_t)ly;
        k.level = (uint8_t)l;
        k.slot = (uint8_t)slot;
        k.response = (uint8_t)(p >> 24);
        k.pad = 0;
        k.out = inlap ? (uint32_t)(nk - 1 - (int)lapbefore) : (uint32_t)(i - (int)lapbefore);
        if (inlap) lapbefore++;
        sel[(size_t)slot * cap + i] = k;
    }
    if (tid == 0) {
        slot_counts[slot * 4] = nk;
        slot_counts[slot * 4 + 1] = nk - (int)laptot; /* monoIndex */
        slot_counts[slot * 4 + 2] = (int32_t)redo_mask;
    }
}

/* k_octree_v4's node arrays: cur, nxt, Kq (8 bytes reserved), Cnt, cb, newIdx, prank, ordv.  newIdx and the second half of
 * Kq are unused; they stay in the layout because the kernel's occupancy and the host's fine-depth choice under the LDS
 * budget were measured with them (shrinking them is a change of its own, to be measured) */
size_t vk_octree_lds_bytes(int maxNodes) { return (size_t)maxNodes * (16 + 16 + 8 + 8 + 2 + 2 + 2 + 2) + 64; }

void vk_octree(hipStream_t st, const uint8_t* cand_region, size_t cand_stride, int ncells, const OctParams& P,
               uint32_t* keys_a, void* sorted_a, size_t pts_stride,
               uint32_t* sel_xyr, int32_t* sel_cnt, int32_t* err_flag, int nlevels, int nslots, int32_t* deep_flags,
               int regkeys /* vslam_tuning.oct_regkeys: -1 by batch size, 0 | 1 forced */, int threads /* 256 | 512 | 1024 */) {
    const dim3 grid(nslots, nlevels);
    /* oct_regkeys is a deprecated alias: it used to keep the keys in registers between two walks, in a 1024-thread
     * workgroup.  There is one walk now and nothing to keep; 1 means what oct_threads = 1024 means, 0 and -1 leave the
     * choice to oct_threads (whose default is 1024 for one or two images, where latency is what counts). */
    const bool rk = regkeys < 0 ? nslots <= 2 : regkeys == 1;
    const size_t lds = (size_t)P.fineLdsOff + (size_t)P.fineLdsBytes;
    /* Threads per problem.  1024 finish a single frame's level-0 problem soonest; in a
     * batch every (slot, level) problem has a workgroup of its own anyway, and a SMALL workgroup leaves the CU's wave
     * slots and issue cycles to the other contexts' kernels: 256 instead of 1024 threads is +4 % mono, +7 % stereo,
     * +13 % mono at 2000 features in the pipeline (measured with the two-walk kernel).  1080p, with 65 k keys on level 0,
     * wanted 512 then (+2 %); with one walk 512 alone is the shortest stage and LOSES 4 % in the pipeline against the
     * two-walk kernel, while 256 gains 3-5 % (profiles/octree_critical_path_ab.txt): 256 for every batch. */
    const int th = rk ? 1024 : (threads == 256 || threads == 512) ? threads : 1024;
#define OCT4_LAUNCH(TH)                                                                                          \
    hipLaunchKernelGGL((k_octree_v4<TH>), grid, dim3(TH), lds, st, cand_region, cand_stride, ncells, P, keys_a, \
                       (uint2*)sorted_a, pts_stride, sel_xyr, sel_cnt, err_flag, deep_flags)
    if (th == 256) OCT4_LAUNCH(256);
    else if (th == 512) OCT4_LAUNCH(512);
    else OCT4_LAUNCH(1024);
#undef OCT4_LAUNCH
}

void vk_assign_out(hipStream_t st, const OctParams& P, const PyramidGeom& g, uint32_t* sel_xyr, int32_t* sel_cnt, int lap0,
                   int lap1, SelKp* sel, int32_t* slot_counts, int cap, int32_t* err_flag, int nslots,
                   const int32_t* deep_flags) {
    hipLaunchKernelGGL(k_assign_out, dim3(nslots), dim3(AO_T), 0, st, P, g, sel_xyr, sel_cnt, lap0, lap1, sel,
                       slot_counts, cap, err_flag, deep_flags);
}

/* hipFuncAttributeMaxDynamicSharedMemorySize is a property of the FUNCTION, shared by every context of the process: only
 * ever raise it (a small context created after a large one must not lower the limit the large one launches with) */
int vk_octree_set_max_lds(size_t bytes) {
    /* ... and of the DEVICE: hipFuncSetAttribute acts on the current device, so the raised limit is remembered per
     * device (a context on device 1 created after one on device 0 must set it again) */
    static std::mutex mu;
    static size_t have_dev[64] = {0};
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return (int)hipErrorInvalidDevice;
    size_t& have = have_dev[dev];
    if (bytes <= have) return 0;
    const void* fns[3] = {(const void*)k_octree_v4<1024>, (const void*)k_octree_v4<512>, (const void*)k_octree_v4<256>};
    for (int i = 0; i < 3; i++) {
        const int rc = (int)hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (rc) return rc;
    }
    have = bytes;
    return 0;
}
