/* vslam_voc_train.hip -- DBoW3::Vocabulary::create (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp:157-571) on the device.
 *
 * The tree is built level by level.  `perm` holds the feature indices; every node of the level owns a contiguous
 * segment of it in ascending feature order (the order the reference's groups keep, which the seeding depends on), and
 * nodeOf[position] names the node (-1: the position belongs to a finished leaf).  All nodes of a level go through each
 * kernel together, so the number of launches and of host waits per level depends on k and on the Lloyd passes, never
 * on how many nodes the level has:
 *   seeding   k_seed_pick(0) draws the first centre; then per round r = 1..k-1 k_seed_dist (distance to the newest
 *             centre, the guarded min update, an inclusive scan of min_dists inside each 256-position chunk),
 *             k_chunk_scan (exclusive scan of the chunk sums) and k_seed_pick(r): one LANE per node takes dist_sum as a
 *             difference of two global prefixes, computes cut_d and finds the first prefix >= cut_d by binary search
 *             (prefixes are non-decreasing integers).  A node of 20 features costs a lane, a node of a million too.
 *   Lloyd     k_assign (one lane per feature; the centres come from LDS when the whole workgroup sits in one node),
 *             k_mean_count + k_mean_majority from the second pass on, k_lloyd_check (one lane per node) which freezes
 *             the nodes whose association repeated and raises one word the host reads: "is any node still moving".
 *   partition k_part_hist / k_part_scan / k_part_childoff / k_part_scatter: a stable split of every segment by cluster.
 * Sums are integers throughout (min_dists <= 256, N <= 2^24), so no order of summation can change a result. */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "vslam_mem.h"
#include "vslam_voc_train.h"

using namespace vslam_vt;

int vslam_bow_descend_words(const vslam_voc* v, const uint8_t* dev_desc, int n, int32_t* dev_word, double* dev_weight,
                            int32_t* dev_nid, hipStream_t stream); /* vslam_bow.hip */

namespace {

constexpr int kChunk = 256;      /* positions per workgroup of the seeding, assign and partition kernels */
constexpr int kMeanChunk = 1024; /* positions per workgroup of k_mean_count */
constexpr int kCountStride = 260; /* 256 bit counts, the group size, padding to 16 bytes */

enum : int32_t { F_SMALL = 1, F_SEED_STOP = 2, F_DONE = 4, F_HIT = 8 };

struct NodeDev {
    int32_t off, cnt;
    uint64_t key;
    uint32_t draws;
    int32_t nclus, flags, moving, passes;
    int32_t cidx; /* row of the count table (k-means nodes only) */
    int32_t pad[2];
};
static_assert(sizeof(NodeDev) == 48, "NodeDev layout");

struct StatsDev {
    unsigned long long redraws, empty_groups;
    int32_t early_stops, hit_max_iter, any_moving, pad;
};

struct Args {
    const uint4* desc; /* N x 2 */
    int32_t N, k, nnodes, nkm, max_iter;
    uint32_t mask;
    int32_t nchunks;
    int32_t *perm, *nodeOf, *perm2, *nodeOf2;
    NodeDev* nodes;
    const int32_t* kmNodes; /* k-means nodes of the level, by cidx */
    uint8_t* assoc;
    uint32_t *minD, *pre;
    uint32_t* chunkSum;
    unsigned long long* chunkBase;
    uint4* cent;      /* nnodes x k x 2 */
    uint32_t* counts; /* nkm x k x kCountStride */
    uint32_t* gsz;    /* nnodes x k: group sizes */
    int32_t* choff;   /* nnodes x k: first position of every child segment */
    uint32_t *tailH, *tailP; /* nchunks x k, (nchunks + 1) x k */
    const int32_t* nextIdx;  /* nnodes x k: node of the next level, or -1 */
    StatsDev* st;
};

__device__ __forceinline__ uint32_t ham(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

/* inclusive scan over the 256 lanes of a workgroup; *total = sum of all */
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t* total) {
    __shared__ uint32_t waveSum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) waveSum[w] = v;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = waveSum[i];
        if (i < w) base += s;
        all += s;
    }
    *total = all;
    __syncthreads();
    return v + base;
}

/* associations of the nodes with n <= k: one cluster per feature, in order (:248-258) */
__global__ void __launch_bounds__(kChunk) k_level_init(Args A) {
    const int i = blockIdx.x * kChunk + threadIdx.x;
    if (i >= A.N) return;
    const int n = A.nodeOf[i];
    if (n < 0) return;
    const NodeDev& nd = A.nodes[n];
    if (nd.cnt <= A.k) A.assoc[i] = (uint8_t)(i - nd.off);
}

__global__ void __launch_bounds__(kChunk) k_seed_dist(Args A, int r) {
    const int i = blockIdx.x * kChunk + threadIdx.x;
    uint32_t v = 0;
    if (i < A.N) {
        const int n = A.nodeOf[i];
        if (n >= 0) {
            const NodeDev& nd = A.nodes[n];
            if (!(nd.flags & (F_SMALL | F_SEED_STOP)) && nd.nclus == r) {
                const int f = A.perm[i];
                const uint4* c = A.cent + ((size_t)n * A.k + (r - 1)) * 2;
                const uint32_t d = ham(A.desc[(size_t)f * 2], A.desc[(size_t)f * 2 + 1], c[0], c[1]);
                uint32_t m = d; /* r == 1: the initial distances (:441-444); the update against the same centre changes nothing */
                if (r > 1) {
                    m = A.minD[i];
                    if (m > 0 && d < m) m = d; /* :452-456 */
                }
                A.minD[i] = m;
                v = m;
            }
        }
    }
    uint32_t total;
    const uint32_t incl = block_scan_256(v, &total);
    if (i < A.N) A.pre[i] = incl;
    if (threadIdx.x == 0) A.chunkSum[blockIdx.x] = total;
}

/* chunkBase[c] = sum of chunkSum[0..c): one workgroup, tiles of 256 with a running carry */
__global__ void __launch_bounds__(kChunk) k_chunk_scan(Args A) {
    unsigned long long carry = 0;
    for (int base = 0; base < A.nchunks; base += kChunk) {
        const int c = base + threadIdx.x;
        const uint32_t v = c < A.nchunks ? A.chunkSum[c] : 0u; /* <= 65536 each: a tile's sum fits 32 bits */
        uint32_t total;
        const uint32_t incl = block_scan_256(v, &total);
        if (c < A.nchunks) A.chunkBase[c] = carry + (incl - v);
        carry += total;
    }
}

__device__ __forceinline__ void copy_desc(uint4* dst, const uint4* desc, int f) {
    dst[0] = desc[(size_t)f * 2];
    dst[1] = desc[(size_t)f * 2 + 1];
}

/* one lane per node.  r == 0: the first centre (:433-436), or the clusters of a node with n <= k.  r >= 1: dist_sum,
 * cut_d and the pick of centre r (:460-485) */
__global__ void __launch_bounds__(64) k_seed_pick(Args A, int r) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= A.nnodes) return;
    NodeDev nd = A.nodes[n];
    uint4* cent = A.cent + (size_t)n * A.k * 2;
    if (r == 0) {
        if (nd.cnt <= A.k) {
            for (int c = 0; c < nd.cnt; c++) copy_desc(cent + c * 2, A.desc, A.perm[nd.off + c]);
            nd.nclus = nd.cnt;
            nd.flags = F_SMALL | F_DONE;
        } else {
            const uint32_t first = vslamvoc_draw(nd.key, 0, A.mask) % (uint32_t)nd.cnt;
            copy_desc(cent, A.desc, A.perm[nd.off + (int)first]);
            nd.nclus = 1;
            nd.draws = 1;
        }
        A.nodes[n] = nd;
        return;
    }
    if ((nd.flags & (F_SMALL | F_SEED_STOP)) || nd.nclus != r) return;
    auto G = [&](int i) { return A.chunkBase[i / kChunk] + A.pre[i]; }; /* inclusive prefix over all positions */
    const unsigned long long g0 = nd.off > 0 ? G(nd.off - 1) : 0ull;
    const int last = nd.off + nd.cnt - 1;
    const unsigned long long sum = G(last) - g0;
    if (sum == 0) { /* :486-487 */
        A.nodes[n].flags = nd.flags | F_SEED_STOP;
        atomicAdd(&A.st->early_stops, 1);
        return;
    }
    uint32_t redraws = 0;
    const double cut_d = next_cut(nd.key, &nd.draws, A.mask, sum, &redraws);
    if (redraws) atomicAdd(&A.st->redraws, (unsigned long long)redraws);
    int lo = nd.off, hi = last; /* first position whose running sum is >= cut_d; the last one if none (:472-481) */
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((double)(G(mid) - g0) >= cut_d) hi = mid;
        else lo = mid + 1;
    }
    copy_desc(cent + nd.nclus * 2, A.desc, A.perm[lo]);
    A.nodes[n].draws = nd.draws;
    A.nodes[n].nclus = nd.nclus + 1;
}

/* :307-326: nearest centre by strict <, the lowest cluster wins a tie */
__global__ void __launch_bounds__(kChunk) k_assign(Args A, int first) {
    __shared__ uint4 sc[kMaxK * 2];
    const int base = blockIdx.x * kChunk;
    const int i = base + threadIdx.x;
    const int nFirst = A.nodeOf[base], nLast = A.nodeOf[min(base + kChunk, A.N) - 1];
    const bool uniform = nFirst >= 0 && nFirst == nLast; /* segments are contiguous: the whole workgroup is in one node */
    if (uniform) {
        const NodeDev& nd = A.nodes[nFirst];
        if (nd.flags & F_DONE) return;
        const uint4* c = A.cent + (size_t)nFirst * A.k * 2;
        for (int e = threadIdx.x; e < nd.nclus * 2; e += kChunk) sc[e] = c[e];
        __syncthreads();
    }
    if (i >= A.N) return;
    const int n = A.nodeOf[i];
    if (n < 0) return;
    const NodeDev& nd = A.nodes[n];
    if (nd.flags & F_DONE) return;
    const int f = A.perm[i];
    const uint4 a0 = A.desc[(size_t)f * 2], a1 = A.desc[(size_t)f * 2 + 1];
    const uint4* c = uniform ? sc : A.cent + (size_t)n * A.k * 2;
    uint32_t best = 0xffffffffu;
    const int nc = nd.nclus;
    for (int j = 0; j < nc; j++) best = min(best, (ham(a0, a1, c[j * 2], c[j * 2 + 1]) << 8) | (uint32_t)j);
    const uint8_t ic = (uint8_t)(best & 0xffu);
    if (!first && A.assoc[i] != ic) A.nodes[n].moving = 1; /* every writer stores the same value */
    A.assoc[i] = ic;
}

/* one lane per node, after every assign pass: :331-354 and the max_iter bound */
__global__ void __launch_bounds__(64) k_lloyd_check(Args A, int first) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= A.nnodes) return;
    NodeDev& nd = A.nodes[n];
    if (nd.flags & F_DONE) return;
    const int passes = ++nd.passes;
    if (!first && !nd.moving) {
        nd.flags |= F_DONE;
    } else if (passes >= A.max_iter) {
        nd.flags |= F_DONE | F_HIT;
        atomicAdd(&A.st->hit_max_iter, 1);
    } else {
        A.st->any_moving = 1;
    }
    nd.moving = 0;
}

/* DescManip::meanValue, first half: the 256 bit counts and the size of every (node, cluster) group.  A workgroup takes
 * 1024 positions.  When they all lie in one node the counts are gathered in LDS first -- two 16-bit counters per word, a
 * counter cannot pass 1024 -- and only the non-zero ones go to HBM; otherwise (many small nodes under one workgroup)
 * every set bit is one integer atomic in HBM.  Integer adds commute: the order of arrival cannot change a count. */
__global__ void __launch_bounds__(256) k_mean_count(Args A) {
    __shared__ uint32_t lc[kMaxK * 128];
    __shared__ uint32_t ls[kMaxK];
    const int base = blockIdx.x * kMeanChunk;
    const int end = min(base + kMeanChunk, A.N);
    const int nFirst = A.nodeOf[base], nLast = A.nodeOf[end - 1];
    if (nFirst >= 0 && nFirst == nLast) {
        const NodeDev& nd = A.nodes[nFirst];
        if (nd.flags & F_DONE) return;
        const int nc = nd.nclus;
        for (int e = threadIdx.x; e < nc * 128; e += 256) lc[e] = 0;
        if (threadIdx.x < nc) ls[threadIdx.x] = 0;
        __syncthreads();
        for (int i = base + threadIdx.x; i < end; i += 256) {
            const int f = A.perm[i];
            const int c = A.assoc[i];
            const uint4 a0 = A.desc[(size_t)f * 2], a1 = A.desc[(size_t)f * 2 + 1];
            const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            atomicAdd(&ls[c], 1u);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                uint32_t x = w[q];
                while (x) {
                    const int b = __ffs((int)x) - 1 + q * 32;
                    x &= x - 1;
                    atomicAdd(&lc[c * 128 + (b >> 1)], 1u << (16 * (b & 1)));
                }
            }
        }
        __syncthreads();
        uint32_t* rows = A.counts + (size_t)nd.cidx * A.k * kCountStride;
        for (int e = threadIdx.x; e < nc * 128; e += 256) {
            const uint32_t v = lc[e];
            uint32_t* row = rows + (size_t)(e >> 7) * kCountStride + (e & 127) * 2;
            if (v & 0xffffu) atomicAdd(row, v & 0xffffu);
            if (v >> 16) atomicAdd(row + 1, v >> 16);
        }
        if (threadIdx.x < nc && ls[threadIdx.x]) atomicAdd(rows + (size_t)threadIdx.x * kCountStride + 256, ls[threadIdx.x]);
        return;
    }
    for (int i = base + threadIdx.x; i < end; i += 256) {
        const int n = A.nodeOf[i];
        if (n < 0) continue;
        const NodeDev& nd = A.nodes[n];
        if (nd.flags & F_DONE) continue;
        const int f = A.perm[i];
        const uint4 a0 = A.desc[(size_t)f * 2], a1 = A.desc[(size_t)f * 2 + 1];
        const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        uint32_t* row = A.counts + ((size_t)nd.cidx * A.k + A.assoc[i]) * kCountStride;
        atomicAdd(row + 256, 1u);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint32_t x = w[q];
            while (x) {
                const int b = __ffs((int)x) - 1 + q * 32;
                x &= x - 1;
                atomicAdd(row + b, 1u);
            }
        }
    }
}

/* DescManip::meanValue, second half: one lane per (k-means node, cluster, dword).  An empty group leaves its centre */
__global__ void __launch_bounds__(256) k_mean_majority(Args A) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int w = (int)(t & 7);
    const size_t g = t >> 3;
    if (g >= (size_t)A.nkm * A.k) return;
    const int ci = (int)(g / A.k), c = (int)(g % A.k);
    const int n = A.kmNodes[ci];
    const NodeDev& nd = A.nodes[n];
    if ((nd.flags & F_DONE) || c >= nd.nclus) return;
    const uint32_t* row = A.counts + g * kCountStride;
    const uint32_t size = row[256];
    if (size == 0) {
        if (w == 0) atomicAdd(&A.st->empty_groups, 1ull);
        return;
    }
    const uint32_t th = majority_threshold(size);
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 32; q += 4) {
        const uint4 x = *(const uint4*)(row + w * 32 + q);
        v |= (uint32_t)(x.x >= th) << q | (uint32_t)(x.y >= th) << (q + 1) | (uint32_t)(x.z >= th) << (q + 2) |
             (uint32_t)(x.w >= th) << (q + 3);
    }
    ((uint32_t*)(A.cent + ((size_t)n * A.k + c) * 2))[w] = v;
}

/* group sizes of every node, and per chunk the histogram of the positions that lie in the chunk's LAST node: for a node
 * that runs on into later chunks these are exactly its positions here */
__global__ void __launch_bounds__(kChunk) k_part_hist(Args A) {
    __shared__ uint32_t hist[kMaxK];
    const int base = blockIdx.x * kChunk;
    const int i = base + threadIdx.x;
    const int nTail = A.nodeOf[min(base + kChunk, A.N) - 1];
    if (threadIdx.x < kMaxK) hist[threadIdx.x] = 0;
    __syncthreads();
    if (i < A.N) {
        const int n = A.nodeOf[i];
        if (n >= 0) {
            const int c = min((int)A.assoc[i], A.k - 1); /* always < nclus <= k; the clamp only keeps the index in the row */
            atomicAdd(&A.gsz[(size_t)n * A.k + c], 1u);
            if (n == nTail) atomicAdd(&hist[c], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < A.k) A.tailH[(size_t)blockIdx.x * A.k + threadIdx.x] = hist[threadIdx.x];
}

/* tailP[q][c] = sum of tailH[0..q)[c]: one lane per cluster */
__global__ void __launch_bounds__(64) k_part_scan(Args A) {
    const int c = threadIdx.x;
    if (c >= A.k) return;
    uint32_t run = 0;
    for (int q = 0; q < A.nchunks; q++) {
        A.tailP[(size_t)q * A.k + c] = run;
        run += A.tailH[(size_t)q * A.k + c];
    }
    A.tailP[(size_t)A.nchunks * A.k + c] = run;
}

__global__ void __launch_bounds__(64) k_part_childoff(Args A) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= A.nnodes) return;
    const NodeDev& nd = A.nodes[n];
    int run = nd.off;
    for (int c = 0; c < nd.nclus; c++) {
        A.choff[(size_t)n * A.k + c] = run;
        run += (int)A.gsz[(size_t)n * A.k + c];
    }
}

/* stable split: the rank of a position inside its (node, cluster) group = the group's members in the node's earlier
 * chunks (a difference of two scanned tail histograms) + those before it in this chunk */
__global__ void __launch_bounds__(kChunk) k_part_scatter(Args A) {
    __shared__ uint32_t keys[kChunk];
    const int i = blockIdx.x * kChunk + threadIdx.x;
    int n = -1, c = 0;
    if (i < A.N) {
        n = A.nodeOf[i];
        if (n >= 0) c = min((int)A.assoc[i], A.k - 1);
    }
    const uint32_t key = n >= 0 ? ((uint32_t)n << 6 | (uint32_t)c) : 0xffffffffu;
    keys[threadIdx.x] = key;
    __syncthreads();
    if (n < 0) return;
    uint32_t rank = 0;
    for (int j = 0; j < (int)threadIdx.x; j++) rank += keys[j] == key;
    const int q0 = A.nodes[n].off / kChunk;
    if ((int)blockIdx.x > q0) rank += A.tailP[(size_t)blockIdx.x * A.k + c] - A.tailP[(size_t)q0 * A.k + c];
    const size_t slot = (size_t)n * A.k + c;
    const uint32_t dest = (uint32_t)A.choff[slot] + rank;
    if (dest >= (uint32_t)A.N || rank >= A.gsz[slot]) return; /* cannot happen with consistent counts; never write outside */
    A.perm2[dest] = A.perm[i];
    A.nodeOf2[dest] = A.nextIdx[slot];
}

__global__ void __launch_bounds__(kChunk) k_iota(int32_t* p, int n) {
    const int i = blockIdx.x * kChunk + threadIdx.x;
    if (i < n) p[i] = i;
}

/* ms of a phase: event pairs recorded around its launches, read at the next host wait */
struct PhaseClock {
    hipStream_t stream = nullptr;
    struct Span {
        hipEvent_t a, b;
        int phase;
    };
    std::vector<Span> pending;
    std::vector<hipEvent_t> spare;
    float ms[5] = {0, 0, 0, 0, 0};
    int open = -1;
    hipEvent_t get() {
        if (!spare.empty()) {
            hipEvent_t e = spare.back();
            spare.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(int phase) {
        Span s{get(), get(), phase};
        (void)hipEventRecord(s.a, stream);
        pending.push_back(s);
        open = phase;
    }
    void end() {
        (void)hipEventRecord(pending.back().b, stream);
        open = -1;
    }
    void collect() { /* after a stream synchronisation */
        for (Span& s : pending) {
            float t = 0;
            if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) ms[s.phase] += t;
            spare.push_back(s.a), spare.push_back(s.b);
        }
        pending.clear();
    }
    ~PhaseClock() {
        for (Span& s : pending) spare.push_back(s.a), spare.push_back(s.b);
        for (hipEvent_t e : spare) (void)hipEventDestroy(e);
    }
};
enum { PH_SEED, PH_ASSIGN, PH_MEAN, PH_PART, PH_WEIGHTS };

struct StreamOwner {
    hipStream_t s = nullptr;
    ~StreamOwner() {
        if (s) (void)hipStreamDestroy(s);
    }
};

struct LevelNode {
    int32_t off, cnt;
    uint64_t key;
    int tree; /* index into the host tree */
};

int train(int device, const vslam_voc_train_params& p, const uint8_t* desc, int desc_location, const int64_t* doc_offsets,
          int n_docs, int64_t n64, vslam_voc_file** out, vslam_voc_train_stats* stats) {
    const int N = (int)n64, k = p.k;
    HIPCHK(hipSetDevice(device));
    StreamOwner so;
    HIPCHK(hipStreamCreateWithFlags(&so.s, hipStreamNonBlocking));
    hipStream_t stream = so.s;
    PhaseClock clock;
    clock.stream = stream;
    vslam_event evAll0, evAll1;
    int rc;
    if ((rc = evAll0.ensure()) || (rc = evAll1.ensure())) return rc;
    HIPCHK(hipEventRecord(evAll0, stream));

    vslam_dbuf<uint8_t> dDescOwn, dAssoc;
    const uint8_t* dDesc = desc;
    if (desc_location != VSLAM_IMGS_DEVICE) {
        if ((rc = dDescOwn.alloc((size_t)N * 32))) return rc;
        HIPCHK(hipMemcpyAsync(dDescOwn.get(), desc, (size_t)N * 32, hipMemcpyHostToDevice, stream));
        dDesc = dDescOwn.get();
    }
    const int nchunks = (N + kChunk - 1) / kChunk;
    vslam_dbuf<int32_t> dPerm, dPerm2, dNodeOf, dNodeOf2, dKm, dChoff, dNextIdx;
    vslam_dbuf<uint32_t> dMinD, dPre, dChunkSum, dCounts, dGsz, dTailH, dTailP;
    vslam_dbuf<unsigned long long> dChunkBase;
    vslam_dbuf<NodeDev> dNodes;
    vslam_dbuf<uint4> dCent;
    vslam_dbuf<StatsDev> dSt;
    if ((rc = dPerm.alloc(N)) || (rc = dPerm2.alloc(N)) || (rc = dNodeOf.alloc(N)) || (rc = dNodeOf2.alloc(N)) ||
        (rc = dAssoc.alloc(N)) || (rc = dMinD.alloc(N)) || (rc = dPre.alloc(N)) || (rc = dChunkSum.alloc(nchunks)) ||
        (rc = dChunkBase.alloc(nchunks)) || (rc = dTailH.alloc((size_t)nchunks * k)) ||
        (rc = dTailP.alloc((size_t)(nchunks + 1) * k)) || (rc = dSt.alloc(1)))
        return rc;
    HIPCHK(hipMemsetAsync(dSt.get(), 0, sizeof(StatsDev), stream));
    HIPCHK(hipMemsetAsync(dNodeOf.get(), 0, (size_t)N * 4, stream)); /* level 1: every position is in node 0, the root's step */
    hipLaunchKernelGGL(k_iota, dim3(nchunks), dim3(kChunk), 0, stream, dPerm.get(), N);

    std::vector<TreeNode> tree(1);
    std::vector<LevelNode> level(1, LevelNode{0, N, vslamvoc_mix(p.seed), 0});
    vslam_voc_train_stats st;
    memset(&st, 0, sizeof(st));
    std::vector<NodeDev> hNodes;
    std::vector<int32_t> hKm, hNext;
    std::vector<uint32_t> hGsz;
    std::vector<uint8_t> hCent;

    for (int lev = 1; lev <= p.L && !level.empty(); lev++) {
        const int nn = (int)level.size();
        hNodes.assign(nn, NodeDev{});
        hKm.clear();
        for (int n = 0; n < nn; n++) {
            hNodes[n].off = level[n].off, hNodes[n].cnt = level[n].cnt, hNodes[n].key = level[n].key;
            hNodes[n].cidx = -1;
            if (level[n].cnt > k) {
                hNodes[n].cidx = (int32_t)hKm.size();
                hKm.push_back(n);
            } else {
                st.small_nodes++;
            }
        }
        const int nkm = (int)hKm.size();
        const size_t slots = (size_t)nn * k;
        if ((rc = dNodes.ensure(nn)) || (rc = dCent.ensure(slots * 2)) || (rc = dGsz.ensure(slots)) ||
            (rc = dChoff.ensure(slots)) || (rc = dNextIdx.ensure(slots)) || (rc = dKm.ensure(std::max(nkm, 1))) ||
            (rc = dCounts.ensure(std::max<size_t>((size_t)nkm * k * kCountStride, 1))))
            return rc;
        HIPCHK(hipMemcpyAsync(dNodes.get(), hNodes.data(), (size_t)nn * sizeof(NodeDev), hipMemcpyHostToDevice, stream));
        if (nkm) HIPCHK(hipMemcpyAsync(dKm.get(), hKm.data(), (size_t)nkm * 4, hipMemcpyHostToDevice, stream));
        Args A;
        memset(&A, 0, sizeof(A));
        A.desc = (const uint4*)dDesc, A.N = N, A.k = k, A.nnodes = nn, A.nkm = nkm, A.max_iter = p.max_iter, A.mask = p.rand_mask;
        A.nchunks = nchunks, A.perm = dPerm, A.nodeOf = dNodeOf, A.perm2 = dPerm2, A.nodeOf2 = dNodeOf2, A.nodes = dNodes;
        A.kmNodes = dKm, A.assoc = dAssoc, A.minD = dMinD, A.pre = dPre, A.chunkSum = dChunkSum, A.chunkBase = dChunkBase;
        A.cent = dCent, A.counts = dCounts, A.gsz = dGsz, A.choff = dChoff, A.tailH = dTailH, A.tailP = dTailP;
        A.nextIdx = dNextIdx, A.st = dSt;
        const dim3 gPos(nchunks), gNode((nn + 63) / 64);

        clock.begin(PH_SEED);
        hipLaunchKernelGGL(k_level_init, gPos, dim3(kChunk), 0, stream, A);
        hipLaunchKernelGGL(k_seed_pick, gNode, dim3(64), 0, stream, A, 0);
        for (int r = 1; r < k && nkm; r++) {
            hipLaunchKernelGGL(k_seed_dist, gPos, dim3(kChunk), 0, stream, A, r);
            hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(kChunk), 0, stream, A);
            hipLaunchKernelGGL(k_seed_pick, gNode, dim3(64), 0, stream, A, r);
        }
        clock.end();
        HIPCHK(hipGetLastError());

        for (int pass = 0; nkm; pass++) {
            if (pass > 0) {
                clock.begin(PH_MEAN);
                HIPCHK(hipMemsetAsync(dCounts.get(), 0, (size_t)nkm * k * kCountStride * 4, stream));
                hipLaunchKernelGGL(k_mean_count, dim3((N + kMeanChunk - 1) / kMeanChunk), dim3(256), 0, stream, A);
                hipLaunchKernelGGL(k_mean_majority, dim3((unsigned)(((size_t)nkm * k * 8 + 255) / 256)), dim3(256), 0, stream, A);
                clock.end();
            }
            clock.begin(PH_ASSIGN);
            hipLaunchKernelGGL(k_assign, gPos, dim3(kChunk), 0, stream, A, pass == 0 ? 1 : 0);
            hipLaunchKernelGGL(k_lloyd_check, gNode, dim3(64), 0, stream, A, pass == 0 ? 1 : 0);
            clock.end();
            HIPCHK(hipGetLastError());
            int32_t moving = 0; /* the one word the host reads per pass */
            HIPCHK(hipMemcpyAsync(&moving, &dSt.get()->any_moving, 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemsetAsync(&dSt.get()->any_moving, 0, 4, stream));
            HIPCHK(hipStreamSynchronize(stream));
            clock.collect();
            if (!moving) break;
        }

        clock.begin(PH_PART);
        const bool split = lev < p.L;
        if (split) {
            HIPCHK(hipMemsetAsync(dGsz.get(), 0, slots * 4, stream));
            hipLaunchKernelGGL(k_part_hist, gPos, dim3(kChunk), 0, stream, A);
            hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(64), 0, stream, A);
            hipLaunchKernelGGL(k_part_childoff, gNode, dim3(64), 0, stream, A);
            HIPCHK(hipGetLastError());
        }
        hCent.resize(slots * 32);
        hGsz.assign(slots, 0);
        HIPCHK(hipMemcpyAsync(hNodes.data(), dNodes.get(), (size_t)nn * sizeof(NodeDev), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(hCent.data(), dCent.get(), slots * 32, hipMemcpyDeviceToHost, stream));
        if (split) HIPCHK(hipMemcpyAsync(hGsz.data(), dGsz.get(), slots * 4, hipMemcpyDeviceToHost, stream));
        clock.end(); /* the host's tree building below is in ms_total only */
        HIPCHK(hipStreamSynchronize(stream));

        /* the children of every node of the level, in cluster order; those with more than one feature form the next level */
        std::vector<LevelNode> next;
        hNext.assign(slots, -1);
        for (int n = 0; n < nn; n++) {
            const NodeDev& nd = hNodes[n];
            st.draws += nd.draws;
            if (nd.cidx >= 0) {
                st.total_passes += nd.passes;
                st.max_passes = std::max(st.max_passes, nd.passes);
            }
            int run = nd.off;
            for (int c = 0; c < nd.nclus; c++) {
                TreeNode t;
                t.parent = level[n].tree, t.level = lev;
                memcpy(t.desc, &hCent[((size_t)n * k + c) * 32], 32);
                const int id = (int)tree.size();
                tree[level[n].tree].children.push_back(id);
                tree.push_back(t);
                if (!split) continue;
                const int size = (int)hGsz[(size_t)n * k + c];
                if (size > 1) {
                    hNext[(size_t)n * k + c] = (int32_t)next.size();
                    next.push_back(LevelNode{run, size, vslamvoc_child_key(nd.key, c), id});
                } else if (size == 1) {
                    st.single_leaves++;
                }
                run += size;
            }
        }
        if (split && !next.empty()) {
            clock.begin(PH_PART);
            HIPCHK(hipMemcpyAsync(dNextIdx.get(), hNext.data(), slots * 4, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemsetAsync(dNodeOf2.get(), 0xff, (size_t)N * 4, stream));
            hipLaunchKernelGGL(k_part_scatter, gPos, dim3(kChunk), 0, stream, A);
            HIPCHK(hipGetLastError());
            clock.end();
            HIPCHK(hipStreamSynchronize(stream)); /* hNext and the level's tables are reused by the next level */
            dPerm.swap(dPerm2);
            dNodeOf.swap(dNodeOf2);
        }
        clock.collect();
        level.swap(next);
    }

    StatsDev hSt;
    HIPCHK(hipMemcpy(&hSt, dSt.get(), sizeof(hSt), hipMemcpyDeviceToHost));
    st.redraws = (int64_t)hSt.redraws, st.empty_groups = (int64_t)hSt.empty_groups;
    st.early_stops = hSt.early_stops, st.hit_max_iter = hSt.hit_max_iter;

    vslam_voc_file* f = finish_tree(p, tree, &st);
    if (p.weighting == 0 || p.weighting == 2) {
        /* setNodeWeights: Vocabulary::transform of every training feature by the product's own kernel */
        vslam_voc* voc = nullptr;
        if ((rc = vslam_voc_file_upload(device, f, &voc))) {
            vslam_voc_file_close(f);
            return rc;
        }
        vslam_dbuf<int32_t> dWord, dNid;
        vslam_dbuf<double> dW;
        std::vector<int32_t> word((size_t)N);
        clock.begin(PH_WEIGHTS);
        if (!(rc = dWord.alloc(N)) && !(rc = dNid.alloc(N)) && !(rc = dW.alloc(N)) &&
            !(rc = vslam_bow_descend_words(voc, dDesc, N, dWord, dW, dNid, stream))) {
            clock.end();
            if (hipMemcpyAsync(word.data(), dWord.get(), (size_t)N * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess) {
                g_err = "vocabulary training: reading the words back failed";
                rc = VSLAM_ERR_HIP;
            }
        }
        vslam_voc_destroy(voc);
        if (rc) {
            vslam_voc_file_close(f);
            return rc;
        }
        clock.collect();
        set_weights(*f, word.data(), doc_offsets, n_docs);
    } else {
        set_weights(*f, nullptr, doc_offsets, n_docs);
    }
    HIPCHK(hipEventRecord(evAll1, stream));
    HIPCHK(hipEventSynchronize(evAll1));
    (void)hipEventElapsedTime(&st.ms_total, evAll0, evAll1);
    st.ms_seed = clock.ms[PH_SEED], st.ms_assign = clock.ms[PH_ASSIGN], st.ms_mean = clock.ms[PH_MEAN];
    st.ms_partition = clock.ms[PH_PART], st.ms_weights = clock.ms[PH_WEIGHTS];
    if (stats) *stats = st;
    *out = f;
    return VSLAM_OK;
}

}  // namespace

extern "C" int vslam_voc_train(int device, const vslam_voc_train_params* params, const uint8_t* desc, int desc_location,
                               const int64_t* doc_offsets, int n_docs, vslam_voc_file** out, vslam_voc_train_stats* stats) {
    if (!out || !desc || (desc_location != VSLAM_IMGS_HOST && desc_location != VSLAM_IMGS_DEVICE)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    vslam_voc_train_params p;
    int64_t n = 0;
    int rc = check_params(params, doc_offsets, n_docs, &p, &n); /* before any HIP call: nothing is launched on bad input */
    if (rc != VSLAM_OK) {
        g_err = vslam_voc_file_last_error();
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_err = "no usable HIP device (this library has no CPU fallback)";
        return VSLAM_ERR_NO_DEVICE;
    }
    return train(device, p, desc, desc_location, doc_offsets, n_docs, n, out, stats);
}
