/* vslam_frustum.hip -- the first half of Tracking::SearchLocalPoints (tracking.cpp:3217-3235) on the device:
 * Frame::isInFrustum over the local map, then an ordered compaction of the points that go on to
 * FMatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (k_sbp_rank mode 1, unchanged).
 *
 * k_frustum          one lane per MapPoint, one workgroup per chunk of VSLAM_FRUSTUM_CHUNK points: the record of
 *                    vslam_frustum.h for every point, mTrackDepth, and per chunk the number of points in view (nToMatch) and
 *                    of points to keep.  keep = mbTrackInView && !(bFarPoints && mTrackDepth > thFarPoints): the skip the
 *                    matcher applies itself at fmatcher.cpp:327-350, applied before it.
 * k_frustum_compact  the same grid: every workgroup sums the chunk counts before its own (at most 256, one per lane), ranks
 *                    its lanes by ballot / popcount and a four-entry scan of the wave totals in LDS, and scatters record,
 *                    descriptor, matcher flags and original index of the kept points IN THEIR ORIGINAL ORDER -- the matcher
 *                    walks vpMapPoints in order and its result depends on it.  Slots beyond the capacity are not written;
 *                    the last workgroup writes the true count, the clamped count the matcher reads, and nToMatch.
 *
 * k_rig_keep, k_rig_compact: the same compaction for a two-camera rig (left || right), behind k_frustum_rig of vslam_kb8.hip.
 *
 * Two launches, plain stores: no workgroup waits for another one and no atomic decides an order.
 * The arithmetic is FP32 with two FP64 norms and glibc's logf polynomial in FP64 per point: a few hundred operations per
 * lane, 65536 lanes at most.
 */
#include "vslam_ctx.h"
#include "vslam_frustum.h"

static_assert(VSLAM_FRUSTUM_CHUNK == 256 && VSLAM_FRUSTUM_MAX_POINTS / VSLAM_FRUSTUM_CHUNK <= VSLAM_FRUSTUM_CHUNK,
              "k_frustum_compact sums the chunk counts with one load per lane");
static_assert(sizeof(vslam_map_point) == 36 && sizeof(vslam_mp_track) == 24, "record layouts");

__device__ __forceinline__ int fr_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK)
k_frustum(FrustumArgsDev A) {
    __shared__ int s_view[4], s_keep[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * VSLAM_FRUSTUM_CHUNK + tid;
    bool view = false, keep = false;
    if (i < A.n) {
        const vslam_map_point mp = A.pts[i];
        vslam_mp_track t;
        float depth;
        vslam_fr::in_frustum(A.F, mp, &t, &depth);
        A.track[i] = t;
        A.depth[i] = depth;
        view = (t.flags & 1u) != 0;
        keep = view && !(A.farPoints && depth > A.thFarPoints);
    }
    const unsigned long long bv = __ballot(view), bk = __ballot(keep);
    if (lane == 0) {
        s_view[wave] = __popcll(bv);
        s_keep[wave] = __popcll(bk);
    }
    __syncthreads();
    if (tid == 0) {
        A.chunkInView[blockIdx.x] = s_view[0] + s_view[1] + s_view[2] + s_view[3];
        A.chunkKeep[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
    }
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK)
k_frustum_compact(FrustumCompactDev A) {
    __shared__ int s_before[4], s_views[4], s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const bool last = b == (int)gridDim.x - 1;
    /* chunk counts: lane t holds chunk t (nchunks <= 256) */
    const int before = fr_wave_sum(tid < b ? A.chunkKeep[tid] : 0);
    const int views = fr_wave_sum((last && tid < A.nchunks) ? A.chunkInView[tid] : 0);
    const int i = b * VSLAM_FRUSTUM_CHUNK + tid;
    bool keep = false;
    uint32_t fl = 0;
    if (i < A.n) {
        fl = A.track[i].flags;
        keep = (fl & 1u) && !(A.farPoints && A.depth[i] > A.thFarPoints);
    }
    const unsigned long long bk = __ballot(keep);
    const int rank = __popcll(bk & ((1ull << lane) - 1ull));
    if (lane == 0) {
        s_before[wave] = before;
        s_views[wave] = views;
        s_wave[wave] = __popcll(bk);
    }
    __syncthreads();
    const int base = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    int woff = 0;
    for (int w = 0; w < wave; w++) woff += s_wave[w];
    const int pos = base + woff + rank;
    if (keep && pos < A.cap) {
        A.trackC[pos] = A.track[i];
        const uint4* src = (const uint4*)(A.desc + (size_t)i * 32);
        uint4* dst = (uint4*)(A.descC + (size_t)pos * 32);
        dst[0] = src[0];
        dst[1] = src[1];
        A.flagsC[pos] = (uint8_t)(1u | (fl & 2u)); /* bit 0: valid query; bit 1: Observations() > 0 blocks its keypoint */
        A.indexC[pos] = i;
    }
    if (last && tid == 0) {
        const int kept = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        A.counts[0] = kept;
        A.counts[1] = min(kept, A.cap);
        A.counts[2] = s_views[0] + s_views[1] + s_views[2] + s_views[3];
    }
}

/* The rig's compaction (behind k_frustum_rig, which writes both record arrays, both depths and the per-chunk left || right
 * counts, and is not edited for this): a point goes on to the matcher iff (left bit 0 || right bit 0) and it is not far.  The far
 * test (fmatcher.cpp:333) reads mTrackDepth, the LEFT depth, for every point: 0 where the left camera does not see it, so a
 * right-only point is never far.  k_rig_keep counts the kept points per chunk; k_rig_compact is k_frustum_compact with two
 * record arrays: ballot / popcount ranks over a running base, original order kept, plain stores. */
__device__ __forceinline__ bool rig_keep(const FrustumRigCompactDev& A, int i, uint32_t fl) {
    return (fl & 1u) && !(A.farPoints && A.depthL[i] > A.thFarPoints);
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK)
k_rig_keep(FrustumRigCompactDev A) {
    __shared__ int s_keep[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * VSLAM_FRUSTUM_CHUNK + tid;
    const uint32_t fl = i < A.n ? (A.trackL[i].flags | A.trackR[i].flags) : 0u; /* one MapPoint: bit 1 is the same in both */
    const bool keep = i < A.n && rig_keep(A, i, fl);
    const unsigned long long bk = __ballot(keep);
    if (lane == 0) s_keep[wave] = __popcll(bk);
    __syncthreads();
    if (tid == 0) A.chunkKeep[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK)
k_rig_compact(FrustumRigCompactDev A) {
    __shared__ int s_before[4], s_views[4], s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const bool last = b == (int)gridDim.x - 1;
    const int before = fr_wave_sum(tid < b ? A.chunkKeep[tid] : 0);
    const int views = fr_wave_sum((last && tid < A.nchunks) ? A.chunkInView[tid] : 0);
    const int i = b * VSLAM_FRUSTUM_CHUNK + tid;
    const uint32_t fl = i < A.n ? (A.trackL[i].flags | A.trackR[i].flags) : 0u; /* one MapPoint: bit 1 is the same in both */
    const bool keep = i < A.n && rig_keep(A, i, fl);
    const unsigned long long bk = __ballot(keep);
    const int rank = __popcll(bk & ((1ull << lane) - 1ull));
    if (lane == 0) {
        s_before[wave] = before;
        s_views[wave] = views;
        s_wave[wave] = __popcll(bk);
    }
    __syncthreads();
    const int base = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    int woff = 0;
    for (int w = 0; w < wave; w++) woff += s_wave[w];
    const int pos = base + woff + rank;
    if (keep && pos < A.cap) {
        A.trackLC[pos] = A.trackL[i];
        A.trackRC[pos] = A.trackR[i];
        const uint4* src = (const uint4*)(A.desc + (size_t)i * 32);
        uint4* dst = (uint4*)(A.descC + (size_t)pos * 32);
        dst[0] = src[0];
        dst[1] = src[1];
        A.flagsC[pos] = (uint8_t)(1u | (fl & 2u)); /* bit 1: Observations() > 0, the occupancy a write leaves in its slot */
        A.indexC[pos] = i;
    }
    if (last && tid == 0) {
        const int kept = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        A.counts[0] = kept;
        A.counts[1] = min(kept, A.cap);
        A.counts[2] = s_views[0] + s_views[1] + s_views[2] + s_views[3];
    }
}

void vk_rig_compact(hipStream_t st, const FrustumRigCompactDev& A) {
    if (A.n <= 0) return;
    hipLaunchKernelGGL(k_rig_keep, dim3(A.nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A);
    hipLaunchKernelGGL(k_rig_compact, dim3(A.nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A);
}

void vk_frustum(hipStream_t st, const FrustumArgsDev& A) {
    if (A.n <= 0) return;
    const int nchunks = (A.n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    hipLaunchKernelGGL(k_frustum, dim3(nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A);
}

void vk_frustum_compact(hipStream_t st, const FrustumCompactDev& A) {
    if (A.n <= 0) return;
    hipLaunchKernelGGL(k_frustum_compact, dim3(A.nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A);
}
