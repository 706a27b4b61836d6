/* vslam_projection_kernels.hip -- the kernels of the SearchByProjection family, Frame::UnprojectStereo and the search
 * half of Fuse / SearchBySim3 (launched from vslam_projection.hip).
 *
 * ==================================================================================================
 * FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * (fmatcher.cpp:2471-2687, pinhole frames: Nleft == -1) -- the per-frame tracking matcher of
 * TrackWithMotionModel (tracking.cpp:2728).  Same decomposition as SearchForInitialization (vslam_init_kernel.hip):
 *
 *   k_sbp_rank   (parallel, one wave per last-frame keypoint): project its MapPoint into the current frame
 *                (Rcw*x3Dw+tcw as ONE cv::gemm: products accumulated in double, rounded once; 1.0/z in
 *                double; Pinhole::project in float), query the window (Frame::GetFeaturesInArea with the
 *                forward / backward / +-1 octave rule), apply the order-free mvuRight gate, and write the M
 *                smallest keys = dist << 24 | gridcell << 12 | i2 in ascending order ("first wins" on equal
 *                distance is the key order).
 *   k_sbp_replay (one wave, last-frame keypoints in index order): the only sequential state is "current
 *                keypoint i2 already carries a MapPoint with observations" (the skip at fmatcher.cpp:2545-
 *                2547); the first list entry that is not occupied is bestIdx2.  An exhausted full list falls
 *                back to a full re-scan of that query.  Assignments go to a log; mvpMapPoints ("last writer
 *                wins"), the rotation histogram, ComputeThreeMaxima and nmatches are rebuilt from it.
 * ================================================================================================== */
#include "vslam_kernels.h"
#include "vslam_wave.h"
#include "vslam_matchdev.h"
#include "vslam_kb8.h"

#define SBP_TH_HIGH 100
#define SBP_QPB 16 /* queries per k_sbp_rank workgroup (4 waves x 4) */

struct SbpCand { /* one keypoint of the current frame */
    float x, y, uRight;
    uint16_t cell; /* 0xFFFF: outside the grid */
    uint16_t octave;
};
struct SbpProj { /* projection record of one last-frame keypoint (k_sbp_rank -> k_sbp_replay's re-scan) */
    float u, v, radius, ur;
    int32_t minLevel, maxLevel, valid, pad;
};
static_assert(sizeof(SbpProj) == 32, "k_s3k_compact moves a record as two uint4");

__device__ __forceinline__ bool sbp_level_ok(int octave, int minLevel, int maxLevel) { /* frame.cpp:712-728 */
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    if (!bCheckLevels) return true;
    if (octave < minLevel) return false;
    if (maxLevel >= 0 && octave > maxLevel) return false;
    return true;
}

/* the order-free part of the candidate loop body (fmatcher.cpp:2541-2556): window, level, mvuRight gate.  Cell range,
 * level, then distance, as GetFeaturesInArea has them: with the distance in front of the level (si_in_window as one call)
 * the k_sbpm chain measured 5 % slower (profiles/matcher_kernel_helpers_ab.txt) */
__device__ __forceinline__ bool sbp_candidate_ok(const SbpCand& cd, const SiWindow& w, const SbpProj& pr) {
    if (!si_cell_in_window(cd.cell, w)) return false;
    if (!sbp_level_ok(cd.octave, pr.minLevel, pr.maxLevel)) return false;
    const float distx = __fsub_rn(cd.x, pr.u), disty = __fsub_rn(cd.y, pr.v);
    if (!(fabsf(distx) < pr.radius && fabsf(disty) < pr.radius)) return false;
    if (cd.uRight > 0.f) { /* CurrentFrame.mvuRight[i2] > 0 */
        const float er = fabsf(__fsub_rn(pr.ur, cd.uRight));
        if (er > pr.radius) return false;
    }
    return true;
}

__device__ __forceinline__ SbpCand sbp_make_cand(const vslam_kp& k, float uRight, const SiBounds& b, const SiGridInv& inv) {
    SbpCand c;
    c.x = k.x;
    c.y = k.y;
    c.uRight = uRight;
    c.cell = (uint16_t)si_grid_cell(k.x, k.y, b, inv); /* -1 -> 0xFFFF */
    c.octave = (uint16_t)k.octave;
    return c;
}

/* ---- k_sbp_rank's query projections, one per J.mode; all of them wave-uniform ---- */

/* Pinhole::project (pinhole.cpp:13-16) */
__device__ __forceinline__ float2 sbp_pinhole(const SbpJobDev& J, const SbpPoint& pc) {
    return make_float2(__fadd_rn(__fdiv_rn(__fmul_rn(J.fx, pc.x), pc.z), J.cx),
                       __fadd_rn(__fdiv_rn(__fmul_rn(J.fy, pc.y), pc.z), J.cy));
}
/* the closed interval over the Frame's float grid bounds */
__device__ __forceinline__ bool sbp_in_frame(float2 uv, const SiBounds& b) {
    return !(uv.x < b.minX || uv.x > b.maxX) && !(uv.y < b.minY || uv.y > b.maxY);
}

/* mode 1: pre-projected MapPoints (fmatcher.cpp:327-350) */
__device__ __forceinline__ SbpProj sbp_proj_tracked(const SbpJobs& JS, const SbpJobDev& J, const MpTrack& mp) {
    SbpProj pr = {};
    if (!(mp.flags & 1)) return pr;
    float r = (double)mp.viewCos > 0.998 ? 2.5f : 4.0f; /* RadiusByViewingCos, fmatcher.cpp:493-499 */
    if (J.th != 1.0f) r = __fmul_rn(r, J.th);
    pr.u = mp.projX;
    pr.v = mp.projY;
    pr.radius = __fmul_rn(r, JS.scale[min(max(mp.level, 0), JS.nlevels - 1)]);
    pr.ur = mp.projXR;
    pr.minLevel = mp.level - 1;
    pr.maxLevel = mp.level;
    pr.valid = 1;
    return pr;
}

/* mode 0: the last frame's MapPoints, pMP && !LastFrame.mvbOutlier[i] */
__device__ __forceinline__ SbpProj sbp_proj_last_frame(const SbpJobs& JS, const SbpJobDev& J, const SbpPoint& pc, int oct,
                                                       const SiBounds& bnd) {
    SbpProj pr = {};
    const float invzc = (float)__ddiv_rn(1.0, (double)pc.z);
    if (invzc < 0.f) return pr;
    const float2 uv = sbp_pinhole(J, pc);
    if (!sbp_in_frame(uv, bnd)) return pr;
    pr.u = uv.x;
    pr.v = uv.y;
    pr.radius = __fmul_rn(J.th, JS.scale[min(max(oct, 0), JS.nlevels - 1)]);
    pr.ur = __fsub_rn(uv.x, __fmul_rn(J.mbf, invzc));
    if (J.forward) { pr.minLevel = oct; pr.maxLevel = -1; }
    else if (J.backward) { pr.minLevel = 0; pr.maxLevel = oct; }
    else { pr.minLevel = oct - 1; pr.maxLevel = oct + 1; }
    pr.valid = 1;
    return pr;
}

/* modes 2 and 3, first half: PO = x3Dw - Ow (Ow = -Rcw^T tcw is cv::Mat algebra on the caller's side: it arrives in
 * JS.kf.ow), dist3D = cv::norm(PO) inside the point's scale-invariance range */
struct SbpDist {
    float p0, p1, p2, dist3D, maxDist;
    bool inRange;
};
__device__ __forceinline__ SbpDist sbp_dist(const SbpKfDev& kf, int q, float X, float Y, float Z) {
    SbpDist d;
    d.p0 = __fsub_rn(X, kf.ow[0]);
    d.p1 = __fsub_rn(Y, kf.ow[1]);
    d.p2 = __fsub_rn(Z, kf.ow[2]);
    d.dist3D = vslam_md::norm3(d.p0, d.p1, d.p2);
    d.maxDist = kf.maxDist[q];
    d.inRange = !(d.dist3D < kf.minDist[q] || d.dist3D > d.maxDist);
    return d;
}
/* ... second half: PredictScale, radius = th * scale[level], levels [level - 1, maxLevel(level)] */
__device__ __forceinline__ SbpProj sbp_proj_level(const SbpJobs& JS, float th, float2 uv, const SbpDist& d, int levelsUp) {
    SbpProj pr = {};
    const int level = vslam_md::predict_level(d.maxDist, d.dist3D, JS.kf.logScaleFactor, JS.nlevels);
    pr.u = uv.x;
    pr.v = uv.y;
    pr.radius = __fmul_rn(th, JS.scale[level]);
    pr.minLevel = level - 1;
    pr.maxLevel = level + levelsUp;
    pr.valid = 1;
    return pr;
}

/* mode 2: KeyFrame MapPoints into the current frame, fmatcher.cpp:2705-2743; pMP && !isBad() && !sAlreadyFound.count(pMP) */
__device__ __forceinline__ SbpProj sbp_proj_keyframe(const SbpJobs& JS, const SbpJobDev& J, int q, const SbpPoint& pc,
                                                     float X, float Y, float Z, const SiBounds& bnd) {
    const float2 uv = sbp_pinhole(J, pc); /* no depth test here */
    if (!sbp_in_frame(uv, bnd)) return SbpProj{};
    const SbpDist d = sbp_dist(JS.kf, q, X, Y, Z);
    if (!d.inRange) return SbpProj{};
    return sbp_proj_level(JS, J.th, uv, d, /* maxLevel = level + */ 1);
}

/* mode 3: candidate MapPoints into a KeyFrame under Scw, fmatcher.cpp:773-825 / :890-941; !pMP->isBad() &&
 * !spAlreadyFound.count(pMP).  wbnd: the KeyFrame's integer bounds */
__device__ __forceinline__ SbpProj sbp_proj_sim3(const SbpJobs& JS, const SbpJobDev& J, int q, const SbpPoint& pc,
                                                 float X, float Y, float Z, const SiBounds& wbnd) {
    if (pc.z < 0.0f) return SbpProj{};
    float2 uv;
    if (JS.kf.projKind == 0) {
        uv = sbp_pinhole(J, pc);
    } else {
        const float invz = __fdiv_rn(1.0f, pc.z);
        uv.x = __fadd_rn(__fmul_rn(J.fx, __fmul_rn(pc.x, invz)), J.cx);
        uv.y = __fadd_rn(__fmul_rn(J.fy, __fmul_rn(pc.y, invz)), J.cy);
    }
    if (!(uv.x >= wbnd.minX && uv.x < wbnd.maxX && uv.y >= wbnd.minY && uv.y < wbnd.maxY)) return SbpProj{}; /* KeyFrame::IsInImage, keyframe.cpp:701-703 */
    const SbpDist d = sbp_dist(JS.kf, q, X, Y, Z);
    if (!d.inRange) return SbpProj{};
    /* PO.dot(Pn) < 0.5*dist: cv::Mat::dot accumulates in double */
    if (vslam_md::dot3_mat(d.p0, d.p1, d.p2, JS.kf.normals + 3 * q) < __dmul_rn(0.5, (double)d.dist3D)) return SbpProj{};
    return sbp_proj_level(JS, J.th, uv, d, /* maxLevel = level + */ 0);
}

/* mode 4: the last frame's MapPoints into the current frame of a two-fisheye rig (fmatcher.cpp:2494-2659 with
 * CurrentFrame.Nleft != -1).  Job 0 is the left branch: as mode 0 with KannalaBrandt8::project.  Job 1 is the right branch
 * (:2593-2611): x3Dr = Rrl * x3Dc + trl as one gemm, projected through the LEFT camera's model (:2596 reads mpCamera, not
 * mpCamera2), and no depth test and no in-frame test.  That the left branch's three `continue`s skip the right branch is not
 * known here -- the blocks of a launch are unordered -- but to the resolver, which reads the left job's prefix. */
__device__ __forceinline__ SbpProj sbp_proj_rig(const SbpJobs& JS, const SbpJobDev& J, const RigFrameDev& R, int right,
                                                const SbpPoint& pc, int oct, const SiBounds& bnd) {
    SbpProj pr = {};
    vslam_kb8::Uv uv;
    if (!right) {
        const float invzc = (float)__ddiv_rn(1.0, (double)pc.z);
        if (invzc < 0.f) return pr;
        uv = vslam_kb8::kb8_project(R.cam, pc.x, pc.y, pc.z);
        if (!sbp_in_frame(make_float2(uv.u, uv.v), bnd)) return pr;
    } else {
        const SbpPoint pr3 = sbp_transform(R.Trl, pc.x, pc.y, pc.z, J.gemmFloat);
        uv = vslam_kb8::kb8_project(R.cam, pr3.x, pr3.y, pr3.z);
    }
    pr.u = uv.u;
    pr.v = uv.v;
    pr.radius = __fmul_rn(J.th, JS.scale[min(max(oct, 0), JS.nlevels - 1)]);
    if (J.forward) { pr.minLevel = oct; pr.maxLevel = -1; }
    else if (J.backward) { pr.minLevel = 0; pr.maxLevel = oct; }
    else { pr.minLevel = oct - 1; pr.maxLevel = oct + 1; }
    pr.valid = 1;
    return pr;
}

/* mode 2 with a fisheye CurrentFrame (fmatcher.cpp:2705-2743 with KannalaBrandt8::project at :2718): as sbp_proj_keyframe.
 * There is no depth test: a point behind the camera is projected like any other (theta > pi / 2) and goes on where it lands
 * inside the bounds */
__device__ __forceinline__ SbpProj sbp_proj_keyframe_kb8(const SbpJobs& JS, const SbpJobDev& J, const vslam_kb8_camera& cam,
                                                         int q, const SbpPoint& pc, float X, float Y, float Z,
                                                         const SiBounds& bnd) {
    const vslam_kb8::Uv o = vslam_kb8::kb8_project(cam, pc.x, pc.y, pc.z);
    const float2 uv = make_float2(o.u, o.v);
    if (!sbp_in_frame(uv, bnd)) return SbpProj{};
    const SbpDist d = sbp_dist(JS.kf, q, X, Y, Z);
    if (!d.inRange) return SbpProj{};
    return sbp_proj_level(JS, J.th, uv, d, /* maxLevel = level + */ 1);
}

/* one body, three kernels (vslam_sbp_rank_body.inc): the rig kernel adds query mode 4 and the struct it reads, the KB8 kernel
 * reads modes 2 and 3 as their fisheye forms, and the kernel the pinhole matchers launch keeps its argument list and its code */
__global__ void __launch_bounds__(256)
k_sbp_rank(SbpJobs JS) {
#define SBP_RANK_RIG 0
#include "vslam_sbp_rank_body.inc"
#undef SBP_RANK_RIG
}
__global__ void __launch_bounds__(256)
k_sbp_rank_rig(SbpJobs JS, RigFrameDev R) {
#define SBP_RANK_RIG 1
#include "vslam_sbp_rank_body.inc"
#undef SBP_RANK_RIG
}
/* SearchByProjection(CurrentFrame, pKF, ..) with a fisheye CurrentFrame (mode 2), and the ranking of the survivors of
 * k_s3k_gate (mode 3: SearchByProjection(pKF, Scw, ..) with a fisheye KeyFrame) */
__global__ void __launch_bounds__(256)
k_sbp_rank_kb8(SbpJobs JS, vslam_kb8_camera cam) {
#define SBP_RANK_RIG 2
#include "vslam_sbp_rank_body.inc"
#undef SBP_RANK_RIG
}

/* full re-scan of one query's window in candidate order (the reference loop body) -> best key or ~0 */
__device__ uint32_t sbp_full_scan(const SbpProj& pr, const vslam_kp* curKps, const float* uRight, int nCur,
                                  const uint8_t* mpDescQ, const uint8_t* curDesc, const uint32_t* occupied,
                                  const SiBounds& bnd, const SiBounds& wbnd, const SiGridInv& inv, int lane) {
    uint32_t bestKey = 0xFFFFFFFFu;
    const SiWindow win = si_window_b(pr.u, pr.v, pr.radius, wbnd, inv);
    if (!win.empty) {
        const uint4 da = ((const uint4*)mpDescQ)[0], db = ((const uint4*)mpDescQ)[1];
        for (int c = lane; c < nCur; c += 64) {
            const SbpCand cd = sbp_make_cand(curKps[c], uRight ? uRight[c] : -1.f, bnd, inv);
            if (cd.cell == 0xFFFF || occupied[c] || !sbp_candidate_ok(cd, win, pr)) continue;
            const uint4 ta = ((const uint4*)curDesc)[(size_t)c * 2], tb = ((const uint4*)curDesc)[(size_t)c * 2 + 1];
            bestKey = min(bestKey, si_key(si_hamming(da, db, ta, tb), cd.cell, (uint32_t)c));
        }
    }
    return wave_min_u32(bestKey);
}

/* ------------------------------------------------------------------------------------------------
 * The sequential rule "query q takes the first candidate of its sorted list that no earlier query with
 * observations has taken" is a serial dictatorship, and a serial dictatorship is the fixpoint of deferred
 * acceptance with one common priority order: every query points at a candidate; a candidate is held by the
 * lowest-index blocking query pointing at it; whoever sees a lower-index holder moves on to its next candidate.
 * Holders' indices only decrease, so a rejection is final and the fixpoint is the sequential result.  One
 * 1024-thread workgroup per job iterates this in parallel (a handful of rounds) instead of one wave walking
 * 2000 queries in order.  Only when some query runs off a FULL sorted prefix (it would need candidates that
 * k_sbp_rank did not keep) the job is handed to k_sbp_replay, which walks it sequentially with full re-scans.
 * ---------------------------------------------------------------------------------------------- */
#define SBP_RT 1024
#define SBP_QPT 4 /* queries per thread: capacity 4096 */
__global__ void __launch_bounds__(SBP_RT)
k_sbp_resolve(SbpJobs JS, int forceSeq) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& J = JS.job[blockIdx.x];
    const uint32_t thHigh = JS.kf.thHigh ? (uint32_t)(JS.kf.thHigh - 1) : (uint32_t)SBP_TH_HIGH;
    const int M = JS.M;
    const auto [nLast, nCur] = sbp_counts(J);
    int32_t* holder = (int32_t*)sbsm; /* nCur: lowest-index blocking query pointing here; -1 = occupied from the start */
    int32_t* owner = holder + nCur;   /* nCur: highest-index query assigned here (mvpMapPoints: last writer wins) */
    __shared__ int s_changed, s_seq, s_nlog, s_removed;
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_seq = forceSeq;
        s_nlog = 0;
        s_removed = 0;
    }
    if (tid < VSLAM_HISTO_LENGTH) s_hist[tid] = 0;
    for (int c = tid; c < nCur; c += SBP_RT) {
        holder[c] = (J.occupied0 && J.occupied0[c]) ? -1 : 0x7FFFFFFF;
        owner[c] = -1;
    }
    uint32_t key[SBP_QPT];
    int ptr[SBP_QPT];
    bool blocking[SBP_QPT];
#pragma unroll
    for (int k = 0; k < SBP_QPT; k++) {
        const int q = tid + k * SBP_RT;
        ptr[k] = 0;
        key[k] = q < nLast ? J.topm[(size_t)q * M] : 0xFFFFFFFFu;
        blocking[k] = q < nLast && (J.flags[q] & 2);
    }
    __syncthreads();
    for (int round = 0; round < 4096 && !s_seq; round++) { /* s_seq / s_changed are block-uniform at the barriers */
        if (tid == 0) s_changed = 0;
#pragma unroll
        for (int k = 0; k < SBP_QPT; k++)
            if (key[k] != 0xFFFFFFFFu && blocking[k] && si_key_dist(key[k]) <= thHigh)
                atomicMin(&holder[si_key_index(key[k])], tid + k * SBP_RT);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SBP_QPT; k++) {
            const int q = tid + k * SBP_RT;
            if (key[k] != 0xFFFFFFFFu && holder[si_key_index(key[k])] < q) { /* taken by an earlier query: next candidate */
                ptr[k]++;
                if (ptr[k] >= M) {
                    s_seq = 1; /* ran off a full prefix */
                    key[k] = 0xFFFFFFFFu;
                } else {
                    key[k] = J.topm[(size_t)q * M + ptr[k]]; /* ~0: the list is complete and exhausted */
                }
                s_changed = 1;
            }
        }
        __syncthreads();
        if (!s_changed) break;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) *J.needSeq = s_seq;
    if (s_seq) return;
    /* assignments */
    uint32_t bin[SBP_QPT];
#pragma unroll
    for (int k = 0; k < SBP_QPT; k++) {
        const int q = tid + k * SBP_RT;
        bin[k] = 255;
        if (key[k] != 0xFFFFFFFFu && si_key_dist(key[k]) <= thHigh) {
            const int i2 = (int)si_key_index(key[k]);
            atomicMax(&owner[i2], q);
            atomicAdd(&s_nlog, 1);
            bin[k] = 254;
            if (J.checkOri) {
                const int b = vslam_md::rot_bin(J.lastKps[q].angle, J.curKps[i2].angle, VSLAM_HISTO_LENGTH);
                bin[k] = (uint32_t)b;
                atomicAdd(&s_hist[b], 1);
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < nCur; c += SBP_RT) J.matchCur[c] = owner[c];
    __syncthreads();
    if (J.checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
#pragma unroll
        for (int k = 0; k < SBP_QPT; k++) {
            const int b = (int)bin[k];
            if (b < VSLAM_HISTO_LENGTH && !vslam_md::keeps_bin(mx, b)) { /* fmatcher.cpp:2668-2681 */
                J.matchCur[si_key_index(key[k])] = -1;
                atomicAdd(&s_removed, 1);
            }
        }
    }
    __syncthreads();
    if (tid == 0) J.nmatches[0] = s_nlog - s_removed;
}

__global__ void __launch_bounds__(64)
k_sbp_replay(SbpJobs JS, int* fallbacks) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& J = JS.job[blockIdx.x];
    const uint32_t thHigh = JS.kf.thHigh ? (uint32_t)(JS.kf.thHigh - 1) : (uint32_t)SBP_TH_HIGH;
    const int M = JS.M;
    const auto [nLast, nCur] = sbp_counts(J);
    const vslam_kp* __restrict__ lastKps = J.lastKps;
    const vslam_kp* __restrict__ curKps = J.curKps;
    const uint8_t* __restrict__ curDesc = J.curDesc;
    const uint8_t* __restrict__ mpDesc = J.mpDesc;
    const uint8_t* __restrict__ flags = J.flags;
    const float* __restrict__ uRight = J.uRight;
    const uint8_t* __restrict__ occupied0 = J.occupied0;
    const SbpProj* __restrict__ proj = J.proj;
    const uint32_t* __restrict__ topm = J.topm;
    int32_t* __restrict__ matchCur = J.matchCur;
    int32_t* __restrict__ nmatches_out = J.nmatches;
    struct { int checkOri; SiBounds bnd; } A = {J.checkOri, J.bnd};
    uint32_t* occupied = (uint32_t*)sbsm;              /* nCur: mvpMapPoints[i2] with Observations() > 0 */
    int32_t* ownerEntry = (int32_t*)(occupied + nCur); /* nCur: last log entry that wrote mvpMapPoints[i2] */
    uint32_t* alog = (uint32_t*)(ownerEntry + nCur);   /* nLast: (query << 12 | i2), in order */
    uint8_t* logBin = (uint8_t*)(alog + nLast);        /* nLast: rotation bin of a log entry */
    uint32_t* kbuf = (uint32_t*)(sbsm + (((size_t)nCur * 8 + (size_t)nLast * 5 + 15) & ~(size_t)15)); /* 64 x M */
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    const int lane = threadIdx.x;
    if (*J.needSeq == 0) return; /* k_sbp_resolve finished this job */
    const SiGridInv inv = si_grid_inv(A.bnd);
    const SiBounds wbnd = J.mode == 3 ? si_kf_bounds(A.bnd) : A.bnd;
    for (int c = lane; c < nCur; c += 64) {
        occupied[c] = occupied0 ? occupied0[c] : 0u;
        ownerEntry[c] = -1;
        matchCur[c] = -1;
    }
    if (lane < VSLAM_HISTO_LENGTH) s_hist[lane] = 0;
    __syncthreads();

    int nlog = 0, nfb = 0;
    for (int qb = 0; qb < nLast; qb += 64) {
        const int nq = min(64, nLast - qb);
        __syncthreads();
        for (int i = lane; i < nq * M; i += 64) kbuf[i] = topm[(size_t)qb * M + i];
        const uint32_t myflags = lane < nq ? flags[qb + lane] : 0u; /* lane tq holds query qb+tq's flags */
        __syncthreads();
        uint32_t keyN = lane < M ? kbuf[lane] : 0xFFFFFFFFu;
        uint32_t occN = keyN != 0xFFFFFFFFu ? occupied[si_key_index(keyN)] : 0u;
        for (int tq = 0; tq < nq; tq++) {
            const uint32_t key = keyN, occ = occN;
            if (tq + 1 < nq) {
                keyN = lane < M ? kbuf[(tq + 1) * M + lane] : 0xFFFFFFFFu;
                occN = keyN != 0xFFFFFFFFu ? occupied[si_key_index(keyN)] : 0u;
            }
            const bool valid = key != 0xFFFFFFFFu;
            const unsigned long long mv = __ballot(valid), mk = __ballot(valid && !occ);
            if (mv == 0) continue; /* vIndices2 empty, or every candidate failed an order-free gate */
            uint32_t gBest;
            if (mk) {
                const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
                gBest = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
            } else if (__popcll(mv) < M) {
                continue; /* the list is complete and every entry is occupied: bestDist stays 256 */
            } else {
                nfb++;
                gBest = sbp_full_scan(proj[qb + tq], curKps, uRight, nCur, mpDesc + (size_t)(qb + tq) * 32, curDesc,
                                      occupied, A.bnd, wbnd, inv, lane);
                if (gBest == 0xFFFFFFFFu) continue;
            }
            if (si_key_dist(gBest) > thHigh) continue; /* bestDist <= TH_HIGH (ORBdist in the KeyFrame overload) */
            const uint32_t i2 = si_key_index(gBest);
            const uint32_t fl = (uint32_t)__builtin_amdgcn_readlane((int)myflags, tq);
            if (lane == 0) {
                alog[nlog] = ((uint32_t)(qb + tq) << 12) | i2;
                if (fl & 2) occupied[i2] = 1u; /* pMP->Observations() > 0: later queries skip i2 */
            }
            nlog++;
            if ((fl & 2) && keyN != 0xFFFFFFFFu && si_key_index(keyN) == i2) occN = 1u;
        }
    }
    __syncthreads();
    if (fallbacks && lane == 0 && nfb) atomicAdd(fallbacks, nfb);
    /* mvpMapPoints[bestIdx2] = pMP: the last writer stays */
    for (int e = lane; e < nlog; e += 64) atomicMax(&ownerEntry[alog[e] & 0xFFF], e);
    __syncthreads();
    for (int e = lane; e < nlog; e += 64) {
        const uint32_t le = alog[e];
        const int q = (int)(le >> 12), i2 = (int)(le & 0xFFF);
        if (ownerEntry[i2] == e) matchCur[i2] = q;
        if (A.checkOri) {
            const int bin = vslam_md::rot_bin(lastKps[q].angle, curKps[i2].angle, VSLAM_HISTO_LENGTH);
            logBin[e] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1);
        }
    }
    __syncthreads();
    int removed = 0;
    if (A.checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
        /* every entry of a rejected bin clears mvpMapPoints[idx] and decrements nmatches (fmatcher.cpp:2668-2681) */
        for (int e = lane; e < nlog; e += 64) {
            if (!vslam_md::keeps_bin(mx, logBin[e])) {
                matchCur[alog[e] & 0xFFF] = -1;
                removed++;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) removed += __shfl_xor(removed, o, 64);
    if (lane == 0) nmatches_out[0] = nlog - removed;
}

size_t vk_sbp_rank_lds(int nCur) { return (size_t)nCur * sizeof(SbpCand); }
size_t vk_sbp_replay_lds(int nCur, int nLast) {
    return (((size_t)nCur * 8 + (size_t)nLast * 5 + 15) & ~(size_t)15) + 64 * SI_MAX_M * 4;
}
size_t vk_sbp_scratch_bytes(int nLast, int M) { return (size_t)nLast * (sizeof(SbpProj) + 4 * (size_t)M); }
size_t vk_sbp_proj_bytes(int nLast) { return (size_t)nLast * sizeof(SbpProj); }
/* ------------------------------------------------------------------------------------------------
 * SearchByProjection(Frame& F, const vector<MapPoint*>&, th, ...) (fmatcher.cpp:321-411): same ranking, but a
 * query now looks at its first TWO free candidates (best / second with their octaves, ratio test only when both
 * lie on the same level).  A query's proposal can therefore appear or vanish while the occupancy around it
 * changes, so the resolution is a plain fixpoint: every round rebuilds "lowest-index blocking query that chose
 * this keypoint" from the current choices and lets every query choose again; by induction on the query index the
 * unique fixpoint is the sequential result.  Same hand-over to a sequential wave when a list prefix runs out.
 * ---------------------------------------------------------------------------------------------- */
#define SBPM_M 8
__global__ void __launch_bounds__(SBP_RT)
k_sbpm_resolve(SbpJobs JS, int forceSeq) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& J = JS.job[blockIdx.x];
    const int M = min(JS.M, SBPM_M);
    const auto [nLast, nCur] = sbp_counts(J);
    int32_t* holder = (int32_t*)sbsm;
    int32_t* owner = holder + nCur;
    uint8_t* oct = (uint8_t*)(owner + nCur);
    __shared__ int s_changed, s_seq, s_nlog;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_seq = forceSeq;
        s_nlog = 0;
        s_changed = 0;
    }
    for (int c = tid; c < nCur; c += SBP_RT) {
        oct[c] = (uint8_t)J.curKps[c].octave;
        owner[c] = -1;
    }
    uint32_t keys[SBP_QPT][SBPM_M];
    int choice[SBP_QPT];
    bool blocking[SBP_QPT], full[SBP_QPT];
#pragma unroll
    for (int k = 0; k < SBP_QPT; k++) {
        const int q = tid + k * SBP_RT;
        choice[k] = -1;
        blocking[k] = q < nLast && (J.flags[q] & 2);
        full[k] = true;
#pragma unroll
        for (int j = 0; j < SBPM_M; j++) {
            keys[k][j] = (q < nLast && j < M) ? J.topm[(size_t)q * JS.M + j] : 0xFFFFFFFFu;
            if (j < M && keys[k][j] == 0xFFFFFFFFu) full[k] = false;
        }
    }
    __syncthreads();
    for (int round = 0; round < 1024 && !s_seq; round++) {
        for (int c = tid; c < nCur; c += SBP_RT) holder[c] = (J.occupied0 && J.occupied0[c]) ? -1 : 0x7FFFFFFF;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SBP_QPT; k++)
            if (choice[k] >= 0 && blocking[k]) atomicMin(&holder[choice[k]], tid + k * SBP_RT);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SBP_QPT; k++) {
            const int q = tid + k * SBP_RT;
            if (keys[k][0] == 0xFFFFFFFFu) continue; /* no candidates at all */
            int found = 0, best = -1, bd = 256, bl = -1, sd = 256, sl = -1;
#pragma unroll
            for (int j = 0; j < SBPM_M; j++) {
                const uint32_t key = keys[k][j];
                if (key == 0xFFFFFFFFu || found == 2) continue;
                const int c = (int)si_key_index(key);
                if (holder[c] < q) continue; /* held by an earlier query (or occupied from the start) */
                if (found == 0) {
                    best = c;
                    bd = (int)si_key_dist(key);
                    bl = oct[c];
                } else {
                    sd = (int)si_key_dist(key);
                    sl = oct[c];
                }
                found++;
            }
            int nc = -1;
            if (found == 0) {
                if (full[k]) s_seq = 1; /* free candidates may exist beyond the prefix */
            } else if (bd <= SBP_TH_HIGH) {
                if (found == 2) {
                    if (!(bl == sl && (float)bd > __fmul_rn(J.nnratio, (float)sd))) nc = best;
                } else if (!full[k]) {
                    nc = best; /* bestLevel2 stays -1 */
                } else {
                    uint32_t klast = 0xFFFFFFFFu;
#pragma unroll
                    for (int j = 0; j < SBPM_M; j++)
                        if (j == M - 1) klast = keys[k][j];
                    const int dlast = (int)si_key_dist(klast);
                    if ((float)bd <= __fmul_rn(J.nnratio, (float)dlast)) nc = best; /* whatever the second is */
                    else s_seq = 1;
                }
            }
            if (nc != choice[k]) {
                choice[k] = nc;
                s_changed = 1;
            }
        }
        __syncthreads();
        const int ch = s_changed;
        __syncthreads();
        if (tid == 0) s_changed = 0;
        if (!ch) break;
        if (round == 1023 && tid == 0) s_seq = 1;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) *J.needSeq = s_seq;
    if (s_seq) return;
#pragma unroll
    for (int k = 0; k < SBP_QPT; k++)
        if (choice[k] >= 0) {
            atomicMax(&owner[choice[k]], tid + k * SBP_RT); /* F.mvpMapPoints[bestIdx] = pMP: last writer */
            atomicAdd(&s_nlog, 1);
        }
    __syncthreads();
    for (int c = tid; c < nCur; c += SBP_RT) J.matchCur[c] = owner[c];
    if (tid == 0) J.nmatches[0] = s_nlog;
}

/* sequential cross-check / fallback of the same function: one wave, MapPoints in index order, every window
 * scanned in full (two smallest free keys by two wave reductions) */
__global__ void __launch_bounds__(64)
k_sbpm_replay(SbpJobs JS, int* fallbacks) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& J = JS.job[blockIdx.x];
    if (*J.needSeq == 0) return;
    const auto [nLast, nCur] = sbp_counts(J);
    uint32_t* occupied = (uint32_t*)sbsm;
    const int lane = threadIdx.x;
    const SiBounds bnd = J.bnd;
    const SiGridInv inv = si_grid_inv(bnd);
    for (int c = lane; c < nCur; c += 64) {
        occupied[c] = J.occupied0 ? J.occupied0[c] : 0u;
        J.matchCur[c] = -1;
    }
    __syncthreads();
    int nm = 0, nscan = 0;
    for (int q = 0; q < nLast; q++) {
        const SbpProj pr = J.proj[q];
        if (!pr.valid) continue;
        nscan++;
        const SiWindow win = si_window_b(pr.u, pr.v, pr.radius, bnd, inv);
        if (win.empty) continue;
        const uint4 da = ((const uint4*)J.mpDesc)[(size_t)q * 2], db = ((const uint4*)J.mpDesc)[(size_t)q * 2 + 1];
        uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu; /* this lane's two smallest free keys */
        for (int c = lane; c < nCur; c += 64) {
            const SbpCand cd = sbp_make_cand(J.curKps[c], J.uRight ? J.uRight[c] : -1.f, bnd, inv);
            if (cd.cell == 0xFFFF || occupied[c] || !sbp_candidate_ok(cd, win, pr)) continue;
            const uint4 ta = ((const uint4*)J.curDesc)[(size_t)c * 2], tb = ((const uint4*)J.curDesc)[(size_t)c * 2 + 1];
            const uint32_t key = si_key(si_hamming(da, db, ta, tb), cd.cell, (uint32_t)c);
            if (key < k1) { k2 = k1; k1 = key; }
            else if (key < k2) k2 = key;
        }
        const uint32_t g1 = wave_min_u32(k1);
        if (g1 == 0xFFFFFFFFu) continue;
        const uint32_t g2 = wave_min_u32(k1 == g1 ? k2 : k1);
        const int bd = (int)si_key_dist(g1), best = (int)si_key_index(g1);
        if (bd > SBP_TH_HIGH) continue;
        const int bl = J.curKps[best].octave;
        bool accept = true;
        if (g2 != 0xFFFFFFFFu) {
            const int sd = (int)si_key_dist(g2), sl = J.curKps[si_key_index(g2)].octave;
            if (bl == sl && (float)bd > __fmul_rn(J.nnratio, (float)sd)) accept = false;
        }
        if (!accept) continue;
        if (lane == 0) {
            J.matchCur[best] = q;
            if (J.flags[q] & 2) occupied[best] = 1u;
        }
        nm++;
        __syncthreads();
    }
    __syncthreads();
    if (lane == 0) {
        J.nmatches[0] = nm;
        if (fallbacks && nscan) atomicAdd(fallbacks, nscan);
    }
}

size_t vk_sbpm_resolve_lds(int nCur) { return (size_t)nCur * 9 + 16; }

size_t vk_sbp_resolve_lds(int nCur) { return (size_t)nCur * 8; }

void vk_search_by_projection(hipStream_t st, const SbpJobs& JS, int njobs, int maxLast, int maxCur, int* fallbacks,
                             int forceSeq) {
    if (njobs <= 0) return;
    if (maxLast > 0)
        hipLaunchKernelGGL(k_sbp_rank, dim3((maxLast + SBP_QPB - 1) / SBP_QPB, njobs), dim3(256),
                           vk_sbp_rank_lds(maxCur), st, JS);
    if (JS.job[0].mode == 1) {
        hipLaunchKernelGGL(k_sbpm_resolve, dim3(njobs), dim3(SBP_RT), vk_sbpm_resolve_lds(maxCur), st, JS, forceSeq);
        hipLaunchKernelGGL(k_sbpm_replay, dim3(njobs), dim3(64), (size_t)maxCur * 4, st, JS, fallbacks);
        return;
    }
    hipLaunchKernelGGL(k_sbp_resolve, dim3(njobs), dim3(SBP_RT), vk_sbp_resolve_lds(maxCur), st, JS, forceSeq);
    hipLaunchKernelGGL(k_sbp_replay, dim3(njobs), dim3(64), vk_sbp_replay_lds(maxCur, maxLast), st, JS, fallbacks);
}

/* the same with k_sbp_rank_kb8 in front: modes 2 and 3 of a fisheye frame / KeyFrame.  `between` (may be null) is recorded
 * behind the ranking */
void vk_search_by_projection_kb8(hipStream_t st, const SbpJobs& JS, int njobs, int maxLast, int maxCur, int* fallbacks,
                                 int forceSeq, const vslam_kb8_camera& cam, hipEvent_t between) {
    if (njobs <= 0) return;
    if (maxLast > 0)
        hipLaunchKernelGGL(k_sbp_rank_kb8, dim3((maxLast + SBP_QPB - 1) / SBP_QPB, njobs), dim3(256),
                           vk_sbp_rank_lds(maxCur), st, JS, cam);
    if (between) (void)hipEventRecord(between, st);
    hipLaunchKernelGGL(k_sbp_resolve, dim3(njobs), dim3(SBP_RT), vk_sbp_resolve_lds(maxCur), st, JS, forceSeq);
    hipLaunchKernelGGL(k_sbp_replay, dim3(njobs), dim3(64), vk_sbp_replay_lds(maxCur, maxLast), st, JS, fallbacks);
}

/* ------------------------------------------------------------------------------------------------
 * FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863) for fisheye KeyFrames:
 * ONE MapPoint list against up to 16 (KeyFrame, Scw) jobs.  The list is long (the MapPoints of a KeyFrame, of its covisibles
 * and of theirs) and the matcher behind takes 4096 queries, so the gates come first, as in SearchLocalPoints:
 *   k_s3k_gate     one thread per (job, point): everything up to the radius -- validity, Rcw * p + tcw as one gemm, z < 0,
 *                  KannalaBrandt8::project, KeyFrame::IsInImage over the integer bounds, the distance range, the viewing angle
 *                  (both sides in double), PredictScale -- into a projection record, and the survivors per chunk of 256 points
 *   k_s3k_compact  k_rig_compact's ranks: ballot / popcount over a running base of chunk counts, the list order kept; a job's
 *                  survivors get their record, descriptor, flags (3: every accepted point blocks its keypoint) and iMP.  A job
 *                  with more than `cap` survivors hands the matcher none
 *   k_sbp_rank_kb8 (mode 3), k_sbp_resolve, k_sbp_replay: one job each over its survivors
 *   k_s3k_finish   match_kf[idx]: the survivor's position -> its iMP; nmatches (-1: refused) and n_gated
 * ---------------------------------------------------------------------------------------------- */
#define S3K_CHUNK 256
__global__ void __launch_bounds__(S3K_CHUNK)
k_s3k_gate(Sim3Kb8Args A) {
    __shared__ int s_keep[4];
    const Sim3Kb8JobDev& J = A.job[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * S3K_CHUNK + tid;
    SbpProj pr = {};
    if (i < A.nPoints) {
        const FusePoint mp = A.pts[i];
        bool ok = mp.valid != 0 && (!J.valid || J.valid[i]); /* !pMP->isBad() && !spAlreadyFound.count(pMP) */
        const SbpPoint pc = sbp_transform(J.Rcw, J.tcw, mp.pos[0], mp.pos[1], mp.pos[2], A.gemmFloat);
        ok = ok && !(pc.z < 0.0f);
        const vslam_kb8::Uv uv = vslam_kb8::kb8_project(A.cam, pc.x, pc.y, pc.z);
        const SiBounds wb = si_kf_bounds(A.bnd);
        ok = ok && uv.u >= wb.minX && uv.u < wb.maxX && uv.v >= wb.minY && uv.v < wb.maxY; /* KeyFrame::IsInImage */
        const float p0 = __fsub_rn(mp.pos[0], J.Ow[0]), p1 = __fsub_rn(mp.pos[1], J.Ow[1]), p2 = __fsub_rn(mp.pos[2], J.Ow[2]);
        const float dist = vslam_md::norm3(p0, p1, p2);
        ok = ok && !(dist < mp.minDistance || dist > mp.maxDistance);
        ok = ok && !(vslam_md::dot3_mat(p0, p1, p2, mp.normal) < __dmul_rn(0.5, (double)dist));
        if (ok) {
            const int level = vslam_md::predict_level(mp.maxDistance, dist, A.logScaleFactor, A.nlevels);
            pr.u = uv.u;
            pr.v = uv.v;
            pr.radius = __fmul_rn(A.th, A.scale[level]);
            pr.minLevel = level - 1;
            pr.maxLevel = level;
            pr.valid = 1;
        }
        A.gate[(size_t)blockIdx.y * A.nPoints + i] = pr;
    }
    const unsigned long long bk = __ballot(pr.valid != 0);
    if (lane == 0) s_keep[wave] = __popcll(bk);
    __syncthreads();
    if (tid == 0) A.chunkKeep[blockIdx.y * A.nchunks + blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
}

__global__ void __launch_bounds__(S3K_CHUNK)
k_s3k_compact(Sim3Kb8Args A) {
    __shared__ int s_before[4], s_wave[4];
    const Sim3Kb8JobDev& J = A.job[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    /* chunk counts: thread t holds chunk t (nchunks <= 256) */
    int before = tid < b ? A.chunkKeep[blockIdx.y * A.nchunks + tid] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    const int i = b * S3K_CHUNK + tid;
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0; /* the record as two 16-byte words: u, v, radius, ur | minLevel, maxLevel, valid, - */
    if (i < A.nPoints) {
        const uint4* g = (const uint4*)(A.gate + (size_t)blockIdx.y * A.nPoints + i);
        r0 = g[0];
        r1 = g[1];
    }
    const bool keep = r1.z != 0;
    const unsigned long long bk = __ballot(keep);
    const int rank = __popcll(bk & ((1ull << lane) - 1ull));
    if (lane == 0) {
        s_before[wave] = before;
        s_wave[wave] = __popcll(bk);
    }
    __syncthreads();
    const int base = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    int woff = 0;
    for (int w = 0; w < wave; w++) woff += s_wave[w];
    const int pos = base + woff + rank;
    if (keep && pos < A.cap) {
        ((uint4*)(J.projC + pos))[0] = r0;
        ((uint4*)(J.projC + pos))[1] = r1;
        const uint4* src = (const uint4*)(A.mpDesc + (size_t)i * 32);
        uint4* dst = (uint4*)(J.descC + (size_t)pos * 32);
        dst[0] = src[0];
        dst[1] = src[1];
        J.flagsC[pos] = 3; /* bit 0: a query; bit 1: vpMatched[bestIdx] = pMP blocks later points */
        J.indexC[pos] = i;
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        const int kept = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        A.counts[blockIdx.y * 4] = kept;
        A.counts[blockIdx.y * 4 + 1] = kept > A.cap ? 0 : kept;
    }
}

__global__ void __launch_bounds__(256)
k_s3k_finish(Sim3Kb8Args A) {
    const Sim3Kb8JobDev& J = A.job[blockIdx.x];
    const int kept = A.counts[blockIdx.x * 4];
    const bool refused = kept > A.cap;
    for (int c = threadIdx.x; c < J.nKF; c += 256) {
        const int m = J.matchKf[c];
        J.matchKf[c] = (refused || m < 0) ? -1 : J.indexC[m];
    }
    if (threadIdx.x == 0) {
        if (refused) A.result[blockIdx.x * 2] = -1;
        A.result[blockIdx.x * 2 + 1] = kept;
    }
}

void vk_search_sim3_kb8(hipStream_t st, const Sim3Kb8Args& A, const SbpJobs& JS, int njobs, int maxKF, int* fallbacks,
                        int forceSeq, hipEvent_t after_compact, hipEvent_t after_rank) {
    if (njobs <= 0 || A.nPoints <= 0) return;
    hipLaunchKernelGGL(k_s3k_gate, dim3(A.nchunks, njobs), dim3(S3K_CHUNK), 0, st, A);
    hipLaunchKernelGGL(k_s3k_compact, dim3(A.nchunks, njobs), dim3(S3K_CHUNK), 0, st, A);
    if (after_compact) (void)hipEventRecord(after_compact, st);
    vk_search_by_projection_kb8(st, JS, njobs, A.cap, maxKF, fallbacks, forceSeq, A.cam, after_rank);
    hipLaunchKernelGGL(k_s3k_finish, dim3(njobs), dim3(256), 0, st, A);
}

/* ------------------------------------------------------------------------------------------------
 * SearchByProjection(Frame& F, const vector<MapPoint*>&, th, ...) for a two-fisheye rig (fmatcher.cpp:321-491 with
 * Nleft != -1).  All the Hamming work is k_sbp_rank mode 1, unedited, as two jobs of one launch: job 0 ranks the compacted
 * MapPoints against the left keypoints with the caller's th, job 1 against the right keypoints with th = 1 (the bFactor line
 * is missing at :425).  What is left is sequential and couples the two sides:
 *   - a slot of F.mvpMapPoints (Nleft + Nright of them) is occupied iff its LAST writer has observations: a direct write
 *     lands on a free slot only, but the cross-writes through mvLeftToRightMatch / mvRightToLeftMatch (:409-413, :476-480) land
 *     anywhere, so a point without observations frees a slot again;
 *   - the left ratio failure is a `continue` (:403-404): it skips the right branch of the same point;
 *   - the right branch sees what the left branch of the same point has just written.
 * k_rig_resolve is one wave that walks the points in order, as k_sbp_replay does: per point and side two ballots over the
 * sorted prefix (valid, free) give best and second best; occupancy, keypoint octaves, both match maps and the slot owners of
 * BOTH sides live in LDS.  When a block of 64 points is loaded, every prefix entry gathers its keypoint's octave and match-map
 * entry beside its key, and the next point's entries are read while the current one is resolved, so that per point and side only
 * the occupancy read and the write behind it wait for the point before.  A prefix that cannot decide -- it is full and holds fewer than two free entries, and neither
 * "best is beyond TH_HIGH" nor "best passes the ratio test against the prefix's last entry, so against any second" settles
 * it -- is re-scanned in full (rig_full_scan2, the loop body of the reference).  forceSeq (sbp_sequential = 1) re-scans every
 * window and reads no prefix at all: the cross-check path.  Blocks of 64 points: the points without a candidate on either
 * side cost one ballot per block.
 * ---------------------------------------------------------------------------------------------- */
struct RigTwo { /* the two smallest free keys of a window, ~0 = none */
    uint32_t g1, g2;
};
__device__ RigTwo rig_full_scan2(const SbpProj& pr, const SbpJobDev& J, int nCur, const uint8_t* mpDescQ, const uint8_t* occ,
                                 const SiBounds& bnd, const SiGridInv& inv, int lane) {
    uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
    const SiWindow win = si_window_b(pr.u, pr.v, pr.radius, bnd, inv);
    if (!win.empty) {
        const uint4 da = ((const uint4*)mpDescQ)[0], db = ((const uint4*)mpDescQ)[1];
        for (int c = lane; c < nCur; c += 64) {
            const SbpCand cd = sbp_make_cand(J.curKps[c], -1.f, bnd, inv); /* no mvuRight gate in a rig (:370) */
            if (cd.cell == 0xFFFF || occ[c] || !sbp_candidate_ok(cd, win, pr)) continue;
            const uint4 ta = ((const uint4*)J.curDesc)[(size_t)c * 2], tb = ((const uint4*)J.curDesc)[(size_t)c * 2 + 1];
            const uint32_t key = si_key(si_hamming(da, db, ta, tb), cd.cell, (uint32_t)c);
            if (key < k1) { k2 = k1; k1 = key; }
            else if (key < k2) k2 = key;
        }
    }
    RigTwo r;
    r.g1 = wave_min_u32(k1);
    r.g2 = r.g1 == 0xFFFFFFFFu ? 0xFFFFFFFFu : wave_min_u32(k1 == r.g1 ? k2 : k1);
    return r;
}

/* one side of one point: best = -1 nothing to assign (the reference falls through), -2 the ratio test failed (`continue`), else
 * the keypoint to assign and cross = its entry of mvLeftToRightMatch / mvRightToLeftMatch; scanned = 1 if the window was
 * re-scanned.  key, meta: this lane's entry of the point's sorted prefix (lanes >= M hold ~0) and, gathered when the block of
 * points was loaded, that keypoint's octave | match-map entry << 8: best and second best then come out of two ballots and
 * register reads, and the only LDS read that waits for the point before is the occupancy.  oct, cross: the same two tables
 * in LDS, for a re-scanned window.  All results wave-uniform, and by value (vslam_matchdev.h). */
struct RigPick {
    int best, cross, scanned;
};
__device__ RigPick rig_side(uint32_t key, uint32_t meta, int M, int forceSeq, const SbpJobDev& J, int nCur, int q,
                            const uint8_t* occ, const uint8_t* oct, const int16_t* cross, const SiBounds& bnd,
                            const SiGridInv& inv, int lane) {
    if (!forceSeq) {
        const bool valid = key != 0xFFFFFFFFu;
        const bool fr = valid && !occ[si_key_index(key)];
        const unsigned long long mv = __ballot(valid), mf = __ballot(fr);
        if (mv == 0) return RigPick{-1, -1, 0}; /* vIndices empty, or every candidate failed an order-free gate */
        const bool full = __popcll(mv) >= M;
        const int nfree = __popcll(mf);
        bool decided = !full || nfree >= 2; /* a complete list: bestDist2 stays 256 and bestLevel2 -1 where it runs out */
        uint32_t g1 = 0xFFFFFFFFu, m1 = 0;
        if (mf) {
            const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)mf) - 1);
            g1 = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
            m1 = (uint32_t)__builtin_amdgcn_readlane((int)meta, first);
        }
        const uint32_t bd = si_key_dist(g1);
        if (!decided && nfree == 1) {
            /* beyond TH_HIGH nothing is assigned; or the best passes the ratio test against the prefix's last entry, and so
             * against every possible second, whatever its level */
            const uint32_t dlast = si_key_dist((uint32_t)__builtin_amdgcn_readlane((int)key, M - 1));
            decided = bd > (uint32_t)SBP_TH_HIGH || (float)bd <= __fmul_rn(J.nnratio, (float)dlast);
        }
        if (decided) {
            if (!mf || bd > (uint32_t)SBP_TH_HIGH) return RigPick{-1, -1, 0};
            if (nfree >= 2) {
                const unsigned long long mf2 = mf & (mf - 1ull);
                const int second = __builtin_amdgcn_readfirstlane(__ffsll((long long)mf2) - 1);
                const uint32_t g2 = (uint32_t)__builtin_amdgcn_readlane((int)key, second);
                const uint32_t m2 = (uint32_t)__builtin_amdgcn_readlane((int)meta, second);
                if ((m1 & 0xFFu) == (m2 & 0xFFu) && (float)bd > __fmul_rn(J.nnratio, (float)si_key_dist(g2)))
                    return RigPick{-2, -1, 0};
            }
            return RigPick{(int)si_key_index(g1), (int)(int16_t)(m1 >> 8), 0};
        }
    }
    const SbpProj pr = J.proj[q];
    if (!pr.valid) return RigPick{-1, -1, 0};
    const RigTwo t = rig_full_scan2(pr, J, nCur, J.mpDesc + (size_t)q * 32, occ, bnd, inv, lane);
    if (t.g1 == 0xFFFFFFFFu) return RigPick{-1, -1, 1};
    const int bd = (int)si_key_dist(t.g1), best = (int)si_key_index(t.g1);
    if (bd > SBP_TH_HIGH) return RigPick{-1, -1, 1};
    if (t.g2 != 0xFFFFFFFFu) {
        const int sd = (int)si_key_dist(t.g2);
        if (oct[best] == oct[si_key_index(t.g2)] && (float)bd > __fmul_rn(J.nnratio, (float)sd)) return RigPick{-2, -1, 1};
    }
    return RigPick{best, (int)cross[best], 1};
}

#define RIG_LDS_KEYS (2 * 64 * SI_MAX_M * 8)
__global__ void __launch_bounds__(64)
k_rig_resolve(SbpJobs JS, RigResolveDev A) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& JL = JS.job[0];
    const SbpJobDev& JR = JS.job[1];
    const int M = JS.M;
    const int nL = A.nLeft, nR = A.nRight, N = nL + nR;
    const int nMp = sbp_counts(JL).nLast;
    uint2* kbufL = (uint2*)sbsm;                  /* 64 x M: (key, octave | match-map entry << 8) of a block's left prefixes */
    uint2* kbufR = kbufL + 64 * SI_MAX_M;         /* 64 x M: the right ones */
    int16_t* owner = (int16_t*)(sbsm + RIG_LDS_KEYS); /* N: last point written to the slot (compacted index < 4096), -1 */
    int16_t* cross = owner + N;                   /* N: mvLeftToRightMatch | mvRightToLeftMatch */
    uint8_t* occ = (uint8_t*)(cross + N);         /* N: the slot holds a MapPoint with Observations() > 0 */
    uint8_t* oct = occ + N;                       /* N: keypoint octaves */
    const int lane = threadIdx.x;
    const SiBounds bnd = JL.bnd;
    const SiGridInv inv = si_grid_inv(bnd);
    for (int c = lane; c < N; c += 64) {
        owner[c] = -1;
        cross[c] = (int16_t)(c < nL ? A.leftToRight[c] : A.rightToLeft[c - nL]);
        occ[c] = (A.occupied0 && A.occupied0[c]) ? 1 : 0;
        oct[c] = (uint8_t)(c < nL ? JL.curKps[c].octave : JR.curKps[c - nL].octave);
    }
    __syncthreads();
    const uint2 none = make_uint2(0xFFFFFFFFu, 0u);
    int nm = 0, nfb = 0;
    for (int qb = 0; qb < nMp; qb += 64) {
        const int nq = min(64, nMp - qb);
        __syncthreads();
        if (!A.forceSeq)
            for (int i = lane; i < nq * M; i += 64) {
                const uint32_t kl = JL.topm[(size_t)qb * M + i], kr = JR.topm[(size_t)qb * M + i];
                const int il = (int)si_key_index(kl), ir = nL + (int)si_key_index(kr);
                kbufL[i] = kl == 0xFFFFFFFFu ? none : make_uint2(kl, oct[il] | ((uint32_t)(uint16_t)cross[il] << 8));
                kbufR[i] = kr == 0xFFFFFFFFu ? none : make_uint2(kr, oct[ir] | ((uint32_t)(uint16_t)cross[ir] << 8));
            }
        const uint32_t myflags = lane < nq ? JL.flags[qb + lane] : 0u; /* lane t holds point qb + t's flags */
        __syncthreads();
        bool anyL, anyR;
        if (A.forceSeq) {
            anyL = lane < nq && JL.proj[qb + lane].valid;
            anyR = lane < nq && JR.proj[qb + lane].valid;
        } else {
            anyL = lane < nq && kbufL[lane * M].x != 0xFFFFFFFFu;
            anyR = lane < nq && kbufR[lane * M].x != 0xFFFFFFFFu;
        }
        const unsigned long long mL = __ballot(anyL), mR = __ballot(anyR);
        unsigned long long todo = mL | mR;
        /* the next point's prefixes are read while the current one is resolved: they do not depend on it */
        uint2 nxL = none, nxR = none;
        if (todo && !A.forceSeq && lane < M) {
            const int t0 = __ffsll((long long)todo) - 1;
            nxL = kbufL[t0 * M + lane];
            nxR = kbufR[t0 * M + lane];
        }
        while (todo) {
            const int tq = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            todo &= todo - 1ull;
            const uint2 eL = nxL, eR = nxR;
            if (todo && !A.forceSeq && lane < M) {
                const int t1 = __ffsll((long long)todo) - 1;
                nxL = kbufL[t1 * M + lane];
                nxR = kbufR[t1 * M + lane];
            }
            const int q = qb + tq;
            const uint8_t blk = (__builtin_amdgcn_readlane((int)myflags, tq) & 2) ? 1 : 0;
            if ((mL >> tq) & 1ull) { /* the left branch, fmatcher.cpp:339-420 */
                const RigPick pk = rig_side(eL.x, eL.y, M, A.forceSeq, JL, nL, q, occ, oct, cross, bnd, inv, lane);
                nfb += pk.scanned;
                if (pk.best == -2) continue; /* :403-404 skips the right branch as well */
                if (pk.best >= 0) {
                    if (lane == 0) {
                        owner[pk.best] = (int16_t)q;
                        occ[pk.best] = blk;
                        if (pk.cross != -1) { /* :409-413: the slot is not looked at */
                            owner[nL + pk.cross] = (int16_t)q;
                            occ[nL + pk.cross] = blk;
                        }
                    }
                    nm += pk.cross != -1 ? 2 : 1;
                    __syncthreads();
                }
            }
            if ((mR >> tq) & 1ull) { /* the right branch, :422-488 */
                const RigPick pk = rig_side(eR.x, eR.y, M, A.forceSeq, JR, nR, q, occ + nL, oct + nL, cross + nL, bnd, inv, lane);
                nfb += pk.scanned;
                if (pk.best >= 0) {
                    if (lane == 0) {
                        if (pk.cross != -1) { /* :476-480 */
                            owner[pk.cross] = (int16_t)q;
                            occ[pk.cross] = blk;
                        }
                        owner[nL + pk.best] = (int16_t)q;
                        occ[nL + pk.best] = blk;
                    }
                    nm += pk.cross != -1 ? 2 : 1;
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();
    for (int c = lane; c < N; c += 64) A.matchCur[c] = owner[c];
    if (lane == 0) {
        A.nmatches[0] = nm;
        if (A.fallbacks && nfb) atomicAdd(A.fallbacks, nfb);
    }
}

size_t vk_rig_resolve_lds(int nSlots) { return (size_t)RIG_LDS_KEYS + (size_t)nSlots * 6; }

void vk_search_rig(hipStream_t st, const SbpJobs& JS, const RigResolveDev& A, int maxMp, hipEvent_t between) {
    if (maxMp <= 0) return;
    hipLaunchKernelGGL(k_sbp_rank, dim3((maxMp + SBP_QPB - 1) / SBP_QPB, 2), dim3(256),
                       vk_sbp_rank_lds(max(A.nLeft, A.nRight)), st, JS);
    if (between) (void)hipEventRecord(between, st);
    hipLaunchKernelGGL(k_rig_resolve, dim3(1), dim3(64), vk_rig_resolve_lds(A.nLeft + A.nRight), st, JS, A);
}

/* ------------------------------------------------------------------------------------------------
 * SearchByProjection(CurrentFrame, LastFrame) for a two-fisheye rig (fmatcher.cpp:2494-2684 with Nleft != -1), behind
 * k_sbp_rank_rig.  The left branch writes slots [0, nLeft) only and reads the occupancy of those alone, the right branch
 * [nLeft, nLeft + nRight): each side by itself is the serial dictatorship k_sbp_resolve solves.  What couples them is order-free:
 *   - the left branch's three `continue`s (invzc < 0, uv outside the bounds, vIndices2 empty) skip the right branch of the same
 *     query.  A left record that is not valid leaves an empty prefix, and without an mvuRight gate the prefix is empty iff
 *     vIndices2 is: "the left prefix's first key is ~0" is all three.  A left window whose candidates are all occupied has a
 *     first key, and the right branch runs (bestDist stays 256 and control falls through to :2593).
 *   - ONE rotation histogram and one nmatches over the entries of both sides.
 * k_sbp_rig_resolve is k_sbp_resolve's fixpoint over both sides at once in one workgroup: a thread holds four left and four
 * right queries, holder / owner are indexed by slot, and the finish -- last writer per slot, histogram, three maxima, nmatches
 * -- runs over both.  A query that runs off a FULL prefix hands the call to k_sbp_rig_replay: one wave, the left queries in
 * order, then the right ones (the sides do not see each other's writes), full re-scans where a prefix is exhausted; with
 * forceSeq (sbp_sequential = 1) it reads no prefix but the left first keys and re-scans every window.
 * ---------------------------------------------------------------------------------------------- */
#define SBP_RIG_QPT (2 * SBP_QPT)
__global__ void __launch_bounds__(SBP_RT)
k_sbp_rig_resolve(SbpJobs JS, RigFrameDev R) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& JL = JS.job[0];
    const SbpJobDev& JR = JS.job[1];
    const int M = JS.M;
    const int nLast = sbp_counts(JL).nLast;
    const int nL = R.nLeft, N = R.nLeft + R.nRight;
    int32_t* holder = (int32_t*)sbsm; /* N slots: lowest-index blocking query of the slot's side pointing here; -1 = occupied from the start */
    int32_t* owner = holder + N;      /* N slots: highest-index query assigned here */
    __shared__ int s_changed, s_seq, s_nlog, s_removed;
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_seq = R.forceSeq;
        s_nlog = 0;
        s_removed = 0;
    }
    if (tid < VSLAM_HISTO_LENGTH) s_hist[tid] = 0;
    for (int c = tid; c < N; c += SBP_RT) {
        holder[c] = (R.occupied0 && R.occupied0[c]) ? -1 : 0x7FFFFFFF;
        owner[c] = -1;
    }
    /* k < SBP_QPT: left query tid + k * SBP_RT; k >= SBP_QPT: the right branch of query tid + (k - SBP_QPT) * SBP_RT */
    uint32_t key[SBP_RIG_QPT];
    int ptr[SBP_RIG_QPT];
    bool blocking[SBP_QPT];
#pragma unroll
    for (int k = 0; k < SBP_QPT; k++) {
        const int q = tid + k * SBP_RT;
        ptr[k] = ptr[k + SBP_QPT] = 0;
        key[k] = q < nLast ? JL.topm[(size_t)q * M] : 0xFFFFFFFFu;
        /* a left `continue` (:2509-2517, :2534-2535) skips the right branch */
        key[k + SBP_QPT] = key[k] != 0xFFFFFFFFu ? JR.topm[(size_t)q * M] : 0xFFFFFFFFu;
        blocking[k] = q < nLast && (JL.flags[q] & 2);
    }
    __syncthreads();
    for (int round = 0; round < 4096 && !s_seq; round++) { /* s_seq / s_changed are block-uniform at the barriers */
        if (tid == 0) s_changed = 0;
#pragma unroll
        for (int k = 0; k < SBP_RIG_QPT; k++)
            if (key[k] != 0xFFFFFFFFu && blocking[k % SBP_QPT] && si_key_dist(key[k]) <= (uint32_t)SBP_TH_HIGH)
                atomicMin(&holder[(k < SBP_QPT ? 0 : nL) + (int)si_key_index(key[k])], tid + (k % SBP_QPT) * SBP_RT);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SBP_RIG_QPT; k++) {
            const int q = tid + (k % SBP_QPT) * SBP_RT;
            const SbpJobDev& J = k < SBP_QPT ? JL : JR;
            if (key[k] != 0xFFFFFFFFu && holder[(k < SBP_QPT ? 0 : nL) + (int)si_key_index(key[k])] < q) {
                ptr[k]++;
                if (ptr[k] >= M) {
                    s_seq = 1; /* ran off a full prefix */
                    key[k] = 0xFFFFFFFFu;
                } else {
                    key[k] = J.topm[(size_t)q * M + ptr[k]]; /* ~0: the list is complete and exhausted */
                }
                s_changed = 1;
            }
        }
        __syncthreads();
        if (!s_changed) break;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) *R.needSeq = s_seq;
    if (s_seq) return;
    /* the joint finish: both sides' assignments into one log */
    uint32_t bin[SBP_RIG_QPT];
#pragma unroll
    for (int k = 0; k < SBP_RIG_QPT; k++) {
        const int q = tid + (k % SBP_QPT) * SBP_RT;
        const SbpJobDev& J = k < SBP_QPT ? JL : JR;
        bin[k] = 255;
        if (key[k] != 0xFFFFFFFFu && si_key_dist(key[k]) <= (uint32_t)SBP_TH_HIGH) {
            const int i2 = (int)si_key_index(key[k]);
            atomicMax(&owner[(k < SBP_QPT ? 0 : nL) + i2], q);
            atomicAdd(&s_nlog, 1);
            bin[k] = 254;
            if (JL.checkOri) { /* kpLF: keypoints_[i] | keypointsRight_[i - Nleft], the caller's one array; kpCF of the side */
                const int b = vslam_md::rot_bin(JL.lastKps[q].angle, J.curKps[i2].angle, VSLAM_HISTO_LENGTH);
                bin[k] = (uint32_t)b;
                atomicAdd(&s_hist[b], 1);
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < N; c += SBP_RT) R.matchCur[c] = owner[c];
    __syncthreads();
    if (JL.checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
#pragma unroll
        for (int k = 0; k < SBP_RIG_QPT; k++) {
            const int b = (int)bin[k];
            if (b < VSLAM_HISTO_LENGTH && !vslam_md::keeps_bin(mx, b)) { /* fmatcher.cpp:2668-2681 */
                R.matchCur[(k < SBP_QPT ? 0 : nL) + (int)si_key_index(key[k])] = -1;
                atomicAdd(&s_removed, 1);
            }
        }
    }
    __syncthreads();
    if (tid == 0) R.nmatches[0] = s_nlog - s_removed;
}

__global__ void __launch_bounds__(64)
k_sbp_rig_replay(SbpJobs JS, RigFrameDev R) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    const SbpJobDev& JL = JS.job[0];
    const SbpJobDev& JR = JS.job[1];
    const int M = JS.M;
    const int nLast = sbp_counts(JL).nLast;
    const int nL = R.nLeft, N = R.nLeft + R.nRight;
    uint32_t* occupied = (uint32_t*)sbsm;            /* N: the slot holds a MapPoint with Observations() > 0 */
    int32_t* ownerEntry = (int32_t*)(occupied + N);  /* N: last log entry that wrote the slot */
    uint32_t* alog = (uint32_t*)(ownerEntry + N);    /* 2 * nLast: (query << 13 | slot), left entries first */
    uint8_t* logBin = (uint8_t*)(alog + 2 * nLast);  /* 2 * nLast: rotation bin of a log entry */
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    const int lane = threadIdx.x;
    if (*R.needSeq == 0) return; /* k_sbp_rig_resolve finished the call */
    const SiBounds bnd = JL.bnd;
    const SiGridInv inv = si_grid_inv(bnd);
    for (int c = lane; c < N; c += 64) {
        occupied[c] = (R.occupied0 && R.occupied0[c]) ? 1u : 0u;
        ownerEntry[c] = -1;
        R.matchCur[c] = -1;
    }
    if (lane < VSLAM_HISTO_LENGTH) s_hist[lane] = 0;
    __syncthreads();
    int nlog = 0, nfb = 0;
    for (int side = 0; side < 2; side++) {
        const SbpJobDev& J = side ? JR : JL;
        const int base = side ? nL : 0, nCur = side ? R.nRight : nL;
        for (int qb = 0; qb < nLast; qb += 64) {
            const int nq = min(64, nLast - qb);
            /* lane t: query qb + t is not walked -- the left branch left by a `continue`, or (no prefix read) nothing to scan */
            bool skip = lane >= nq || JL.topm[(size_t)(qb + lane) * M] == 0xFFFFFFFFu;
            if (!skip && R.forceSeq) skip = !J.proj[qb + lane].valid;
            const unsigned long long todo = ~__ballot(skip);
            const uint32_t myflags = lane < nq ? J.flags[qb + lane] : 0u;
            for (int tq = 0; tq < nq; tq++) {
                if (!((todo >> tq) & 1ull)) continue;
                const int q = qb + tq;
                uint32_t gBest = 0xFFFFFFFFu;
                bool scan = R.forceSeq != 0;
                if (!scan) {
                    const uint32_t key = lane < M ? J.topm[(size_t)q * M + lane] : 0xFFFFFFFFu;
                    const bool valid = key != 0xFFFFFFFFu;
                    const bool fr = valid && !occupied[base + (int)si_key_index(key)];
                    const unsigned long long mv = __ballot(valid), mk = __ballot(fr);
                    if (mv == 0) continue; /* the right window holds nothing */
                    if (mk) {
                        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
                        gBest = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
                    } else if (__popcll(mv) < M) {
                        continue; /* the list is complete and every entry is occupied: bestDist stays 256 */
                    } else {
                        scan = true;
                    }
                }
                if (scan) {
                    nfb++;
                    gBest = sbp_full_scan(J.proj[q], J.curKps, nullptr, nCur, J.mpDesc + (size_t)q * 32, J.curDesc, occupied + base,
                                          bnd, bnd, inv, lane);
                }
                if (gBest == 0xFFFFFFFFu || si_key_dist(gBest) > (uint32_t)SBP_TH_HIGH) continue;
                const uint32_t slot = (uint32_t)base + si_key_index(gBest);
                const uint32_t fl = (uint32_t)__builtin_amdgcn_readlane((int)myflags, tq);
                if (lane == 0) {
                    alog[nlog] = ((uint32_t)q << 13) | slot;
                    if (fl & 2) occupied[slot] = 1u; /* pMP->Observations() > 0: later queries of this side skip the slot */
                }
                nlog++;
                __syncthreads(); /* one wave: orders lane 0's write before the next query's reads */
            }
        }
    }
    __syncthreads();
    if (R.fallbacks && lane == 0 && nfb) atomicAdd(R.fallbacks, nfb);
    for (int e = lane; e < nlog; e += 64) atomicMax(&ownerEntry[alog[e] & 0x1FFF], e);
    __syncthreads();
    for (int e = lane; e < nlog; e += 64) {
        const uint32_t le = alog[e];
        const int q = (int)(le >> 13), slot = (int)(le & 0x1FFF);
        if (ownerEntry[slot] == e) R.matchCur[slot] = q;
        if (JL.checkOri) {
            const float ang = slot < nL ? JL.curKps[slot].angle : JR.curKps[slot - nL].angle;
            const int bin = vslam_md::rot_bin(JL.lastKps[q].angle, ang, VSLAM_HISTO_LENGTH);
            logBin[e] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1);
        }
    }
    __syncthreads();
    int removed = 0;
    if (JL.checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
        for (int e = lane; e < nlog; e += 64) {
            if (!vslam_md::keeps_bin(mx, logBin[e])) {
                R.matchCur[alog[e] & 0x1FFF] = -1;
                removed++;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) removed += __shfl_xor(removed, o, 64);
    if (lane == 0) R.nmatches[0] = nlog - removed;
}

size_t vk_sbp_rig_resolve_lds(int nSlots) { return (size_t)nSlots * 8; }
size_t vk_sbp_rig_replay_lds(int nSlots, int nLast) { return (size_t)nSlots * 8 + (size_t)nLast * 10; }

void vk_search_frame_rig(hipStream_t st, const SbpJobs& JS, const RigFrameDev& R, int nLast, hipEvent_t between) {
    if (nLast <= 0) return;
    hipLaunchKernelGGL(k_sbp_rank_rig, dim3((nLast + SBP_QPB - 1) / SBP_QPB, 2), dim3(256),
                       vk_sbp_rank_lds(max(R.nLeft, R.nRight)), st, JS, R);
    if (between) (void)hipEventRecord(between, st);
    hipLaunchKernelGGL(k_sbp_rig_resolve, dim3(1), dim3(SBP_RT), vk_sbp_rig_resolve_lds(R.nLeft + R.nRight), st, JS, R);
    hipLaunchKernelGGL(k_sbp_rig_replay, dim3(1), dim3(64), vk_sbp_rig_replay_lds(R.nLeft + R.nRight, nLast), st, JS, R);
}

/* ------------------------------------------------------------------------------------------------
 * Frame::UnprojectStereo (frame.cpp:1023-1037) for every left keypoint of up to VSLAM_MAX_SBP_JOBS stereo
 * pairs: z = mvDepth[i] > 0  ->  x3Dc = ((u-cx)*z*invfx, (v-cy)*z*invfy, z), x3Dw = mRwc*x3Dc + mOw (one
 * cv::gemm, sbp_transform).  These are the points UpdateLastFrame turns into (temporal) MapPoints for
 * TrackWithMotionModel, i.e. the last-frame side of SearchByProjection; flags = has-a-point | observations.
 * ---------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256)
k_unproject_stereo(UnprojJobs U) {
    const UnprojJob& J = U.job[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(*J.nPtr, U.cap);
    if (i >= U.cap) return;
    float X = 0.f, Y = 0.f, Z = 0.f;
    uint8_t fl = 0;
    if (i < n) {
        const float z = J.depth[i];
        if (z > 0.f) {
            const vslam_kp k = J.kps[i];
            const float x = __fmul_rn(__fmul_rn(__fsub_rn(k.x, U.cx), z), U.invfx);
            const float y = __fmul_rn(__fmul_rn(__fsub_rn(k.y, U.cy), z), U.invfy);
            const SbpPoint w = sbp_transform(J.Twc, x, y, z, U.gemmFloat);
            X = w.x;
            Y = w.y;
            Z = w.z;
            fl = (uint8_t)(1 | (U.observations ? 2 : 0));
        }
    }
    J.x3Dw[3 * i] = X;
    J.x3Dw[3 * i + 1] = Y;
    J.x3Dw[3 * i + 2] = Z;
    J.flags[i] = fl;
}

void vk_unproject_stereo(hipStream_t st, const UnprojJobs& U, int njobs) {
    if (njobs <= 0) return;
    hipLaunchKernelGGL(k_unproject_stereo, dim3((U.cap + 255) / 256, njobs), dim3(256), 0, st, U);
}

/* ------------------------------------------------------------------------------------------------
 * The search half of FMatcher::Fuse (fmatcher.cpp:1918-2119 with bRight = false; Sim3 overload :2121-2243):
 * per MapPoint  Rcw*p + tcw (one cv::gemm, sbp_transform), depth >= 0, Pinhole::project, KeyFrame::IsInImage,
 * cv::norm(p - Ow) inside the scale-invariance range, viewing angle (cv::Mat::dot, both accumulate in double),
 * MapPoint::PredictScale (mappoint.cpp:506-521: ceil(logf(max/dist) / mfLogScaleFactor), glibc logf), radius =
 * th * scale[level], KeyFrame::GetFeaturesInArea (keyframe.cpp:656-699), level gate, chi2 gate (7.8 with a right
 * coordinate, 5.99 without; not in the Sim3 overload), then the least Hamming distance, first of the window order
 * wins: key = dist << 24 | cell << 12 | index -> wave min.  Nothing here depends on other MapPoints; the map
 * mutation that follows in the reference (Replace / AddObservation / vpReplacePoint) stays with the caller.
 * One wave per MapPoint, the KeyFrame's keypoints in LDS as for SearchByProjection.
 * ---------------------------------------------------------------------------------------------- */
#define FUSE_QPB 16
__global__ void __launch_bounds__(256)
k_fuse_rank(FuseArgsDev A) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    SbpCand* cand = (SbpCand*)sbsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SiBounds bnd = A.bnd;               /* Frame::mnMinX..: the cells of the grid the KeyFrame copied */
    const SiBounds kbnd = si_kf_bounds(bnd);  /* the KeyFrame's integer copy (keyframe.cpp:44): window origin, IsInImage */
    const SiGridInv inv = si_grid_inv(bnd);
    for (int i = tid; i < A.nKF; i += 256) cand[i] = sbp_make_cand(A.kfKps[i], A.kfURight[i], bnd, inv);
    __syncthreads();
    for (int q = blockIdx.x * FUSE_QPB + wave; q < min(A.nPoints, (int)(blockIdx.x + 1) * FUSE_QPB); q += 4) {
        const FusePoint mp = A.pts[q];
        uint32_t best = 0xFFFFFFFFu;
        uint32_t far = 0xFFFFFFFFu; /* cell << 12 | index of the first candidate at distance 256, which the key cannot hold */
        bool go = mp.valid != 0;
        float u = 0.f, v = 0.f, ur = 0.f, radius = 0.f;
        int level = 0;
        if (go && A.sim3 == 2) { /* SearchBySim3, one direction (fmatcher.cpp:2301-2332 / :2381-2412) */
            const SbpPoint p1 = sbp_transform(A.Rcw, A.tcw, mp.pos[0], mp.pos[1], mp.pos[2], A.gemmFloat);
            const SbpPoint pc = sbp_transform(A.Rb, A.tb, p1.x, p1.y, p1.z, A.gemmFloat);
            const float xc = pc.x, yc = pc.y, zc = pc.z;
            go = !(zc < 0.0f);
            if (go) {
                const float invz = (float)__ddiv_rn(1.0, (double)zc); /* const float invz = 1.0/z */
                u = __fadd_rn(__fmul_rn(A.fx, __fmul_rn(xc, invz)), A.cx);
                v = __fadd_rn(__fmul_rn(A.fy, __fmul_rn(yc, invz)), A.cy);
                go = u >= kbnd.minX && u < kbnd.maxX && v >= kbnd.minY && v < kbnd.maxY; /* KeyFrame::IsInImage */
            }
            if (go) {
                const float dist3D = vslam_md::norm3(xc, yc, zc); /* cv::norm(p3Dc2) */
                go = !(dist3D < mp.minDistance || dist3D > mp.maxDistance);
                if (go) {
                    level = vslam_md::predict_level(mp.maxDistance, dist3D, A.logScaleFactor, A.nlevels);
                    radius = __fmul_rn(A.th, A.scale[level]);
                }
            }
        } else if (go) { /* wave-uniform */
            const SbpPoint pc = sbp_transform(A.Rcw, A.tcw, mp.pos[0], mp.pos[1], mp.pos[2], A.gemmFloat);
            const float xc = pc.x, yc = pc.y, zc = pc.z;
            go = !(zc < 0.0f);
            if (go) {
                const float invz = __fdiv_rn(1.0f, zc);
                u = __fadd_rn(__fdiv_rn(__fmul_rn(A.fx, xc), zc), A.cx);
                v = __fadd_rn(__fdiv_rn(__fmul_rn(A.fy, yc), zc), A.cy);
                go = u >= kbnd.minX && u < kbnd.maxX && v >= kbnd.minY && v < kbnd.maxY; /* KeyFrame::IsInImage */
                ur = __fsub_rn(u, __fmul_rn(A.bf, invz));
            }
            if (go) {
                const float p0 = __fsub_rn(mp.pos[0], A.Ow[0]), p1 = __fsub_rn(mp.pos[1], A.Ow[1]),
                            p2 = __fsub_rn(mp.pos[2], A.Ow[2]);
                const float dist3D = vslam_md::norm3(p0, p1, p2);
                go = !(dist3D < mp.minDistance || dist3D > mp.maxDistance);
                if (go) go = !(vslam_md::dot3_mat(p0, p1, p2, mp.normal) < __dmul_rn(0.5, (double)dist3D));
                if (go) {
                    level = vslam_md::predict_level(mp.maxDistance, dist3D, A.logScaleFactor, A.nlevels);
                    radius = __fmul_rn(A.th, A.scale[level]);
                }
            }
        }
#define FUSE_NKF A.nKF
#define FUSE_KF_DESC A.kfDesc
#define FUSE_SIM3 A.sim3
#define FUSE_RIG 0
#define FUSE_OFFSET 0
#define FUSE_BEST_IDX A.bestIdx
#define FUSE_BEST_DIST A.bestDist
#include "vslam_fuse_rank_body.inc"
#undef FUSE_NKF
#undef FUSE_KF_DESC
#undef FUSE_SIM3
#undef FUSE_RIG
#undef FUSE_OFFSET
#undef FUSE_BEST_IDX
#undef FUSE_BEST_DIST
    }
}

void vk_fuse_search(hipStream_t st, const FuseArgsDev& A) {
    if (A.nPoints <= 0) return;
    hipLaunchKernelGGL(k_fuse_rank, dim3((A.nPoints + FUSE_QPB - 1) / FUSE_QPB), dim3(256), vk_sbp_rank_lds(A.nKF), st, A);
}

/* ------------------------------------------------------------------------------------------------
 * The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame and both cameras of a two-fisheye rig
 * (fmatcher.cpp:1918-2119 with pKF->NLeft != -1; the Scw overload :2121-2243 as sim3 = 1): k_fuse_rank's sim3 == 0 / 1 gates
 * with KannalaBrandt8::project of the JOB'S camera in place of Pinhole::project, no invz / ur (a rig's mvuRight is -1
 * throughout: the monocular chi2 branch alone), the side's own keypoints as the window's grid, and idxOffset (0 or NLeft,
 * :2079) added to the reported index.  One MapPoint list against up to VSLAM_MAX_FUSE_RIG_JOBS (KeyFrame, camera) jobs: the
 * job is blockIdx.y, read from the by-value argument block with a uniform index.  A workgroup builds its job's candidate
 * table in LDS and serves 16 MapPoints, one wave each; the projection is wave-uniform.  Window, level gate, chi2 gate, Hamming
 * minimum, far rule, reduction and write are k_fuse_rank's own text (vslam_fuse_rank_body.inc).  No workgroup waits for another; every
 * loop is bounded by nKF or by the 16 points of the block.
 * ---------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256)
k_fuse_rank_rig(FuseRigArgs A) {
    extern __shared__ __align__(16) uint8_t sbsm[];
    SbpCand* cand = (SbpCand*)sbsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FuseRigJobDev& J = A.job[blockIdx.y];
    const vslam_kb8_camera& cam = A.cam[J.camera];
    const int nKF = J.nKF;
    const SiBounds bnd = A.bnd;
    const SiBounds kbnd = si_kf_bounds(bnd);
    const SiGridInv inv = si_grid_inv(bnd);
    for (int i = tid; i < nKF; i += 256) cand[i] = sbp_make_cand(J.kps[i], -1.f, bnd, inv);
    __syncthreads();
    int32_t* bestIdx = A.bestIdx + (size_t)blockIdx.y * A.nPoints;
    int32_t* bestDist = A.bestDist + (size_t)blockIdx.y * A.nPoints;
    for (int q = blockIdx.x * FUSE_QPB + wave; q < min(A.nPoints, (int)(blockIdx.x + 1) * FUSE_QPB); q += 4) {
        const FusePoint mp = A.pts[q];
        uint32_t best = 0xFFFFFFFFu;
        uint32_t far = 0xFFFFFFFFu; /* sim3: cell << 12 | index of the first candidate at distance 256 */
        bool go = mp.valid != 0 && (!J.valid || J.valid[q] != 0); /* pMP && !isBad(), !IsInKeyFrame(pKF) */
        float u = 0.f, v = 0.f, radius = 0.f;
        int level = 0;
        if (go) { /* wave-uniform */
            const SbpPoint pc = sbp_transform(J.Rcw, J.tcw, mp.pos[0], mp.pos[1], mp.pos[2], A.gemmFloat);
            go = !(pc.z < 0.0f);
            if (go) {
                const vslam_kb8::Uv uv = vslam_kb8::kb8_project(cam, pc.x, pc.y, pc.z);
                u = uv.u;
                v = uv.v;
                go = u >= kbnd.minX && u < kbnd.maxX && v >= kbnd.minY && v < kbnd.maxY; /* KeyFrame::IsInImage */
            }
            if (go) {
                const float p0 = __fsub_rn(mp.pos[0], J.Ow[0]), p1 = __fsub_rn(mp.pos[1], J.Ow[1]),
                            p2 = __fsub_rn(mp.pos[2], J.Ow[2]);
                const float dist3D = vslam_md::norm3(p0, p1, p2);
                go = !(dist3D < mp.minDistance || dist3D > mp.maxDistance);
                if (go) go = !(vslam_md::dot3_mat(p0, p1, p2, mp.normal) < __dmul_rn(0.5, (double)dist3D));
                if (go) {
                    level = vslam_md::predict_level(mp.maxDistance, dist3D, A.logScaleFactor, A.nlevels);
                    radius = __fmul_rn(A.th, A.scale[level]);
                }
            }
        }
#define FUSE_NKF nKF
#define FUSE_KF_DESC J.desc
#define FUSE_SIM3 J.sim3
#define FUSE_RIG 1
#define FUSE_OFFSET J.idxOffset
#define FUSE_BEST_IDX bestIdx
#define FUSE_BEST_DIST bestDist
#include "vslam_fuse_rank_body.inc"
#undef FUSE_NKF
#undef FUSE_KF_DESC
#undef FUSE_SIM3
#undef FUSE_RIG
#undef FUSE_OFFSET
#undef FUSE_BEST_IDX
#undef FUSE_BEST_DIST
    }
}

void vk_fuse_search_rig(hipStream_t st, const FuseRigArgs& A, int njobs, int maxKF) {
    if (A.nPoints <= 0 || njobs <= 0) return;
    hipLaunchKernelGGL(k_fuse_rank_rig, dim3((A.nPoints + FUSE_QPB - 1) / FUSE_QPB, njobs), dim3(256), vk_sbp_rank_lds(maxKF), st,
                       A);
}

int vk_sbp_set_max_lds(size_t bytes) {
    int rc = (int)hipFuncSetAttribute((const void*)k_sbp_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_fuse_rank_rig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbpm_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbp_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_fuse_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_rig_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbp_rank_rig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbp_rig_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbp_rig_replay, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    rc = (int)hipFuncSetAttribute((const void*)k_sbp_rank_kb8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc) return rc;
    return (int)hipFuncSetAttribute((const void*)k_sbp_replay, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
