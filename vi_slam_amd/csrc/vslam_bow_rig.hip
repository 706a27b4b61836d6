/* vslam_bow_rig.hip -- FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * (fmatcher.cpp:546-748) for a two-fisheye rig (F.Nleft != -1), one frame against up to 16 keyframes in one pass, and the
 * rig form of the KeyFrame-KeyFrame overload (:1100-1240).
 *
 * The rules, as the reference writes them:
 *   - F has N = Nleft + Nright features; descriptor rows and mFeatVec indices run over [0, N), left first (frame.cpp:1137).  A
 *     rig KeyFrame is indexed the same way, and KeyFrame features of BOTH sides are queries.
 *   - only shared vocabulary nodes are paired (the lower_bound walk).
 *   - for a KeyFrame feature with a good MapPoint, ONE pass over the node's frame features skips occupied slots and keeps
 *     bestDist1 / bestDist2 / bestIdxF over realIdxF < Nleft and bestDist1R / bestIdxFR over the rest; the first candidate in
 *     FeatureVector order wins a tie.
 *   - the left write happens iff bestDist1 <= TH_LOW and bestDist1 < mfNNratio * bestDist2.
 *   - the right branch is NESTED in `if (bestDist1 <= TH_LOW)` (:680 lies within :650): it runs whether or not the left ratio
 *     test passed, and it does not run when the left best is above TH_LOW or when no free left candidate exists (bestDist1
 *     stays 256).  Its ratio test is `.. || true` (:682): bestDist1R <= TH_LOW alone writes bestIdxFR; bestDist2R is dead.
 *   - every write increments nmatches and enters ONE rotation histogram over both sides; the angles are those of keypoints_ /
 *     keypointsRight_ by index on both the KeyFrame and the Frame side.  Only free slots are candidates, so a slot is written
 *     at most once.
 *   - with Nright == 0 this is the pinhole function (vslam_search_by_bow).
 *
 * k_sbow_nodes_rig is k_sbow_nodes (vslam_bow.hip) with a job index in blockIdx.y, the side test on both descriptor reads and a
 * third wave reduction for the right key; k_sbow_finish_rig is k_sbow_finish with one workgroup per job.  A frame feature
 * belongs to one node and a match table to one job, so no workgroup waits for another.
 */
#include "vslam_sbp_host.h" /* vslam_ctx.h; rig_frame_ptrs_ok */
#include "vslam_kernels.h"
#include "vslam_wave.h"
#include "vslam_matchdev.h"

#define SBOWR_TH_LOW 50
#define SBOWR_MAXC 32 /* candidates per lane: 2048 frame features under one node, both sides together */
#define SBOWR_MAX_JOBS 16
#define SBOWR_MAX_SIDE 4096

struct SbowRigJob {
    const uint8_t *kfDescL, *kfDescR, *kfFlags;
    const float* kfAngle;
    const int32_t *kfNodes, *kfOff, *kfFeat;
    int32_t nKFnodes, kfNLeft;
};

struct SbowRigArgs {
    SbowRigJob job[SBOWR_MAX_JOBS];
    const uint8_t *fDescL, *fDescR;
    const vslam_kp *fKpsL, *fKpsR; /* the angles of keypoints_ / keypointsRight_ */
    const int32_t *fNodes, *fOff, *fFeat;
    int32_t nFnodes, nLeft, nF, checkOri;
    float nnratio;
    int32_t* matchF;   /* [job][nF], initialised to -1 by the launch wrapper */
    uint8_t* matchBin; /* [job][nF] */
    int32_t* nmatches; /* [job] */
    int32_t* overflow;
};

__device__ __forceinline__ uint32_t sbowr_hamming(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__global__ void __launch_bounds__(64) k_sbow_nodes_rig(SbowRigArgs A) {
    const int lane = threadIdx.x;
    const int kn = blockIdx.x;
    const int jb = blockIdx.y;
    const SbowRigJob& J = A.job[jb];
    if (kn >= J.nKFnodes) return;
    const int node = J.kfNodes[kn];
    int lo = 0, hi = A.nFnodes; /* lower_bound in F's node list */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.fNodes[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= A.nFnodes || A.fNodes[lo] != node) return;
    const int f0 = A.fOff[lo], cF = A.fOff[lo + 1] - f0;
    if (cF > 64 * SBOWR_MAXC) {
        if (lane == 0) atomicExch(A.overflow, 1);
        return;
    }
    int32_t* matchF = A.matchF + (size_t)jb * A.nF;
    uint8_t* matchBin = A.matchBin + (size_t)jb * A.nF;
    uint32_t occ = 0; /* bit c: my c-th candidate already carries a MapPoint */
    for (int a = J.kfOff[kn]; a < J.kfOff[kn + 1]; a++) {
        const int realIdxKF = J.kfFeat[a];
        if (!J.kfFlags[realIdxKF]) continue; /* !pMP || pMP->isBad() */
        const uint4* dKF = realIdxKF < J.kfNLeft ? (const uint4*)J.kfDescL + (size_t)realIdxKF * 2
                                                 : (const uint4*)J.kfDescR + (size_t)(realIdxKF - J.kfNLeft) * 2;
        const uint4 da = dKF[0], db = dKF[1];
        uint32_t k1 = 0xFFFFFFFFu, d2 = 256u; /* left: my best key, my second-best distance */
        uint32_t kR = 0xFFFFFFFFu;            /* right: my best key */
        for (int c = 0, b = lane; b < cF; c++, b += 64) {
            if (occ & (1u << c)) continue; /* vpMapPointMatches[realIdxF] */
            const int realIdxF = A.fFeat[f0 + b];
            const bool left = realIdxF < A.nLeft;
            const uint4* dF = left ? (const uint4*)A.fDescL + (size_t)realIdxF * 2
                                   : (const uint4*)A.fDescR + (size_t)(realIdxF - A.nLeft) * 2;
            const uint32_t dist = sbowr_hamming(da, db, dF[0], dF[1]);
            const uint32_t key = (dist << 16) | (uint32_t)b;
            if (!left) {
                kR = min(kR, key);
            } else if (key < k1) {
                if (k1 != 0xFFFFFFFFu) d2 = min(d2, k1 >> 16);
                k1 = key;
            } else {
                d2 = min(d2, dist);
            }
        }
        const uint32_t g = wave_min_u32(k1);
        if (g == 0xFFFFFFFFu) continue; /* no free left candidate: bestDist1 stays 256, the right branch is not reached */
        const uint32_t bestDist1 = g >> 16;
        if (bestDist1 > SBOWR_TH_LOW) continue; /* :650, the right branch lies inside */
        const uint32_t contrib = (k1 == g) ? d2 : (k1 == 0xFFFFFFFFu ? 256u : min(k1 >> 16, 256u));
        const uint32_t second = wave_min_u32(contrib);
        const uint32_t gR = wave_min_u32(kR);
        const bool writeL = (float)(int)bestDist1 < __fmul_rn(A.nnratio, (float)(int)second);
        const bool writeR = gR != 0xFFFFFFFFu && (gR >> 16) <= SBOWR_TH_LOW; /* `|| true`, :682 */
        const int bposL = (int)(g & 0xFFFFu), bposR = (int)(gR & 0xFFFFu);
        if (writeL && (bposL & 63) == lane) occ |= 1u << (bposL >> 6);
        if (writeR && (bposR & 63) == lane) occ |= 1u << (bposR >> 6);
        if (lane == 0) {
            const float angKF = A.checkOri ? J.kfAngle[realIdxKF] : 0.0f;
            if (writeL) {
                const int bestIdxF = A.fFeat[f0 + bposL];
                matchF[bestIdxF] = realIdxKF;
                uint8_t bin = 255;
                if (A.checkOri) bin = (uint8_t)vslam_md::rot_bin(angKF, A.fKpsL[bestIdxF].angle, VSLAM_HISTO_LENGTH);
                matchBin[bestIdxF] = bin;
            }
            if (writeR) {
                const int bestIdxFR = A.fFeat[f0 + bposR];
                matchF[bestIdxFR] = realIdxKF;
                uint8_t bin = 255;
                if (A.checkOri) bin = (uint8_t)vslam_md::rot_bin(angKF, A.fKpsR[bestIdxFR - A.nLeft].angle, VSLAM_HISTO_LENGTH);
                matchBin[bestIdxFR] = bin;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_sbow_finish_rig(SbowRigArgs A) {
    __shared__ int s_hist[VSLAM_HISTO_LENGTH];
    __shared__ int s_n, s_removed;
    const int tid = threadIdx.x;
    const int jb = blockIdx.x;
    int32_t* matchF = A.matchF + (size_t)jb * A.nF;
    const uint8_t* matchBin = A.matchBin + (size_t)jb * A.nF;
    if (tid < VSLAM_HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) {
        s_n = 0;
        s_removed = 0;
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < A.nF; i += 256)
        if (matchF[i] >= 0) {
            mine++;
            if (A.checkOri) atomicAdd(&s_hist[matchBin[i]], 1);
        }
    atomicAdd(&s_n, mine);
    __syncthreads();
    if (A.checkOri) {
        const vslam_md::ThreeMaxima mx = vslam_md::three_maxima(s_hist, VSLAM_HISTO_LENGTH);
        int rem = 0;
        for (int i = tid; i < A.nF; i += 256)
            if (matchF[i] >= 0) {
                if (!vslam_md::keeps_bin(mx, matchBin[i])) {
                    matchF[i] = -1;
                    rem++;
                }
            }
        atomicAdd(&s_removed, rem);
    }
    __syncthreads();
    if (tid == 0) A.nmatches[jb] = s_n - s_removed;
}

/* match tables to -1, the counts and the overflow word behind them to 0 */
__global__ void __launch_bounds__(256) k_sbow_rig_clear(int32_t* matchF, int nMatch, int32_t* counts, int nCounts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nMatch) matchF[i] = -1;
    if (i < nCounts) counts[i] = 0;
}

/* a FeatureVector as vslam_bow_assemble makes it: offsets from 0, not decreasing, indices in [0, n) */
static bool sbowr_fv_ok(const int32_t* off, const int32_t* feat, int nnodes, int n) {
    if (nnodes == 0) return true;
    if (off[0] != 0) return false;
    for (int j = 0; j < nnodes; j++) {
        if (off[j + 1] < off[j]) return false;
        for (int a = off[j]; a < off[j + 1]; a++)
            if (feat[a] < 0 || feat[a] >= n) return false;
    }
    return true;
}

extern "C" int vslam_search_by_bow_rig_async(vslam_fe* fe, const vslam_bow_rig_kf* kf_jobs, int n_kf_jobs,
                                             const vslam_rig_frame* frame, const int32_t* f_fv_nodes, const int32_t* f_fv_off,
                                             const int32_t* f_fv_feat, int n_f_nodes, float nnratio, int check_orientation) {
    if (!fe || !kf_jobs || n_kf_jobs < 1 || n_kf_jobs > SBOWR_MAX_JOBS || !rig_frame_ptrs_ok(frame) || n_f_nodes < 0 ||
        (n_f_nodes && (!f_fv_nodes || !f_fv_off || !f_fv_feat))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < n_kf_jobs; j++) {
        const vslam_bow_rig_kf& k = kf_jobs[j];
        const int n = k.n_left + k.n_right;
        if (k.n_left < 0 || k.n_right < 0 || k.n_nodes < 0 || (k.n_left && !k.dev_desc_left) || (k.n_right && !k.dev_desc_right) ||
            (n && (!k.kps_host || !k.flags_host)) || (k.n_nodes && (!k.fv_nodes || !k.fv_off || !k.fv_feat))) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    }
    if (int rc = fe->sbr_op.begin("a rig SearchByBoW is already in flight (vslam_search_by_bow_rig_wait)")) return rc;
    const int N = frame->n_left + frame->n_right;
    bool big = frame->n_left > SBOWR_MAX_SIDE || frame->n_right > SBOWR_MAX_SIDE;
    for (int j = 0; j < n_kf_jobs; j++) big = big || kf_jobs[j].n_left > SBOWR_MAX_SIDE || kf_jobs[j].n_right > SBOWR_MAX_SIDE;
    if (big) {
        g_err = "SearchByBoW of a rig on the device supports at most 4096 features per camera";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!sbowr_fv_ok(f_fv_off, f_fv_feat, n_f_nodes, N)) {
        g_err = "Frame FeatureVector index out of range";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < n_kf_jobs; j++)
        if (!sbowr_fv_ok(kf_jobs[j].fv_off, kf_jobs[j].fv_feat, kf_jobs[j].n_nodes, kf_jobs[j].n_left + kf_jobs[j].n_right)) {
            g_err = "KeyFrame FeatureVector index out of range";
            return VSLAM_ERR_INVALID;
        }
    /* a job takes part when it has features, nodes and something to match against */
    bool live[SBOWR_MAX_JOBS];
    int max_nodes = 0;
    for (int j = 0; j < n_kf_jobs; j++) {
        const vslam_bow_rig_kf& k = kf_jobs[j];
        live[j] = N > 0 && n_f_nodes > 0 && k.n_left + k.n_right > 0 && k.n_nodes > 0;
        if (live[j]) max_nodes = std::max(max_nodes, k.n_nodes);
    }
    /* the 2048 rule, as k_sbow_nodes applies it: a frame node that some keyframe shares holds more than the lanes take */
    for (int f = 0; f < n_f_nodes; f++) {
        if (f_fv_off[f + 1] - f_fv_off[f] <= 64 * SBOWR_MAXC) continue;
        for (int j = 0; j < n_kf_jobs; j++)
            if (live[j] && std::binary_search(kf_jobs[j].fv_nodes, kf_jobs[j].fv_nodes + kf_jobs[j].n_nodes, f_fv_nodes[f])) {
                g_err = "SearchByBoW: more than 2048 frame features under one vocabulary node";
                return VSLAM_ERR_UNSUPPORTED;
            }
    }
    fe->sbr_op.jobs = n_kf_jobs;
    fe->sbr_op.n = N;
    if (max_nodes == 0) {
        fe->sbr_op.set(true);
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    /* inputs (one upload): the frame's FeatureVector once, then per job flags | angles | nodes | offsets | features; behind
     * them the match tables, the counts with the overflow word, the bins */
    const size_t tf = (size_t)f_fv_off[n_f_nodes];
    size_t sizes[3 + 5 * SBOWR_MAX_JOBS + 3], off[3 + 5 * SBOWR_MAX_JOBS + 3];
    int np = 0;
    sizes[np++] = (size_t)n_f_nodes * 4;
    sizes[np++] = (size_t)(n_f_nodes + 1) * 4;
    sizes[np++] = tf * 4;
    for (int j = 0; j < n_kf_jobs; j++) {
        const vslam_bow_rig_kf& k = kf_jobs[j];
        const size_t n = live[j] ? (size_t)(k.n_left + k.n_right) : 0, nn = live[j] ? (size_t)k.n_nodes : 0;
        sizes[np++] = n;
        sizes[np++] = n * 4;
        sizes[np++] = nn * 4;
        sizes[np++] = nn ? (nn + 1) * 4 : 0;
        sizes[np++] = nn ? (size_t)k.fv_off[k.n_nodes] * 4 : 0;
    }
    const int p_m = np;
    sizes[np++] = (size_t)n_kf_jobs * N * 4;
    sizes[np++] = (size_t)(SBOWR_MAX_JOBS + 4) * 4;
    sizes[np++] = (size_t)n_kf_jobs * N;
    const size_t total = vslam::layout_parts(16, sizes, np, off);
    int rc = fe->sbr.ensure(total);
    if (rc) return rc;
    if ((rc = fe->t_sbr.arm(fe->profiling))) return rc;
    uint8_t *h = fe->sbr.h, *d = fe->sbr.d;
    memcpy(h + off[0], f_fv_nodes, sizes[0]);
    memcpy(h + off[1], f_fv_off, sizes[1]);
    memcpy(h + off[2], f_fv_feat, sizes[2]);
    SbowRigArgs A;
    memset(&A, 0, sizeof(A));
    for (int j = 0; j < n_kf_jobs; j++) {
        if (!live[j]) continue; /* nKFnodes = 0: its waves leave at once */
        const vslam_bow_rig_kf& k = kf_jobs[j];
        const int n = k.n_left + k.n_right, q = 3 + 5 * j;
        memcpy(h + off[q], k.flags_host, (size_t)n);
        for (int i = 0; i < n; i++) ((float*)(h + off[q + 1]))[i] = k.kps_host[i].angle;
        memcpy(h + off[q + 2], k.fv_nodes, sizes[q + 2]);
        memcpy(h + off[q + 3], k.fv_off, sizes[q + 3]);
        memcpy(h + off[q + 4], k.fv_feat, sizes[q + 4]);
        SbowRigJob& J = A.job[j];
        J.kfDescL = k.dev_desc_left;
        J.kfDescR = k.dev_desc_right;
        J.kfNLeft = k.n_left;
        J.kfFlags = d + off[q];
        J.kfAngle = (const float*)(d + off[q + 1]);
        J.kfNodes = (const int32_t*)(d + off[q + 2]);
        J.kfOff = (const int32_t*)(d + off[q + 3]);
        J.kfFeat = (const int32_t*)(d + off[q + 4]);
        J.nKFnodes = k.n_nodes;
    }
    A.fDescL = frame->dev_desc_left;
    A.fDescR = frame->dev_desc_right;
    A.fKpsL = frame->dev_kps_left;
    A.fKpsR = frame->dev_kps_right;
    A.fNodes = (const int32_t*)(d + off[0]);
    A.fOff = (const int32_t*)(d + off[1]);
    A.fFeat = (const int32_t*)(d + off[2]);
    A.nFnodes = n_f_nodes;
    A.nLeft = frame->n_left;
    A.nF = N;
    A.checkOri = check_orientation;
    A.nnratio = nnratio;
    A.matchF = (int32_t*)(d + off[p_m]);
    A.nmatches = (int32_t*)(d + off[p_m + 1]);
    A.overflow = A.nmatches + SBOWR_MAX_JOBS;
    A.matchBin = d + off[p_m + 2];
    hipStream_t st = fe->stream;
    fe->sbr.up(st, 0, off[p_m]);
    const int n_match = n_kf_jobs * N;
    hipLaunchKernelGGL(k_sbow_rig_clear, dim3((std::max(n_match, SBOWR_MAX_JOBS + 4) + 255) / 256), dim3(256), 0, st, A.matchF,
                       n_match, A.nmatches, SBOWR_MAX_JOBS + 4);
    fe->t_sbr.mark(0, st);
    hipLaunchKernelGGL(k_sbow_nodes_rig, dim3(max_nodes, n_kf_jobs), dim3(64), 0, st, A);
    fe->t_sbr.mark(1, st);
    hipLaunchKernelGGL(k_sbow_finish_rig, dim3(n_kf_jobs), dim3(256), 0, st, A);
    fe->t_sbr.mark(2, st);
    HIPCHK(hipGetLastError());
    fe->sbr.down(st, off[p_m], off[p_m + 2] - off[p_m]); /* the match tables and the counts; the bins stay */
    HIPCHK(hipGetLastError());
    fe->sbr_op.set(false);
    fe->sbr_o_m = off[p_m];
    fe->sbr_o_n = off[p_m + 1];
    return VSLAM_OK;
}

extern "C" int vslam_search_by_bow_rig_wait(vslam_fe* fe, int32_t* const* match_f, int* nmatches) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->sbr_op.ready()) return rc;
    const int K = fe->sbr_op.jobs, N = fe->sbr_op.n;
    bool ok = nmatches && (N == 0 || match_f);
    for (int j = 0; ok && j < K && N; j++) ok = match_f[j] != nullptr;
    if (!ok) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < K; j++) nmatches[j] = 0;
    if (fe->sbr_op.take()) { /* nothing to match: nothing was launched */
        for (int j = 0; j < K; j++)
            for (int i = 0; i < N; i++) match_f[j][i] = -1;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    if (int rc = fe->t_sbr.collect()) return rc;
    const int32_t* cnt = (const int32_t*)(fe->sbr.h + fe->sbr_o_n);
    if (cnt[SBOWR_MAX_JOBS]) { /* the host test in _async keeps this from happening; the kernel's guard stays the last word */
        for (int j = 0; j < K; j++)
            for (int i = 0; i < N; i++) match_f[j][i] = -1;
        g_err = "SearchByBoW: more than 2048 frame features under one vocabulary node";
        return VSLAM_ERR_UNSUPPORTED;
    }
    for (int j = 0; j < K; j++) {
        memcpy(match_f[j], fe->sbr.h + fe->sbr_o_m + (size_t)j * N * 4, (size_t)N * 4);
        nmatches[j] = cnt[j];
    }
    return VSLAM_OK;
}

extern "C" int vslam_search_by_bow_rig(vslam_fe* fe, const vslam_bow_rig_kf* kf_jobs, int n_kf_jobs, const vslam_rig_frame* frame,
                                       const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat,
                                       int n_f_nodes, float nnratio, int check_orientation, int32_t* const* match_f,
                                       int* nmatches) {
    if (!frame || !nmatches || n_kf_jobs < 1 || n_kf_jobs > SBOWR_MAX_JOBS || frame->n_left < 0 || frame->n_right < 0) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const long long N = (long long)frame->n_left + frame->n_right;
    for (int j = 0; j < n_kf_jobs && N; j++)
        if (!match_f || !match_f[j]) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    for (int j = 0; j < n_kf_jobs; j++) { /* what a refusal leaves behind */
        nmatches[j] = 0;
        for (long long i = 0; i < N; i++) match_f[j][i] = -1;
    }
    int rc = vslam_search_by_bow_rig_async(fe, kf_jobs, n_kf_jobs, frame, f_fv_nodes, f_fv_off, f_fv_feat, n_f_nodes, nnratio,
                                           check_orientation);
    if (rc) return rc;
    return vslam_search_by_bow_rig_wait(fe, match_f, nmatches);
}

extern "C" int vslam_fe_get_bow_rig_profile(vslam_fe* fe, double* nodes_ms, double* finish_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    fe->t_sbr.read({nodes_ms, finish_ms}, passes);
    return VSLAM_OK;
}

/* FMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (fmatcher.cpp:1100-1240) for rig
 * KeyFrames: the reference skips idx >= mvKeysUn.size() on both sides (:1135, :1155), and mvKeysUn of a rig is keypoints_, NLeft
 * entries -- right features are neither queries nor candidates.  The flags go on with the entries >= n_left cleared, the
 * keypoints padded to the flags' length, and the pinhole entry with its kernels does the rest. */
extern "C" int vslam_search_by_bow_keyframes_rig(vslam_fe* fe, const vslam_kp* kps1_host, const uint8_t* dev_desc1,
                                                 const uint8_t* flags1_host, int n1, int n_left1, const int32_t* fv1_nodes,
                                                 const int32_t* fv1_off, const int32_t* fv1_feat, int n1_nodes,
                                                 const vslam_kp* kps2_host, const uint8_t* dev_desc2,
                                                 const uint8_t* flags2_host, int n2, int n_left2, const int32_t* fv2_nodes,
                                                 const int32_t* fv2_off, const int32_t* fv2_feat, int n2_nodes, float nnratio,
                                                 int check_orientation, int32_t* match12, int* nmatches) {
    if (n1 < 0 || n2 < 0 || n_left1 < 0 || n_left1 > n1 || n_left2 < 0 || n_left2 > n2 || (n_left1 && !kps1_host) ||
        (n_left2 && !kps2_host) || (n1 && !flags1_host) || (n2 && !flags2_host)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    vslam_kp zero;
    memset(&zero, 0, sizeof(zero));
    std::vector<vslam_kp> k1((size_t)std::max(n1, 1), zero), k2((size_t)std::max(n2, 1), zero);
    std::vector<uint8_t> f1((size_t)std::max(n1, 1), 0), f2((size_t)std::max(n2, 1), 0);
    for (int i = 0; i < n_left1; i++) k1[i] = kps1_host[i], f1[i] = flags1_host[i];
    for (int i = 0; i < n_left2; i++) k2[i] = kps2_host[i], f2[i] = flags2_host[i];
    return vslam_search_by_bow_keyframes(fe, k1.data(), dev_desc1, f1.data(), n1, fv1_nodes, fv1_off, fv1_feat, n1_nodes, k2.data(),
                                         dev_desc2, f2.data(), n2, fv2_nodes, fv2_off, fv2_feat, n2_nodes, nnratio,
                                         check_orientation, match12, nmatches);
}
