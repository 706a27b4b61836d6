/* vslam_two_view.hip -- the scoring half of MotionEstimator::Reconstruct (motion_estimation.cpp:2006-2094) on the device:
 * the pair list (:2017-2029), CheckHomography / CheckFundamental for every hypothesis of FindHomography / FindFundamental
 * (:2096-2195; the loops have no early exit) and their selection, for a batch of frame pairs in one enqueue.  Hypothesis
 * generation (8-point sets, Normalize, ComputeH21 / ComputeF21 through cv::SVDecomp) stays with the caller.
 *
 * k_tv_pairs   one workgroup per job walks vnMatches12 in chunks of 256 with a running base: rank by ballot / popcount and
 *              a four-entry scan of the wave totals, as k_frustum_compact does.  Writes (i, matches12[i]) in list order, gathers
 *              (u1, v1, u2, v2) per pair, counts N.  An entry >= n2 sets the job's error word and is not followed.
 * k_tv_score   one workgroup of eight waves per (job, model, 64 hypotheses), lane = hypothesis in every wave.  The terms are
 *              parallel, the sum is not: per round of 64 pairs each wave computes the terms of eight pairs into LDS, then
 *              wave 0 alone adds the 128 terms of the round to its 64 chains in list order, score = (score + t1) + t2 --
 *              exactly the reference's order, for every input -- while the other waves compute the next round.  Inlier
 *              flags go out as one byte per eight pairs and hypothesis.
 * k_tv_select  one workgroup per (job, model): `if (currentScore > score)` over ascending indices = the lowest index with the
 *              maximal score > 0, NaN never; then the winner's flags, one byte per pair, into the result block.
 *
 * Three launches, plain stores: no workgroup waits for another one and no atomic decides an order.
 */
#include "vslam_ctx.h"
#include "vslam_two_view.h"

static_assert(VSLAM_TV_WAVE_PAIRS == 8, "a wave's flags of a round are one byte");
static_assert(VSLAM_TV_SCORE_LANES == 64, "a wave's lanes are the hypotheses of its workgroup");
#define TV_SCORE_THREADS (VSLAM_TV_SCORE_LANES * VSLAM_TV_SCORE_WAVES)
static_assert(TV_SCORE_THREADS >= VSLAM_TV_STAGE_PAIRS, "one lane per pair fetches the next round");
/* k_tv_score's static LDS: both halves of the terms and of the staged pairs.  More than the 64 KB of earlier CDNA parts: it
 * relies on the 160 KB a gfx950 CU has, and leaves room for two workgroups per CU. */
static_assert(2 * (2 * VSLAM_TV_STAGE_PAIRS * VSLAM_TV_SCORE_LANES * 4 + VSLAM_TV_STAGE_PAIRS * 16) <= 160 * 1024 / 2,
              "two workgroups of k_tv_score per gfx950 CU");

#define TV_PAIRS_THREADS 256
#define TV_SELECT_THREADS 256

__global__ void __launch_bounds__(TV_PAIRS_THREADS)
k_tv_pairs(const TvJobDev* __restrict__ jobs) {
    __shared__ int s_wave[4];
    const TvJobDev J = jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    bool err = false;
    for (int start = 0; start < J.n1; start += TV_PAIRS_THREADS) {
        const int i = start + tid;
        const int m = i < J.n1 ? J.matches[i] : -1;
        const bool bad = m >= J.n2;
        err |= bad;
        const bool keep = m >= 0 && !bad;
        const unsigned long long bk = __ballot(keep);
        const int rank = __popcll(bk & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(bk);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; w++) woff += s_wave[w];
        const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        const int pos = base + woff + rank;
        if (keep && pos < J.cap) {
            J.pairs[2 * pos] = i;
            J.pairs[2 * pos + 1] = m;
            const float* a = J.xy1 + (size_t)i * J.stride1;
            const float* b = J.xy2 + (size_t)m * J.stride2;
            ((float4*)J.pts)[pos] = make_float4(a[0], a[1], b[0], b[1]);
        }
        base += total;
        __syncthreads(); /* s_wave is rewritten by the next chunk */
    }
    const int any_err = __syncthreads_or(err ? 1 : 0);
    if (tid == 0) {
        J.hdr[TV_HDR_N] = base;
        J.hdr[TV_HDR_USED] = (any_err || base > J.cap) ? 0 : base;
        J.hdr[TV_HDR_ERR] = any_err ? 1 : 0;
    }
}

/* 64 hypotheses of one model over the job's pairs.  Every wave owns VSLAM_TV_WAVE_PAIRS pairs of a round and computes, lane
 * = hypothesis, their two terms into LDS (s_t[term][lane]: 64 neighbouring floats, no bank conflict) and their flags (one
 * byte per wave and round).  Behind the round's barrier wave 0 adds the round's terms to its chains IN LIST ORDER while the
 * other waves go on to the next round, whose terms go to the other half of s_t: one barrier per round.  (Wave 0 reaches the
 * barrier of round c + 1 only after the chain of round c, so nobody overwrites terms that are still to be added.)  The next
 * round's pairs are fetched by the first lanes before the terms and stored to LDS behind them. */
template <bool FUND>
__device__ __forceinline__ void tv_score_body(const TvJobDev& J, int N, int hyp, bool live, float4 (*s_p)[VSLAM_TV_STAGE_PAIRS],
                                              float (*s_t)[2 * VSLAM_TV_STAGE_PAIRS * VSLAM_TV_SCORE_LANES]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nhyp = FUND ? J.nF : J.nH;
    const int column = (FUND ? J.nH : 0) + hyp, columns = J.nH + J.nF;
    const int src = min(hyp, nhyp - 1); /* nhyp >= 1: the workgroup exists */
    vslam_tv::Mat3 A, B;
    if (FUND) {
        A = vslam_tv::load_mat3(J.F21 + (size_t)src * 9);
        B = A;
    } else {
        A = vslam_tv::load_mat3(J.H21 + (size_t)src * 9);
        B = vslam_tv::load_mat3(J.H12 + (size_t)src * 9);
    }
    const float inv = J.invSigmaSquare;
    const float4* pts = (const float4*)J.pts;
    const int rounds = (N + VSLAM_TV_STAGE_PAIRS - 1) / VSLAM_TV_STAGE_PAIRS;
    float score = 0.0f;
    if (tid < min(VSLAM_TV_STAGE_PAIRS, N)) s_p[0][tid] = pts[tid];
    __syncthreads();
    for (int c = 0; c < rounds; c++) {
        const int base = c * VSLAM_TV_STAGE_PAIRS, cnt = min(VSLAM_TV_STAGE_PAIRS, N - base), buf = c & 1;
        const int next = base + VSLAM_TV_STAGE_PAIRS + tid;
        const bool fetch = tid < VSLAM_TV_STAGE_PAIRS && next < N;
        float4 ahead = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (fetch) ahead = pts[next];
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < VSLAM_TV_WAVE_PAIRS; q++) {
            const int k = wave * VSLAM_TV_WAVE_PAIRS + q;
            if (k < cnt) { /* the same for the whole wave */
                const float4 p = s_p[buf][k];
                const vslam_tv::Terms t = FUND ? vslam_tv::check_f(A, p.x, p.y, p.z, p.w, inv) : vslam_tv::check_h(A, B, p.x, p.y, p.z, p.w, inv);
                s_t[buf][(2 * k) * VSLAM_TV_SCORE_LANES + lane] = t.t1;
                s_t[buf][(2 * k + 1) * VSLAM_TV_SCORE_LANES + lane] = t.t2;
                bits |= (t.in ? 1u : 0u) << q;
            }
        }
        if (live && wave * VSLAM_TV_WAVE_PAIRS < cnt)
            J.flags[(size_t)(base / VSLAM_TV_WAVE_PAIRS + wave) * columns + column] = (uint8_t)bits;
        if (fetch) s_p[buf ^ 1][tid] = ahead;
        __syncthreads();
        if (wave == 0) {
            const float* t = s_t[buf] + lane;
#pragma unroll 8
            for (int k = 0; k < 2 * cnt; k++) score = vslam_tv::fadd(score, t[k * VSLAM_TV_SCORE_LANES]);
        }
    }
    if (wave == 0 && live) (FUND ? J.scoresF : J.scoresH)[hyp] = vslam_tv::report_score(score);
}

__global__ void __launch_bounds__(TV_SCORE_THREADS)
k_tv_score(const TvJobDev* __restrict__ jobs) {
    __shared__ float4 s_p[2][VSLAM_TV_STAGE_PAIRS];
    __shared__ float s_t[2][2 * VSLAM_TV_STAGE_PAIRS * VSLAM_TV_SCORE_LANES];
    const TvJobDev J = jobs[blockIdx.y];
    const int groupsH = (J.nH + VSLAM_TV_SCORE_LANES - 1) / VSLAM_TV_SCORE_LANES;
    const int groupsF = (J.nF + VSLAM_TV_SCORE_LANES - 1) / VSLAM_TV_SCORE_LANES;
    const int g = blockIdx.x;
    if (g >= groupsH + groupsF) return; /* the grid is sized for the job with the most hypotheses */
    const int N = J.hdr[TV_HDR_USED];
    const int lane = threadIdx.x & 63;
    if (g < groupsH) {
        const int hyp = g * VSLAM_TV_SCORE_LANES + lane;
        tv_score_body<false>(J, N, hyp, hyp < J.nH, s_p, s_t);
    } else {
        const int hyp = (g - groupsH) * VSLAM_TV_SCORE_LANES + lane;
        tv_score_body<true>(J, N, hyp, hyp < J.nF, s_p, s_t);
    }
}

__global__ void __launch_bounds__(TV_SELECT_THREADS)
k_tv_select(const TvJobDev* __restrict__ jobs) {
    __shared__ float s_score[4];
    __shared__ int s_index[4];
    const TvJobDev J = jobs[blockIdx.y];
    const bool fund = blockIdx.x == 1;
    const int nhyp = fund ? J.nF : J.nH;
    const float* scores = fund ? J.scoresF : J.scoresH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = J.hdr[TV_HDR_USED];
    vslam_tv::Best b = vslam_tv::best_none();
    for (int h = tid; h < nhyp; h += TV_SELECT_THREADS) b = vslam_tv::best_take(b, scores[h], h);
    for (int o = 32; o > 0; o >>= 1) {
        vslam_tv::Best c;
        c.score = __shfl_xor(b.score, o, 64);
        c.index = __shfl_xor(b.index, o, 64);
        b = vslam_tv::best_merge(b, c);
    }
    if (lane == 0) {
        s_score[wave] = b.score;
        s_index[wave] = b.index;
    }
    __syncthreads();
    b = vslam_tv::Best{s_score[0], s_index[0]};
    for (int w = 1; w < 4; w++) b = vslam_tv::best_merge(b, vslam_tv::Best{s_score[w], s_index[w]});
    if (tid == 0) {
        J.hdr[TV_HDR_BEST_H + (fund ? 1 : 0)] = b.index;
        ((float*)J.hdr)[TV_HDR_SCORE_H + (fund ? 1 : 0)] = b.index >= 0 ? b.score : 0.0f;
    }
    uint8_t* out = fund ? J.inlF : J.inlH;
    const int column = (fund ? J.nH : 0) + b.index, columns = J.nH + J.nF;
    for (int p = tid; p < N; p += TV_SELECT_THREADS)
        out[p] = b.index >= 0 ? (uint8_t)((J.flags[(size_t)(p >> 3) * columns + column] >> (p & 7)) & 1u) : (uint8_t)0;
}

void vk_two_view(hipStream_t st, const TvJobDev* jobs, int njobs, int max_groups, hipEvent_t* ev) {
    if (ev) (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(k_tv_pairs, dim3(njobs), dim3(TV_PAIRS_THREADS), 0, st, jobs);
    if (ev) (void)hipEventRecord(ev[1], st);
    if (max_groups > 0) hipLaunchKernelGGL(k_tv_score, dim3(max_groups, njobs), dim3(TV_SCORE_THREADS), 0, st, jobs);
    if (ev) (void)hipEventRecord(ev[2], st);
    hipLaunchKernelGGL(k_tv_select, dim3(2, njobs), dim3(TV_SELECT_THREADS), 0, st, jobs);
    if (ev) (void)hipEventRecord(ev[3], st);
}

/* ------------------------------------------------------------------ host side */
static bool tv_job_ok(const vslam_two_view_job& j) {
    if (j.n1 < 0 || j.n1 > 65536 || j.n2 < 0) return false;
    if (j.nH < 0 || j.nH > VSLAM_TWO_VIEW_MAX_HYP || j.nF < 0 || j.nF > VSLAM_TWO_VIEW_MAX_HYP) return false;
    if (j.n1 && (!j.kps1 || !j.matches12)) return false;
    if (j.n1 && j.n2 && !j.kps2) return false;
    if (j.nH && (!j.H21 || !j.H12)) return false;
    if (j.nF && !j.F21) return false;
    if ((j.kps_on_device != 0 && j.kps_on_device != 1) || (j.matches_on_device != 0 && j.matches_on_device != 1)) return false;
    if (j.kps_on_device && ((((uintptr_t)j.kps1) & 3) || (((uintptr_t)j.kps2) & 3))) return false;
    if (j.matches_on_device && (((uintptr_t)j.matches12) & 3)) return false;
    return std::isfinite(j.sigma) && j.sigma != 0.0f;
}

extern "C" int vslam_two_view_score_async(vslam_fe* fe, int njobs, const vslam_two_view_job* jobs) {
    if (!fe || !jobs || njobs < 1 || njobs > VSLAM_TWO_VIEW_MAX_JOBS) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < njobs; j++)
        if (!tv_job_ok(jobs[j])) {
            g_err = "two-view job " + std::to_string(j) +
                    ": n1 <= 65536, nH / nF <= 1024, sigma finite and not zero, placements 0 or 1, device arrays 4-byte aligned";
            return VSLAM_ERR_INVALID;
        }
    if (int rc = fe->tv_op.begin("a two-view scoring is already in flight (vslam_two_view_score_wait)")) return rc;
    HIPCHK(hipSetDevice(fe->p.device));
    /* the staging block: job table | per job: H21 H12 F21, packed host keypoints, host matches  (one range up)
     *                    | per job: header, pairs, scores H / F, masks H / F                    (one range down)
     * the scratch block (HBM only): per job the gathered pairs and the flag bytes */
    size_t sizes[1 + 12 * VSLAM_TWO_VIEW_MAX_JOBS], off[1 + 12 * VSLAM_TWO_VIEW_MAX_JOBS]; /* 6 inputs, 6 results per job */
    size_t ssizes[2 * VSLAM_TWO_VIEW_MAX_JOBS], soff[2 * VSLAM_TWO_VIEW_MAX_JOBS];
    int np = 0;
    sizes[np++] = (size_t)njobs * sizeof(TvJobDev);
    int max_groups = 0;
    for (int j = 0; j < njobs; j++) {
        const vslam_two_view_job& q = jobs[j];
        sizes[np++] = (size_t)q.nH * 36;
        sizes[np++] = (size_t)q.nH * 36;
        sizes[np++] = (size_t)q.nF * 36;
        sizes[np++] = q.kps_on_device ? 0 : (size_t)q.n1 * 8;
        sizes[np++] = q.kps_on_device ? 0 : (size_t)q.n2 * 8;
        sizes[np++] = q.matches_on_device ? 0 : (size_t)q.n1 * 4;
        max_groups = std::max(max_groups, (q.nH + VSLAM_TV_SCORE_LANES - 1) / VSLAM_TV_SCORE_LANES +
                                              (q.nF + VSLAM_TV_SCORE_LANES - 1) / VSLAM_TV_SCORE_LANES);
    }
    const int first_res = np;
    for (int j = 0; j < njobs; j++) {
        const vslam_two_view_job& q = jobs[j];
        const size_t cap = (size_t)std::min(q.n1, VSLAM_TWO_VIEW_MAX_PAIRS);
        sizes[np++] = VSLAM_TV_HDR_WORDS * 4;
        sizes[np++] = cap * 8;
        sizes[np++] = (size_t)q.nH * 4;
        sizes[np++] = (size_t)q.nF * 4;
        sizes[np++] = cap;
        sizes[np++] = cap;
        ssizes[2 * j] = cap * 16;
        ssizes[2 * j + 1] = ((cap + VSLAM_TV_WAVE_PAIRS - 1) / VSLAM_TV_WAVE_PAIRS) * (size_t)(q.nH + q.nF);
    }
    const size_t total = vslam::layout_parts(256, sizes, np, off);
    const size_t stotal = vslam::layout_parts(256, ssizes, 2 * njobs, soff);
    int rc = fe->tv.ensure(total);
    if (rc) return rc;
    if ((rc = fe->d_tv_scratch.ensure(std::max(stotal, (size_t)256)))) return rc;
    /* vslam_fe_set_profiling: the three kernels' own spans (vslam_fe_get_two_view_profile) */
    if ((rc = fe->t_tv.arm(fe->profiling))) return rc;
    uint8_t *h = fe->tv.h, *d = fe->tv.d, *s = fe->d_tv_scratch;
    TvJobDev* table = (TvJobDev*)(h + off[0]);
    for (int j = 0; j < njobs; j++) {
        const vslam_two_view_job& q = jobs[j];
        const size_t* in = off + 1 + 6 * j;
        const size_t* out = off + first_res + 6 * j;
        if (q.nH) {
            memcpy(h + in[0], q.H21, (size_t)q.nH * 36);
            memcpy(h + in[1], q.H12, (size_t)q.nH * 36);
        }
        if (q.nF) memcpy(h + in[2], q.F21, (size_t)q.nF * 36);
        if (!q.kps_on_device) {
            float* a = (float*)(h + in[3]);
            float* b = (float*)(h + in[4]);
            for (int i = 0; i < q.n1; i++) {
                a[2 * i] = q.kps1[i].x;
                a[2 * i + 1] = q.kps1[i].y;
            }
            for (int i = 0; i < q.n2; i++) {
                b[2 * i] = q.kps2[i].x;
                b[2 * i + 1] = q.kps2[i].y;
            }
        }
        if (!q.matches_on_device && q.n1) memcpy(h + in[5], q.matches12, (size_t)q.n1 * 4);
        TvJobDev& J = table[j];
        memset(&J, 0, sizeof(J));
        J.xy1 = q.kps_on_device ? (const float*)q.kps1 : (const float*)(d + in[3]);
        J.xy2 = q.kps_on_device ? (const float*)q.kps2 : (const float*)(d + in[4]);
        J.stride1 = J.stride2 = q.kps_on_device ? (int)(sizeof(vslam_kp) / 4) : 2;
        J.matches = q.matches_on_device ? q.matches12 : (const int32_t*)(d + in[5]);
        J.n1 = q.n1;
        J.n2 = q.n2;
        J.cap = std::min(q.n1, VSLAM_TWO_VIEW_MAX_PAIRS);
        J.nH = q.nH;
        J.nF = q.nF;
        J.invSigmaSquare = vslam_tv::inv_sigma_square(q.sigma);
        J.H21 = (const float*)(d + in[0]);
        J.H12 = (const float*)(d + in[1]);
        J.F21 = (const float*)(d + in[2]);
        J.pts = (float*)(s + soff[2 * j]);
        J.flags = s + soff[2 * j + 1];
        J.hdr = (int32_t*)(d + out[0]);
        J.pairs = (int32_t*)(d + out[1]);
        J.scoresH = (float*)(d + out[2]);
        J.scoresF = (float*)(d + out[3]);
        J.inlH = d + out[4];
        J.inlF = d + out[5];
        vslam_fe::TvJobHost& K = fe->tv_jobs[j];
        K.o_hdr = out[0];
        K.o_pairs = out[1];
        K.o_sh = out[2];
        K.o_sf = out[3];
        K.o_ih = out[4];
        K.o_if = out[5];
        K.cap = J.cap;
        K.nH = q.nH;
        K.nF = q.nF;
    }
    hipStream_t st = fe->stream;
    const size_t o_res = off[first_res];
    fe->tv.up(st, 0, o_res);
    hipEvent_t ev[4] = {fe->t_tv.event(0), fe->t_tv.event(1), fe->t_tv.event(2), fe->t_tv.event(3)};
    vk_two_view(st, (const TvJobDev*)(d + off[0]), njobs, max_groups, fe->t_tv.armed ? ev : nullptr);
    HIPCHK(hipGetLastError());
    fe->tv.down(st, o_res, total - o_res);
    HIPCHK(hipGetLastError());
    fe->tv_op.set(false);
    fe->tv_op.jobs = njobs;
    return VSLAM_OK;
}

extern "C" int vslam_two_view_score_wait(vslam_fe* fe, vslam_two_view_result* results) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->tv_op.ready()) return rc;
    if (!results) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    fe->tv_op.take();
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    int rc = fe->t_tv.collect();
    if (rc) return rc;
    const uint8_t* h = fe->tv.h;
    for (int j = 0; j < fe->tv_op.jobs; j++) {
        const vslam_fe::TvJobHost& K = fe->tv_jobs[j];
        const int32_t* hdr = (const int32_t*)(h + K.o_hdr);
        vslam_two_view_result& R = results[j];
        const int n = hdr[TV_HDR_N], used = hdr[TV_HDR_USED];
        R.n_pairs = n;
        R.best_h = hdr[TV_HDR_BEST_H];
        R.best_f = hdr[TV_HDR_BEST_F];
        memcpy(&R.score_h, hdr + TV_HDR_SCORE_H, 4);
        memcpy(&R.score_f, hdr + TV_HDR_SCORE_F, 4);
        if (R.pairs) memcpy(R.pairs, h + K.o_pairs, (size_t)std::min(n, K.cap) * 8);
        if (R.scores_h) memcpy(R.scores_h, h + K.o_sh, (size_t)K.nH * 4);
        if (R.scores_f) memcpy(R.scores_f, h + K.o_sf, (size_t)K.nF * 4);
        if (R.inliers_h) memcpy(R.inliers_h, h + K.o_ih, (size_t)used);
        if (R.inliers_f) memcpy(R.inliers_f, h + K.o_if, (size_t)used);
        if (hdr[TV_HDR_ERR]) {
            g_err = "two-view job " + std::to_string(j) + ": a matches12 entry is >= n2";
            rc = VSLAM_ERR_INVALID;
        } else if (n > K.cap && rc == VSLAM_OK) {
            g_err = "two-view job " + std::to_string(j) + ": " + std::to_string(n) + " pairs; at most " +
                    std::to_string(VSLAM_TWO_VIEW_MAX_PAIRS) + " are scored on the device";
            rc = VSLAM_ERR_UNSUPPORTED;
        }
    }
    return rc;
}

extern "C" int vslam_two_view_score(vslam_fe* fe, const vslam_two_view_job* job, vslam_two_view_result* result) {
    if (!result) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const int rc = vslam_two_view_score_async(fe, 1, job);
    if (rc) return rc;
    return vslam_two_view_score_wait(fe, result);
}

extern "C" int vslam_fe_get_two_view_profile(vslam_fe* fe, double* pairs_ms, double* score_ms, double* select_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    fe->t_tv.read({pairs_ms, score_ms, select_ms}, passes);
    return VSLAM_OK;
}
