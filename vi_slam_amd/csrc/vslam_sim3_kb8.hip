/* vslam_sim3_kb8.hip -- FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863) for
 * fisheye KeyFrames: ONE MapPoint list against up to 16 (KeyFrame, Scw) jobs in one enqueue, the shape of
 * LoopClosing::FindMatchesByProjection's callers.  The rules are stated in include/vslam_fe.h above vslam_sim3_kb8_job; the
 * kernels are k_s3k_gate / k_s3k_compact / k_sbp_rank_kb8 / k_sbp_resolve / k_sbp_replay / k_s3k_finish
 * (vslam_projection_kernels.hip), the host twin vslamh_search_by_projection_sim3_kb8 (vslam_match_host.cpp).  The staging block
 * fe->s3k is this entry's own: the blocking matchers, which fill fe->proj on the host at once, can run while a search is in
 * flight.  What only the kernels touch (gate records, compacted arrays, the matcher's scratch) lives in fe->d_s3k. */
#include <vector>

#include "vslam_sbp_host.h"

static bool s3k_finite(const float* v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int vslam_search_by_projection_sim3_kb8_async(vslam_fe* fe, const vslam_sim3_kb8_params* p,
                                                         const vslam_sim3_kb8_job* jobs, int n_jobs,
                                                         const vslam_fuse_point* points, const uint8_t* mp_desc, int n_points,
                                                         int points_where) {
    static_assert(sizeof(vslam_fuse_point) == sizeof(FusePoint), "vslam_fuse_point layout");
    static_assert(VSLAM_SIM3_KB8_MAX_JOBS == VSLAM_MAX_SIM3_KB8_JOBS && VSLAM_SIM3_KB8_MAX_JOBS <= VSLAM_MAX_SBP_JOBS,
                  "the argument blocks hold every job");
    static_assert(sizeof(Sim3Kb8Args) <= 4000, "Sim3Kb8Args travels as a kernel argument");
    static_assert(VSLAM_LOCAL_POINTS_MAX <= 256 * 256, "k_s3k_compact: thread t of a chunk holds chunk t's count");
    if (!fe || !p || !jobs || n_jobs < 1 || n_jobs > VSLAM_SIM3_KB8_MAX_JOBS || n_points < 0 ||
        (n_points && (!points || !mp_desc)) || (points_where != VSLAM_IMGS_HOST && points_where != VSLAM_IMGS_DEVICE) ||
        p->img_w < 1 || p->img_h < 1 || p->th < 0 || !(p->ratio_hamming >= 0.0f) || !std::isfinite(p->log_scale_factor)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < n_jobs; j++) {
        const vslam_sim3_kb8_job& s = jobs[j];
        if (s.n_kf < 0 || (s.n_kf && (!s.dev_kps || !s.dev_desc)) || !s3k_finite(s.Rcw, 9) || !s3k_finite(s.tcw, 3) ||
            !s3k_finite(s.Ow, 3)) {
            g_err = "invalid job: device arrays for n_kf keypoints, a finite pose";
            return VSLAM_ERR_INVALID;
        }
        if (s.n_kf && ((((uintptr_t)s.dev_desc) & 15) || (((uintptr_t)s.dev_kps) & 3))) { /* uint4 reads of the rows */
            g_err = "a job's dev_desc must be 16-byte aligned, its dev_kps 4-byte aligned";
            return VSLAM_ERR_INVALID;
        }
    }
    if (points_where == VSLAM_IMGS_DEVICE && n_points && ((((uintptr_t)mp_desc) & 15) || (((uintptr_t)points) & 3))) {
        g_err = "device MapPoint descriptors must be 16-byte aligned, device MapPoints 4-byte aligned";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_required(fe)) return rc;
    if (int rc = fe->s3k_op.begin("a KB8 Sim3 search is already in flight (vslam_search_by_projection_sim3_kb8_wait)")) return rc;
    if (n_points > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "SearchByProjection on the device supports at most VSLAM_LOCAL_POINTS_MAX MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    int max_kf = 0;
    for (int j = 0; j < n_jobs; j++) max_kf = std::max(max_kf, jobs[j].n_kf);
    if (max_kf > 4096) { /* the 12-bit index of the ordering key */
        g_err = "SearchByProjection on the device supports at most 4096 keypoints per KeyFrame";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    const int cap = std::min(n_points, 4096); /* survivors the matcher takes per job */
    if (std::max(vk_sbp_rank_lds(max_kf), vk_sbp_replay_lds(max_kf, cap)) > 150 * 1024) {
        g_err = "SearchByProjection: KeyFrame too large for the LDS-resident matcher";
        return VSLAM_ERR_UNSUPPORTED;
    }
    fe->s3k_op.jobs = n_jobs;
    fe->s3k_op.n = n_points;
    for (int j = 0; j < n_jobs; j++) fe->s3k_nkf[j] = jobs[j].n_kf;
    if (n_points == 0) {
        fe->s3k_op.set(true);
        return VSLAM_OK;
    }
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const size_t np = (size_t)n_points, nj = (size_t)n_jobs;
    /* the block (one upload): points | descriptors (host points only) | per job: validity bytes | per job: vpMatched bytes; then
     * (one copy) per job: match_kf | nmatches, n_gated of every job */
    std::vector<size_t> sizes, off;
    sizes.push_back(from_host ? np * sizeof(FusePoint) : 0);
    sizes.push_back(from_host ? np * 32 : 0);
    for (int j = 0; j < n_jobs; j++) sizes.push_back(jobs[j].valid_host ? np : 0);
    for (int j = 0; j < n_jobs; j++) sizes.push_back(jobs[j].kf_matched_host ? (size_t)jobs[j].n_kf : 0);
    const size_t k_m = sizes.size();
    for (int j = 0; j < n_jobs; j++) sizes.push_back((size_t)jobs[j].n_kf * 4);
    sizes.push_back(nj * 8);
    off.resize(sizes.size());
    const size_t total = vslam::layout_parts(16, sizes.data(), (int)sizes.size(), off.data());
    /* what stays in HBM: gate records | chunk counts | counts | needSeq | per job: proj, topm | descC | flagsC | indexC */
    const size_t nchunks = (np + 255) / 256, capz = (size_t)cap;
    std::vector<size_t> ssz = {nj * np * vk_sbp_proj_bytes(1), nj * nchunks * 4, nj * 16, nj * 4}, soff;
    for (int j = 0; j < n_jobs; j++) {
        ssz.push_back(vk_sbp_scratch_bytes(cap, M));
        ssz.push_back(capz * 32);
        ssz.push_back(capz);
        ssz.push_back(capz * 4);
    }
    soff.resize(ssz.size());
    const size_t stotal = vslam::layout_parts(256, ssz.data(), (int)ssz.size(), soff.data());
    if ((rc = fe->s3k.ensure(total))) return rc;
    if ((rc = fe->d_s3k.ensure(stotal))) return rc;
    if ((rc = fe->t_s3k.arm(fe->profiling))) return rc;
    uint8_t *h = fe->s3k.h, *d = fe->s3k.d, *scr = fe->d_s3k;
    if (from_host) {
        memcpy(h + off[0], points, np * sizeof(FusePoint));
        memcpy(h + off[1], mp_desc, np * 32);
    }
    /* bestDist <= TH_LOW*ratioHamming with an integer bestDist: the float product, floored */
    const float lim = 50 * p->ratio_hamming;
    int thr = lim >= 255.0f ? 255 : (int)floorf(lim);
    if (thr < 0) thr = 0;
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    JS.kf.thHigh = thr + 1;
    JS.kf.logScaleFactor = p->log_scale_factor;
    Sim3Kb8Args A;
    memset(&A, 0, sizeof(A));
    A.cam = fe->kb8;
    for (int l = 0; l < fe->p.nlevels; l++) A.scale[l] = fe->tab.scale[l];
    A.th = (float)p->th;
    A.logScaleFactor = p->log_scale_factor;
    A.bnd = matcher_bounds(fe, p->img_w, p->img_h);
    A.gemmFloat = p->gemm_float != 0;
    A.nlevels = fe->p.nlevels;
    A.nPoints = n_points;
    A.cap = cap;
    A.nchunks = (int)nchunks;
    A.pts = from_host ? (const FusePoint*)(d + off[0]) : (const FusePoint*)points;
    A.mpDesc = from_host ? d + off[1] : mp_desc;
    A.gate = (SbpProj*)(scr + soff[0]);
    A.chunkKeep = (int32_t*)(scr + soff[1]);
    A.counts = (int32_t*)(scr + soff[2]);
    A.result = (int32_t*)(d + off[k_m + nj]);
    int32_t* need_seq = (int32_t*)(scr + soff[3]);
    for (int j = 0; j < n_jobs; j++) {
        const vslam_sim3_kb8_job& s = jobs[j];
        Sim3Kb8JobDev& K = A.job[j];
        memcpy(K.Rcw, s.Rcw, sizeof(K.Rcw));
        memcpy(K.tcw, s.tcw, sizeof(K.tcw));
        memcpy(K.Ow, s.Ow, sizeof(K.Ow));
        K.nKF = s.n_kf;
        if (s.valid_host) {
            memcpy(h + off[2 + j], s.valid_host, np);
            K.valid = d + off[2 + j];
        }
        if (s.kf_matched_host) memcpy(h + off[2 + nj + j], s.kf_matched_host, (size_t)s.n_kf);
        uint8_t* js = scr + soff[4 + 4 * j];
        K.descC = scr + soff[4 + 4 * j + 1];
        K.flagsC = scr + soff[4 + 4 * j + 2];
        K.indexC = (int32_t*)(scr + soff[4 + 4 * j + 3]);
        K.matchKf = (int32_t*)(d + off[k_m + j]);
        SbpJobDev& J = JS.job[j];
        J.mode = 3;
        J.th = A.th;
        J.bnd = A.bnd;
        J.gemmFloat = A.gemmFloat;
        J.nLast = cap;
        J.nLastPtr = A.counts + 4 * j + 1;
        J.nCur = s.n_kf;
        J.flags = K.flagsC;
        J.mpDesc = K.descC;
        J.curKps = s.dev_kps;
        J.curDesc = s.dev_desc;
        J.occupied0 = (s.kf_matched_host && s.n_kf) ? d + off[2 + nj + j] : nullptr;
        sbp_job_outputs(&J, js, cap, K.matchKf, A.result + 2 * j, need_seq + j);
        K.projC = J.proj;
    }
    hipStream_t st = fe->stream;
    if (off[k_m]) fe->s3k.up(st, 0, off[k_m]);
    fe->t_s3k.mark(0, st);
    vk_search_sim3_kb8(st, A, JS, n_jobs, max_kf, fe->d_init_fb, fe->tune.sbp_sequential == 1, fe->t_s3k.event(1),
                       fe->t_s3k.event(2));
    fe->t_s3k.mark(3, st);
    HIPCHK(hipGetLastError());
    fe->s3k.down(st, off[k_m], total - off[k_m]);
    HIPCHK(hipGetLastError());
    fe->s3k_op.set(false);
    for (int j = 0; j < n_jobs; j++) fe->s3k_o_m[j] = off[k_m + j];
    fe->s3k_o_res = off[k_m + nj];
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_sim3_kb8_wait(vslam_fe* fe, int32_t* const* match_kf, int* nmatches, int* n_gated) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->s3k_op.ready()) return rc;
    const int n_jobs = fe->s3k_op.jobs;
    bool ok = match_kf && nmatches && n_gated;
    for (int j = 0; ok && j < n_jobs; j++) ok = !fe->s3k_nkf[j] || match_kf[j];
    if (!ok) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (fe->s3k_op.take()) { /* no MapPoints: nothing was launched */
        for (int j = 0; j < n_jobs; j++) {
            for (int i = 0; i < fe->s3k_nkf[j]; i++) match_kf[j][i] = -1;
            nmatches[j] = 0;
            n_gated[j] = 0;
        }
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    if (int rc = fe->t_s3k.collect()) return rc;
    const int32_t* res = (const int32_t*)(fe->s3k.h + fe->s3k_o_res);
    bool refused = false;
    for (int j = 0; j < n_jobs; j++) {
        if (fe->s3k_nkf[j]) memcpy(match_kf[j], fe->s3k.h + fe->s3k_o_m[j], (size_t)fe->s3k_nkf[j] * 4);
        nmatches[j] = res[2 * j];
        n_gated[j] = res[2 * j + 1];
        refused = refused || res[2 * j] < 0;
    }
    if (refused) {
        g_err = "a job has more than 4096 MapPoints behind its projection gates (nmatches -1): run it on the host";
        return VSLAM_ERR_UNSUPPORTED;
    }
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_sim3_kb8(vslam_fe* fe, const vslam_sim3_kb8_params* p, const vslam_sim3_kb8_job* jobs,
                                                   int n_jobs, const vslam_fuse_point* points, const uint8_t* mp_desc,
                                                   int n_points, int points_where, int32_t* const* match_kf, int* nmatches,
                                                   int* n_gated) {
    if (n_jobs >= 1) { /* what a refusal leaves behind, more than 16 jobs included: the caller sized by n_jobs */
        bool ok = jobs && match_kf && nmatches && n_gated;
        for (int j = 0; ok && j < n_jobs; j++) ok = jobs[j].n_kf <= 0 || match_kf[j];
        if (!ok) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
        for (int j = 0; j < n_jobs; j++) {
            for (int i = 0; i < jobs[j].n_kf; i++) match_kf[j][i] = -1;
            nmatches[j] = -1;
            n_gated[j] = -1;
        }
    }
    int rc = vslam_search_by_projection_sim3_kb8_async(fe, p, jobs, n_jobs, points, mp_desc, n_points, points_where);
    if (rc) return rc;
    return vslam_search_by_projection_sim3_kb8_wait(fe, match_kf, nmatches, n_gated);
}

extern "C" int vslam_fe_get_sim3_kb8_profile(vslam_fe* fe, double* gate_ms, double* rank_ms, double* resolve_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    fe->t_s3k.read({gate_ms, rank_ms, resolve_ms}, passes);
    return VSLAM_OK;
}
