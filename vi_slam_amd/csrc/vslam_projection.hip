/* vslam_projection.hip -- the matchers that project MapPoints into a frame: the SearchByProjection family (frame, KeyFrame,
 * Sim3, map points; host-staged and device-resident), the search half of Fuse, MapPoint::ComputeDistinctiveDescriptors,
 * and Frame::isInFrustum / SearchLocalPoints.  Every entry stages through a vslam_staging block (vslam_staging.h). */
#include "vslam_ctx.h"
#include "vslam_frustum.h"
#include "vslam_kb8.h"

/* ------------------------------------------------------------------ SearchByProjection(CurrentFrame, LastFrame) */
extern "C" int vslam_projection_direction(const float* Tcw, const float* Tlw, float mb, int mono, int gemm_float,
                                          int* forward, int* backward) {
    if (!Tcw || !Tlw || !forward || !backward) return VSLAM_ERR_INVALID;
    /* twc = -Rcw.t()*tcw ; tlc = Rlw*twc + tlw (fmatcher.cpp:2482-2492), each ONE cv::gemm */
    float twc[3], tlc2;
    for (int r = 0; r < 3; r++) {
        if (!gemm_float) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)Tcw[k * 4 + r] * (double)Tcw[k * 4 + 3];
            twc[r] = (float)(s * -1.0);
        } else {
            float s = 0;
            for (int k = 0; k < 3; k++) s += Tcw[k * 4 + r] * Tcw[k * 4 + 3];
            twc[r] = -s;
        }
    }
    if (!gemm_float) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)Tlw[8 + k] * (double)twc[k];
        tlc2 = (float)(s + (double)Tlw[11]);
    } else {
        float s = 0;
        for (int k = 0; k < 3; k++) s += Tlw[8 + k] * twc[k];
        tlc2 = s + Tlw[11];
    }
    *forward = (tlc2 > mb && !mono) ? 1 : 0;
    *backward = (-tlc2 > mb && !mono) ? 1 : 0;
    return VSLAM_OK;
}

/* With a KB8 camera set (vslam_fe_set_kb8_camera) an entry point that projects with Pinhole::project over intrinsics of its own
 * refuses: better than silently projecting a fisheye frame as a pinhole. */
static int kb8_refuse(const vslam_fe* fe) {
    const int rc = vslamh_kb8_projecting_entry(fe->has_kb8);
    if (rc) g_err = "a KB8 camera is set: this entry point projects as a pinhole (vslam_fe_set_kb8_camera)";
    return rc;
}

/* ---- what every entry point of the family does around k_sbp_* (vk_search_by_projection) ---- */
/* once per context: the kernels' LDS limit and the re-scan counters; *M_out = length of the sorted candidate prefix */
static int sbp_prepare(vslam_fe* fe, int* M_out) {
    *M_out = std::min(16, std::max(1, tune_or(fe->tune.sbp_topm, 8)));
    if (!fe->proj_lds_set) {
        if (vk_sbp_set_max_lds(150 * 1024) != 0) {
            g_err = "hipFuncSetAttribute(k_sbp_*) failed";
            return VSLAM_ERR_HIP;
        }
        fe->proj_lds_set = true;
    }
    return vslam_init_fb_ensure(fe);
}

/* the header of a job list: the pyramid's scale factors and M; every job zeroed */
static void sbp_jobs_header(const vslam_fe* fe, int M, SbpJobs* JS) {
    static_assert(sizeof(SbpJobs) <= 4000, "SbpJobs travels as a kernel argument");
    memset(JS, 0, sizeof(*JS));
    for (int l = 0; l < fe->p.nlevels; l++) JS->scale[l] = fe->tab.scale[l];
    JS->nlevels = fe->p.nlevels;
    JS->M = M;
}

/* pose, camera, window and switches of a job that projects with vslam_proj_params (modes 0, 2, 3) */
static void sbp_job_camera(const vslam_fe* fe, const vslam_proj_params& p, SbpJobDev* J) {
    memcpy(J->Tcw, p.Tcw, sizeof(J->Tcw));
    J->fx = p.fx; J->fy = p.fy; J->cx = p.cx; J->cy = p.cy; J->mbf = p.mbf; J->th = p.th;
    J->forward = p.forward != 0; J->backward = p.backward != 0; J->checkOri = p.check_orientation != 0;
    J->bnd = matcher_bounds(fe, p.img_w, p.img_h); J->gemmFloat = p.gemm_float != 0;
}

/* a job's scratch at scr (proj | topm of n_last candidates, vk_sbp_scratch_bytes) and its result words */
static void sbp_job_outputs(SbpJobDev* J, uint8_t* scr, int n_last, int32_t* match_cur, int32_t* nmatches, int32_t* need_seq) {
    J->proj = (SbpProj*)scr;
    J->topm = (uint32_t*)(scr + vk_sbp_proj_bytes(n_last));
    J->matchCur = match_cur;
    J->nmatches = nmatches;
    J->needSeq = need_seq;
}

/* One job in fe->proj to its end: launch, [o_m, end) -- the match table, then at o_n nmatches | needSeq -- to the mirror,
 * wait, hand out. */
static int sbp_run_single(vslam_fe* fe, const SbpJobs& JS, int n_last, int n_cur, size_t o_m, size_t o_n, size_t end,
                          int32_t* match_cur, int* nmatches) {
    hipStream_t st = fe->stream;
    vk_search_by_projection(st, JS, 1, n_last, n_cur, fe->d_init_fb, fe->tune.sbp_sequential == 1 /* cross-check path */);
    HIPCHK(hipGetLastError());
    fe->proj.down(st, o_m, end - o_m);
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(match_cur, fe->proj.h + o_m, (size_t)n_cur * 4);
    *nmatches = *(const int32_t*)(fe->proj.h + o_n);
    return VSLAM_OK;
}

/* extras of the KeyFrame overload (fmatcher.cpp:2689-2811); null for SearchByProjection(CurrentFrame, LastFrame) */
struct SbpKfExtras {
    const float *min_dist, *max_dist;
    float ow[3], log_scale_factor;
    int orb_dist;
    const float* normals = nullptr; /* non-null: the Scw overloads (mode 3) */
    int proj_kind = 0;
};

static int sbp_frame_impl(vslam_fe* fe, const vslam_proj_params* p, const vslam_kp* last_kps_host, int n_last,
                          const uint8_t* last_flags, const float* last_x3dw, const uint8_t* mp_desc_host,
                          const vslam_kp* dev_cur_kps, const uint8_t* dev_cur_desc, int n_cur,
                          const float* cur_u_right_host, const uint8_t* cur_occupied_host, const SbpKfExtras* kf,
                          int32_t* match_cur, int* nmatches) {
    if (!fe || !p || n_last < 0 || n_cur < 0 || !nmatches || (n_cur && (!dev_cur_kps || !dev_cur_desc || !match_cur)) ||
        (n_last && (!last_kps_host || !last_flags || !last_x3dw || !mp_desc_host)) || p->img_w < 1 || p->img_h < 1) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_refuse(fe)) return rc;
    *nmatches = 0;
    if (n_cur == 0 || n_last == 0) {
        for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
        return VSLAM_OK;
    }
    if (n_cur > 4096) { /* i2 is a 12-bit field of the ordering key */
        g_err = "SearchByProjection on the device supports at most 4096 current-frame keypoints";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    if (std::max(vk_sbp_rank_lds(n_cur), vk_sbp_replay_lds(n_cur, n_last)) > 150 * 1024) {
        g_err = "SearchByProjection: frame too large for the LDS-resident matcher";
        return VSLAM_ERR_UNSUPPORTED;
    }
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    /* inputs (one upload): kps | x3Dw | mpDesc | flags | uRight | occupied | the KeyFrame overloads' minDist | maxDist |
     * normals; then scratch | match table | nmatches, needSeq */
    const size_t nl = (size_t)n_last, nc = (size_t)n_cur, kfn = kf ? nl : 0;
    const auto [o_kps, o_x, o_d, o_f, o_u, o_o, o_mn, o_mx, o_nr, o_scr, o_m, o_n, total] = vslam::layout(
        16, {nl * sizeof(vslam_kp), nl * 12, nl * 32, nl, nc * 4, nc, kfn * 4, kfn * 4, (kf && kf->normals) ? nl * 12 : 0,
             vk_sbp_scratch_bytes(n_last, M), nc * 4, 16});
    if ((rc = fe->proj.ensure(total))) return rc;
    uint8_t *h = fe->proj.h, *d = fe->proj.d;
    memcpy(h + o_kps, last_kps_host, nl * sizeof(vslam_kp));
    memcpy(h + o_x, last_x3dw, nl * 12);
    memcpy(h + o_d, mp_desc_host, nl * 32);
    memcpy(h + o_f, last_flags, nl);
    if (cur_u_right_host) memcpy(h + o_u, cur_u_right_host, nc * 4);
    if (cur_occupied_host) memcpy(h + o_o, cur_occupied_host, nc);
    if (kf) {
        for (int i = 0; i < n_last; i++) h[o_f + i] = (last_flags[i] & 1) ? 3 : 0; /* every accepted MapPoint blocks its keypoint */
        memcpy(h + o_mn, kf->min_dist, nl * 4);
        memcpy(h + o_mx, kf->max_dist, nl * 4);
        if (kf->normals) memcpy(h + o_nr, kf->normals, nl * 12);
    }
    /* the runtime's copy, not proj.up as in the other entries: this entry alone at n_last = n_cur = 2000 took 693.2 us per
     * call this way and 696.0 us through the copy kernel, between parent runs of 693.0 and 695.9 us
     * (profiles/matcher_staging_ab.txt); the kernel route was to be taken only if it was not above the slower parent run */
    HIPCHK(hipMemcpyAsync(d, h, o_scr, hipMemcpyHostToDevice, fe->stream));
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    SbpJobDev& J = JS.job[0];
    sbp_job_camera(fe, *p, &J);
    J.nLast = n_last; J.nCur = n_cur;
    J.lastKps = (const vslam_kp*)(d + o_kps);
    J.flags = d + o_f;
    J.x3Dw = (const float*)(d + o_x);
    J.mpDesc = d + o_d;
    J.curKps = dev_cur_kps;
    J.curDesc = dev_cur_desc;
    J.uRight = cur_u_right_host ? (const float*)(d + o_u) : nullptr;
    J.occupied0 = cur_occupied_host ? d + o_o : nullptr;
    sbp_job_outputs(&J, d + o_scr, n_last, (int32_t*)(d + o_m), (int32_t*)(d + o_n), (int32_t*)(d + o_n) + 1);
    if (kf) {
        J.mode = kf->normals ? 3 : 2;
        JS.kf.projKind = kf->proj_kind;
        JS.kf.normals = kf->normals ? (const float*)(d + o_nr) : nullptr;
        JS.kf.thHigh = kf->orb_dist + 1;
        JS.kf.logScaleFactor = kf->log_scale_factor;
        JS.kf.minDist = (const float*)(d + o_mn);
        JS.kf.maxDist = (const float*)(d + o_mx);
        for (int i = 0; i < 3; i++) JS.kf.ow[i] = kf->ow[i];
    }
    return sbp_run_single(fe, JS, n_last, n_cur, o_m, o_n, total, match_cur, nmatches);
}

extern "C" int vslam_search_by_projection_frame(vslam_fe* fe, const vslam_proj_params* p,
                                                const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                                const float* last_x3dw, const uint8_t* mp_desc_host,
                                                const vslam_kp* dev_cur_kps, const uint8_t* dev_cur_desc, int n_cur,
                                                const float* cur_u_right_host, const uint8_t* cur_occupied_host,
                                                int32_t* match_cur, int* nmatches) {
    return sbp_frame_impl(fe, p, last_kps_host, n_last, last_flags, last_x3dw, mp_desc_host, dev_cur_kps, dev_cur_desc, n_cur,
                          cur_u_right_host, cur_occupied_host, nullptr, match_cur, nmatches);
}

/* FMatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched,
 * int th, float ratioHamming) (fmatcher.cpp:750-863) and the overload that also records the KeyFrames
 * (:865-981; its projection is spelled differently, proj_variant 1): mode 3 of the projection kernels */
extern "C" int vslam_search_by_projection_sim3(vslam_fe* fe, const vslam_proj_params* p, const float* Ow,
                                               float log_scale_factor, float ratio_hamming, int proj_variant,
                                               const uint8_t* mp_flags, const float* mp_x3dw, const float* mp_normals,
                                               const float* mp_min_dist, const float* mp_max_dist,
                                               const uint8_t* mp_desc_host, int n_points, const vslam_kp* dev_kf_kps,
                                               const uint8_t* dev_kf_desc, int n_kf, const uint8_t* kf_matched_host,
                                               int32_t* match_kf, int* nmatches) {
    if (!Ow || !p || (n_points > 0 && (!mp_min_dist || !mp_max_dist || !mp_normals)) || proj_variant < 0 || proj_variant > 1 ||
        !(ratio_hamming >= 0.0f)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (n_points > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 candidate MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    /* bestDist <= TH_LOW*ratioHamming with an integer bestDist: the float product, floored */
    const float lim = 50 * ratio_hamming;
    int thr = lim >= 255.0f ? 255 : (int)floorf(lim);
    if (thr < 0) thr = 0;
    SbpKfExtras kf;
    kf.min_dist = mp_min_dist;
    kf.max_dist = mp_max_dist;
    for (int i = 0; i < 3; i++) kf.ow[i] = Ow[i];
    kf.log_scale_factor = log_scale_factor;
    kf.orb_dist = thr;
    kf.normals = mp_normals;
    kf.proj_kind = proj_variant;
    vslam_proj_params q = *p;
    q.check_orientation = 0; /* these overloads have no rotation histogram */
    std::vector<vslam_kp> dummy((size_t)std::max(n_points, 1));
    memset(dummy.data(), 0, dummy.size() * sizeof(vslam_kp));
    return sbp_frame_impl(fe, &q, dummy.data(), n_points, mp_flags, mp_x3dw, mp_desc_host, dev_kf_kps, dev_kf_desc, n_kf, nullptr,
                          kf_matched_host, &kf, match_kf, nmatches);
}

/* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (fmatcher.cpp:2689-2811): same ranking / resolution kernels, mode 2 */
extern "C" int vslam_search_by_projection_keyframe(vslam_fe* fe, const vslam_proj_params* p, const float* Ow,
                                                   float log_scale_factor, int orb_dist, const vslam_kp* kf_kps_host,
                                                   int n_kf, const uint8_t* mp_flags, const float* mp_x3dw,
                                                   const float* mp_min_dist, const float* mp_max_dist,
                                                   const uint8_t* mp_desc_host, const vslam_kp* dev_cur_kps,
                                                   const uint8_t* dev_cur_desc, int n_cur,
                                                   const uint8_t* cur_occupied_host, int32_t* match_cur, int* nmatches) {
    if (!Ow || (n_kf > 0 && (!mp_min_dist || !mp_max_dist)) || orb_dist < 1 || orb_dist > 255) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (n_kf > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 KeyFrame keypoints";
        return VSLAM_ERR_UNSUPPORTED;
    }
    SbpKfExtras kf;
    kf.min_dist = mp_min_dist;
    kf.max_dist = mp_max_dist;
    for (int i = 0; i < 3; i++) kf.ow[i] = Ow[i];
    kf.log_scale_factor = log_scale_factor;
    kf.orb_dist = orb_dist;
    return sbp_frame_impl(fe, p, kf_kps_host, n_kf, mp_flags, mp_x3dw, mp_desc_host, dev_cur_kps, dev_cur_desc, n_cur, nullptr,
                          cur_occupied_host, &kf, match_cur, nmatches);
}

extern "C" int vslam_search_by_projection_dev_async(vslam_fe* fe, int njobs, const vslam_sbp_job* jobs) {
    if (!fe || njobs < 1 || njobs > VSLAM_MAX_SBP_JOBS || !jobs) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_refuse(fe)) return rc; /* modes 0, 2, 3 of the batch form all project with the job's intrinsics */
    const int cap = fe->cap;
    if (cap > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 keypoints per frame";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (std::max(vk_sbp_rank_lds(cap), vk_sbp_replay_lds(cap, cap)) > 150 * 1024) {
        g_err = "SearchByProjection: frame too large for the LDS-resident matcher";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    /* per job: proj | topm ; then all match tables and counts together (one result copy) */
    const size_t per_scr = vslam::layout(256, {vk_sbp_scratch_bytes(cap, M)})[1];
    const auto [o_scr, o_res, total] = vslam::layout(256, {per_scr * njobs, (size_t)njobs * cap * 4 + (size_t)njobs * 8});
    if ((rc = fe->sbp.ensure(total))) return rc;
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    int32_t* d_match = (int32_t*)(fe->sbp.d + o_res);
    int32_t* d_nm = d_match + (size_t)njobs * cap;
    for (int j = 0; j < njobs; j++) {
        const vslam_sbp_job& s = jobs[j];
        if (!s.dev_last_kps || !s.dev_n_last || !s.dev_last_flags || !s.dev_last_x3dw || !s.dev_mp_desc ||
            !s.dev_cur_kps || !s.dev_cur_desc || !s.dev_n_cur || s.p.img_w < 1 || s.p.img_h < 1) {
            g_err = "null device pointer in job";
            return VSLAM_ERR_INVALID;
        }
        SbpJobDev& J = JS.job[j];
        sbp_job_camera(fe, s.p, &J);
        J.nLast = cap; J.nCur = cap;
        J.lastKps = s.dev_last_kps; J.nLastPtr = s.dev_n_last; J.flags = s.dev_last_flags; J.x3Dw = s.dev_last_x3dw;
        J.mpDesc = s.dev_mp_desc; J.curKps = s.dev_cur_kps; J.curDesc = s.dev_cur_desc; J.nCurPtr = s.dev_n_cur;
        J.uRight = s.dev_cur_u_right; J.occupied0 = s.dev_cur_occupied;
        sbp_job_outputs(&J, fe->sbp.d + o_scr + per_scr * j, cap, d_match + (size_t)j * cap, d_nm + j, d_nm + njobs + j);
    }
    vk_search_by_projection(fe->stream, JS, njobs, cap, cap, fe->d_init_fb, fe->tune.sbp_sequential == 1);
    HIPCHK(hipGetLastError());
    fe->sbp.down(fe->stream, o_res, (size_t)njobs * cap * 4 + (size_t)njobs * 4);
    HIPCHK(hipGetLastError());
    fe->sbp_jobs = njobs;
    fe->sbp_o_res = o_res;
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_dev_wait(vslam_fe* fe, const int* n_cur, int32_t* const* match_cur,
                                                   int* nmatches) {
    if (!fe || fe->sbp_jobs < 1) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    const int njobs = fe->sbp_jobs, cap = fe->cap;
    const int32_t* h_m = (const int32_t*)(fe->sbp.h + fe->sbp_o_res);
    const int32_t* h_n = h_m + (size_t)njobs * cap;
    for (int j = 0; j < njobs; j++) {
        if (match_cur && match_cur[j] && n_cur) memcpy(match_cur[j], h_m + (size_t)j * cap, (size_t)std::min(n_cur[j], cap) * 4);
        if (nmatches) nmatches[j] = h_n[j];
    }
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ SearchByProjection(F, vpMapPoints) */
extern "C" int vslam_search_by_projection_mappoints(vslam_fe* fe, const vslam_mp_track* mps_host,
                                                    const uint8_t* mp_desc_host, int n_mp, const vslam_kp* dev_cur_kps,
                                                    const uint8_t* dev_cur_desc, int n_cur,
                                                    const float* cur_u_right_host, const uint8_t* cur_occupied_host,
                                                    int img_w, int img_h, float th, float nnratio, int32_t* match_cur,
                                                    int* nmatches) {
    static_assert(sizeof(vslam_mp_track) == sizeof(MpTrack), "vslam_mp_track layout");
    if (!fe || n_mp < 0 || n_cur < 0 || !nmatches || (n_cur && (!dev_cur_kps || !dev_cur_desc || !match_cur)) ||
        (n_mp && (!mps_host || !mp_desc_host)) || img_w < 1 || img_h < 1) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = 0;
    if (n_cur == 0 || n_mp == 0) {
        for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
        return VSLAM_OK;
    }
    if (n_cur > 4096 || n_mp > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 keypoints / MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!(nnratio >= 0.4f)) { /* keys clamp distances to 255; exact for bestDist <= 100 when 0.4 * 255 > 100 */
        g_err = "SearchByProjection on the device needs nnratio >= 0.4";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const size_t nm = (size_t)n_mp, nc = (size_t)n_cur;
    /* inputs (one upload): records | descriptors | flags | uRight | occupied; then scratch | match table | nmatches, needSeq */
    const auto [o_mp, o_d, o_f, o_u, o_o, o_scr, o_m, o_n, total] =
        vslam::layout(16, {nm * sizeof(MpTrack), nm * 32, nm, nc * 4, nc, vk_sbp_scratch_bytes(n_mp, M), nc * 4, 16});
    if ((rc = fe->proj.ensure(total))) return rc;
    uint8_t *h = fe->proj.h, *d = fe->proj.d;
    memcpy(h + o_mp, mps_host, nm * sizeof(MpTrack));
    memcpy(h + o_d, mp_desc_host, nm * 32);
    for (int i = 0; i < n_mp; i++) h[o_f + i] = (uint8_t)(mps_host[i].flags & 3u);
    if (cur_u_right_host) memcpy(h + o_u, cur_u_right_host, nc * 4);
    if (cur_occupied_host) memcpy(h + o_o, cur_occupied_host, nc);
    fe->proj.up(fe->stream, 0, o_scr); /* pinned -> HBM by a kernel (cheaper to enqueue than hipMemcpyAsync) */
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    SbpJobDev& J = JS.job[0];
    J.mode = 1;
    J.th = th;
    J.nnratio = nnratio;
    J.bnd = matcher_bounds(fe, img_w, img_h);
    J.nLast = n_mp;
    J.nCur = n_cur;
    J.mps = (const MpTrack*)(d + o_mp);
    J.mpDesc = d + o_d;
    J.flags = d + o_f;
    J.curKps = dev_cur_kps;
    J.curDesc = dev_cur_desc;
    J.uRight = cur_u_right_host ? (const float*)(d + o_u) : nullptr;
    J.occupied0 = cur_occupied_host ? d + o_o : nullptr;
    sbp_job_outputs(&J, d + o_scr, n_mp, (int32_t*)(d + o_m), (int32_t*)(d + o_n), (int32_t*)(d + o_n) + 1);
    return sbp_run_single(fe, JS, n_mp, n_cur, o_m, o_n, total, match_cur, nmatches);
}

/* ------------------------------------------------------------------ MapPoint::ComputeDistinctiveDescriptors */
extern "C" int vslam_distinctive_descriptors(vslam_fe* fe, const uint8_t* desc_host, const int32_t* offsets, int nsets,
                                             int32_t* best) {
    if (!fe || nsets < 0 || (nsets && (!offsets || !best))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (nsets == 0) return VSLAM_OK;
    int maxN = 0;
    for (int s = 0; s < nsets; s++) {
        const int n = offsets[s + 1] - offsets[s];
        if (n < 0 || offsets[s] < 0) {
            g_err = "offsets must be non-negative and ascending";
            return VSLAM_ERR_INVALID;
        }
        maxN = std::max(maxN, n);
    }
    if (maxN > 2048) {
        g_err = "ComputeDistinctiveDescriptors on the device supports at most 2048 observations per MapPoint";
        return VSLAM_ERR_UNSUPPORTED;
    }
    const int total = offsets[nsets];
    if (total > 0 && !desc_host) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    const auto [o_d, o_o, o_b, bytes] = vslam::layout(16, {(size_t)total * 32, (size_t)(nsets + 1) * 4, (size_t)nsets * 4});
    int rc = fe->proj.ensure(bytes);
    if (rc) return rc;
    uint8_t *h = fe->proj.h, *d = fe->proj.d;
    if (total) memcpy(h + o_d, desc_host, (size_t)total * 32);
    memcpy(h + o_o, offsets, (size_t)(nsets + 1) * 4);
    if (!fe->dist_lds_set && vk_distinctive_set_max_lds(2048 * 32) != 0) {
        g_err = "hipFuncSetAttribute(k_distinctive) failed";
        return VSLAM_ERR_HIP;
    }
    fe->dist_lds_set = true;
    hipStream_t st = fe->stream;
    fe->proj.up(st, 0, o_b);
    vk_distinctive(st, d + o_d, (const int32_t*)(d + o_o), nsets, maxN, (int32_t*)(d + o_b));
    fe->proj.down(st, o_b, (size_t)nsets * 4);
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(best, h + o_b, (size_t)nsets * 4);
    return VSLAM_OK;
}

/* ---- the search half of FMatcher::Fuse (fmatcher.cpp:1918-2119, :2121-2243): k_fuse_rank ---- */
extern "C" int vslam_fuse_search(vslam_fe* fe, const vslam_fuse_params* p, const vslam_fuse_point* points_host,
                                 const uint8_t* mp_desc_host, int n_points, const vslam_kp* dev_kf_kps,
                                 const uint8_t* dev_kf_desc, int n_kf, const float* kf_u_right_host, int32_t* best_idx,
                                 int32_t* best_dist) {
    static_assert(sizeof(vslam_fuse_point) == sizeof(FusePoint), "vslam_fuse_point layout");
    if (!fe || !p || n_points < 0 || n_kf < 0 || (n_points && (!points_host || !mp_desc_host || !best_idx || !best_dist)) ||
        (n_kf && (!dev_kf_kps || !dev_kf_desc)) || p->img_w < 1 || p->img_h < 1) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_refuse(fe)) return rc;
    for (int i = 0; i < n_points; i++) {
        best_idx[i] = -1;
        best_dist[i] = 256;
    }
    if (n_points == 0 || n_kf == 0) return VSLAM_OK;
    if (n_kf > 4096) {
        g_err = "Fuse on the device supports at most 4096 keypoints per KeyFrame";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const size_t np = (size_t)n_points;
    const auto [o_p, o_d, o_u, o_bi, o_bd, total] = vslam::layout(16, {np * sizeof(FusePoint), np * 32, (size_t)n_kf * 4, np * 4, np * 4});
    if ((rc = fe->proj.ensure(total))) return rc;
    uint8_t *h = fe->proj.h, *d = fe->proj.d;
    memcpy(h + o_p, points_host, np * sizeof(FusePoint));
    memcpy(h + o_d, mp_desc_host, np * 32);
    for (int i = 0; i < n_kf; i++) ((float*)(h + o_u))[i] = kf_u_right_host ? kf_u_right_host[i] : -1.0f;
    hipStream_t st = fe->stream;
    fe->proj.up(st, 0, o_bi);
    FuseArgsDev A;
    memset(&A, 0, sizeof(A));
    for (int i = 0; i < 9; i++) A.Rcw[i] = p->Rcw[i];
    for (int i = 0; i < 3; i++) {
        A.tcw[i] = p->tcw[i];
        A.Ow[i] = p->Ow[i];
    }
    for (int i = 0; i < 9; i++) A.Rb[i] = p->Rb[i];
    for (int i = 0; i < 3; i++) A.tb[i] = p->tb[i];
    A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.bf = p->bf; A.th = p->th;
    A.logScaleFactor = p->log_scale_factor;
    A.bnd = matcher_bounds(fe, p->img_w, p->img_h); A.sim3 = p->sim3; A.gemmFloat = p->gemm_float;
    A.nlevels = fe->p.nlevels; A.nPoints = n_points; A.nKF = n_kf;
    for (int l = 0; l < fe->p.nlevels; l++) {
        A.scale[l] = fe->tab.scale[l];
        A.invSigma2[l] = fe->tab.inv_sigma2[l];
    }
    A.pts = (const FusePoint*)(d + o_p);
    A.mpDesc = d + o_d;
    A.kfKps = dev_kf_kps;
    A.kfDesc = dev_kf_desc;
    A.kfURight = (const float*)(d + o_u);
    A.bestIdx = (int32_t*)(d + o_bi);
    A.bestDist = (int32_t*)(d + o_bd);
    vk_fuse_search(st, A);
    fe->proj.down(st, o_bi, total - o_bi);
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(best_idx, h + o_bi, (size_t)n_points * 4);
    memcpy(best_dist, h + o_bd, (size_t)n_points * 4);
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ Frame::isInFrustum + SearchLocalPoints
 * The frustum stage (vslam_frustum.hip) in front of the matcher of vslam_search_by_projection_mappoints.  k_sbp_rank,
 * k_sbpm_resolve and k_sbpm_replay read their MapPoint count as min(*nLastPtr, nLast) in mode 1 exactly as in mode 0, so the
 * matcher is enqueued behind the compaction with nLast = the capacity and nLastPtr = the clamped count in HBM: no host
 * wait between the stages. */
/* a local-points search, rig or not, holds fe->lp until its _wait */
static bool lp_in_flight(const vslam_fe* fe) { return fe->lp_state == 1 || fe->lp_state == 3; }

static bool frustum_params_ok(const vslam_frustum_params* p) {
    if (!p || p->img_w < 1 || p->img_h < 1) return false;
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(p->Tcw[i])) return false;
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(p->Ow[i])) return false;
    return std::isfinite(p->fx) && std::isfinite(p->fy) && std::isfinite(p->cx) && std::isfinite(p->cy) &&
           std::isfinite(p->mbf) && std::isfinite(p->viewing_cos_limit) && std::isfinite(p->log_scale_factor) &&
           std::isfinite(p->th_far_points);
}

static vslam_fr::Frame frustum_frame(const vslam_fe* fe, const vslam_frustum_params* p) {
    const SiBounds b = matcher_bounds(fe, p->img_w, p->img_h);
    const float bb[4] = {b.minX, b.maxX, b.minY, b.maxY};
    return vslam_fr::make_frame(*p, bb, fe->p.nlevels);
}

/* with a KB8 camera the frustum parameters carry the camera's own fx, fy, cx, cy, bit for bit */
static int frustum_camera_ok(const vslam_fe* fe, const vslam_frustum_params* p) {
    const int rc = vslamh_kb8_frustum_check(p, fe->has_kb8 ? &fe->kb8 : nullptr);
    if (rc) g_err = "fx, fy, cx, cy of the frustum parameters differ from the KB8 camera's (vslam_fe_set_kb8_camera)";
    return rc;
}
/* k_frustum, or its fisheye form while a KB8 camera is set: same arguments, same outputs */
static void frustum_launch(const vslam_fe* fe, hipStream_t st, const FrustumArgsDev& A) {
    if (fe->has_kb8) vk_frustum_kb8(st, A, fe->kb8);
    else vk_frustum(st, A);
}

extern "C" int vslam_frame_in_frustum(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points_host, int n,
                                      vslam_mp_track* track_out, float* depth_out, int* n_in_view) {
    if (!fe || !n_in_view || n < 0 || (n && (!points_host || !track_out)) || !frustum_params_ok(p)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    *n_in_view = 0;
    if (n == 0) return VSLAM_OK;
    if (n > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "Frame::isInFrustum on the device supports at most 65536 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (lp_in_flight(fe)) {
        g_err = "a local-points search is in flight (vslam_search_local_points_wait)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    const int nchunks = (n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    const auto [o_pts, o_track, o_depth, o_cv, o_ck, total] = vslam::layout(
        256, {(size_t)n * sizeof(vslam_map_point), (size_t)n * sizeof(vslam_mp_track), (size_t)n * 4, (size_t)nchunks * 4,
              (size_t)nchunks * 4});
    int rc = fe->lp.ensure(total);
    if (rc) return rc;
    uint8_t *h = fe->lp.h, *d = fe->lp.d;
    memcpy(h + o_pts, points_host, (size_t)n * sizeof(vslam_map_point));
    hipStream_t st = fe->stream;
    fe->lp.up(st, o_pts, o_track);
    FrustumArgsDev A;
    A.F = frustum_frame(fe, p);
    A.n = n;
    A.farPoints = p->far_points != 0;
    A.thFarPoints = p->th_far_points;
    A.pts = (const vslam_map_point*)(d + o_pts);
    A.track = (vslam_mp_track*)(d + o_track);
    A.depth = (float*)(d + o_depth);
    A.chunkInView = (int32_t*)(d + o_cv);
    A.chunkKeep = (int32_t*)(d + o_ck);
    frustum_launch(fe, st, A);
    HIPCHK(hipGetLastError());
    fe->lp.down(st, o_track, o_ck - o_track); /* records | depths | in-view counts */
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(track_out, h + o_track, (size_t)n * sizeof(vslam_mp_track));
    if (depth_out) memcpy(depth_out, h + o_depth, (size_t)n * 4);
    int nv = 0;
    for (int c = 0; c < nchunks; c++) nv += ((const int32_t*)(h + o_cv))[c];
    *n_in_view = nv;
    return VSLAM_OK;
}

/* Frame::isInFrustum of a two-fisheye rig (Nleft != -1): one upload, k_frustum_rig, one copy of both record arrays, both
 * depth arrays and the chunk counts */
extern "C" int vslam_frame_in_frustum_rig(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                          const vslam_map_point* points_host, int n, vslam_mp_track* track_left,
                                          vslam_mp_track* track_right, float* depth_left, float* depth_right, int* n_in_view) {
    if (!fe || !rig || !n_in_view || n < 0 || (n && (!points_host || !track_left || !track_right)) || !frustum_params_ok(p) ||
        !vslam_kb8::camera_ok(&rig->cam2)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(rig->Tlr[i]) || !std::isfinite(rig->Trl[i])) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    if (!fe->has_kb8) {
        g_err = "no KB8 camera set (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    *n_in_view = 0;
    if (n == 0) return VSLAM_OK;
    if (n > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "Frame::isInFrustum on the device supports at most 65536 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (lp_in_flight(fe)) {
        g_err = "a local-points search is in flight (vslam_search_local_points_wait)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    const int nchunks = (n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    const size_t nn = (size_t)n;
    const auto [o_pts, o_tl, o_tr, o_dl, o_dr, o_cv, total] =
        vslam::layout(256, {nn * sizeof(vslam_map_point), nn * sizeof(vslam_mp_track), nn * sizeof(vslam_mp_track), nn * 4,
                            nn * 4, (size_t)nchunks * 4});
    int rc = fe->lp.ensure(total);
    if (rc) return rc;
    uint8_t *h = fe->lp.h, *d = fe->lp.d;
    memcpy(h + o_pts, points_host, nn * sizeof(vslam_map_point));
    hipStream_t st = fe->stream;
    fe->lp.up(st, o_pts, o_tl);
    FrustumRigDev A;
    A.F = frustum_frame(fe, p);
    A.cam1 = fe->kb8;
    A.cam2 = rig->cam2;
    A.right = vslam_kb8::rig_right(A.F, *rig);
    A.n = n;
    A.pts = (const vslam_map_point*)(d + o_pts);
    A.trackL = (vslam_mp_track*)(d + o_tl);
    A.trackR = (vslam_mp_track*)(d + o_tr);
    A.depthL = (float*)(d + o_dl);
    A.depthR = (float*)(d + o_dr);
    A.chunkInView = (int32_t*)(d + o_cv);
    vk_frustum_rig(st, A);
    HIPCHK(hipGetLastError());
    fe->lp.down(st, o_tl, total - o_tl);
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(track_left, h + o_tl, nn * sizeof(vslam_mp_track));
    memcpy(track_right, h + o_tr, nn * sizeof(vslam_mp_track));
    if (depth_left) memcpy(depth_left, h + o_dl, nn * 4);
    if (depth_right) memcpy(depth_right, h + o_dr, nn * 4);
    int nv = 0;
    for (int c = 0; c < nchunks; c++) nv += ((const int32_t*)(h + o_cv))[c];
    *n_in_view = nv;
    return VSLAM_OK;
}

extern "C" int vslam_search_local_points_async(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points,
                                               const uint8_t* mp_desc, int n_mp, int points_where,
                                               const vslam_kp* dev_cur_kps, const uint8_t* dev_cur_desc, int n_cur,
                                               const float* cur_u_right_host, const uint8_t* cur_occupied_host, float th,
                                               float nnratio) {
    if (!fe || n_mp < 0 || n_cur < 0 || (n_cur && (!dev_cur_kps || !dev_cur_desc)) || (n_mp && (!points || !mp_desc)) ||
        (points_where != VSLAM_IMGS_HOST && points_where != VSLAM_IMGS_DEVICE) || !frustum_params_ok(p) ||
        !std::isfinite(th)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (points_where == VSLAM_IMGS_DEVICE && n_mp && ((((uintptr_t)mp_desc) & 15) || (((uintptr_t)points) & 3))) {
        g_err = "device MapPoint descriptors must be 16-byte aligned, device MapPoints 4-byte aligned";
        return VSLAM_ERR_INVALID;
    }
    if (lp_in_flight(fe)) {
        g_err = "a local-points search is already in flight (vslam_search_local_points_wait)";
        return VSLAM_ERR_INVALID;
    }
    if (n_mp > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "SearchLocalPoints on the device supports at most 65536 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (n_cur > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 keypoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!(nnratio >= 0.4f)) { /* see vslam_search_by_projection_mappoints */
        g_err = "SearchByProjection on the device needs nnratio >= 0.4";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    fe->lp_n_mp = n_mp;
    fe->lp_n_cur = n_cur;
    if (n_mp == 0 || n_cur == 0) {
        fe->lp_state = 2;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const int cap = std::min(n_mp, VSLAM_FRUSTUM_MAX_KEPT);
    const int nchunks = (n_mp + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    /* uploaded inputs | records of all points | compacted arrays | matcher scratch | results (one copy) */
    const size_t nm = (size_t)n_mp, nc = (size_t)n_cur, host_mp = from_host ? nm : 0;
    const auto [o_u, o_o, o_pts, o_desc, o_track, o_depth, o_cv, o_ck, o_tc, o_dc, o_fc, o_scr, o_m, o_cnt, o_idx, total] =
        vslam::layout(256, {nc * 4, nc, host_mp * sizeof(vslam_map_point), host_mp * 32, nm * sizeof(vslam_mp_track), nm * 4,
                            (size_t)nchunks * 4, (size_t)nchunks * 4, (size_t)cap * sizeof(vslam_mp_track), (size_t)cap * 32,
                            (size_t)cap, vk_sbp_scratch_bytes(cap, M), nc * 4, 256, (size_t)cap * 4});
    if ((rc = fe->lp.ensure(total))) return rc;
    uint8_t *h = fe->lp.h, *d = fe->lp.d;
    if (cur_u_right_host) memcpy(h + o_u, cur_u_right_host, nc * 4);
    if (cur_occupied_host) memcpy(h + o_o, cur_occupied_host, nc);
    if (from_host) {
        memcpy(h + o_pts, points, nm * sizeof(vslam_map_point));
        memcpy(h + o_desc, mp_desc, nm * 32);
    }
    hipStream_t st = fe->stream;
    /* without right coordinates and occupancy a device-resident map uploads nothing */
    const size_t up0 = cur_u_right_host ? o_u : cur_occupied_host ? o_o : o_pts;
    fe->lp.up(st, up0, o_track - up0);
    const bool prof = fe->profiling; /* vslam_fe_set_profiling: the two kernels' own spans (vslam_fe_get_local_points_profile) */
    for (int i = 0; i < 3 && prof; i++)
        if (int rc = fe->ev_lp[i].ensure()) return rc;
    FrustumArgsDev A;
    A.F = frustum_frame(fe, p);
    A.n = n_mp;
    A.farPoints = p->far_points != 0;
    A.thFarPoints = p->th_far_points;
    A.pts = from_host ? (const vslam_map_point*)(d + o_pts) : points;
    A.track = (vslam_mp_track*)(d + o_track);
    A.depth = (float*)(d + o_depth);
    A.chunkInView = (int32_t*)(d + o_cv);
    A.chunkKeep = (int32_t*)(d + o_ck);
    if (prof) (void)hipEventRecord(fe->ev_lp[0], st);
    frustum_launch(fe, st, A);
    if (prof) (void)hipEventRecord(fe->ev_lp[1], st);
    FrustumCompactDev K;
    K.n = n_mp;
    K.nchunks = nchunks;
    K.farPoints = A.farPoints;
    K.cap = cap;
    K.thFarPoints = A.thFarPoints;
    K.track = A.track;
    K.depth = A.depth;
    K.desc = from_host ? d + o_desc : mp_desc;
    K.chunkKeep = A.chunkKeep;
    K.chunkInView = A.chunkInView;
    K.trackC = (vslam_mp_track*)(d + o_tc);
    K.descC = d + o_dc;
    K.flagsC = d + o_fc;
    K.indexC = (int32_t*)(d + o_idx);
    int32_t* cnt = (int32_t*)(d + o_cnt); /* nmatches, needSeq | kept, min(kept, cap), nToMatch */
    K.counts = cnt + 2;
    vk_frustum_compact(st, K);
    if (prof) (void)hipEventRecord(fe->ev_lp[2], st);
    fe->lp_timed = prof;
    HIPCHK(hipGetLastError());
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    SbpJobDev& J = JS.job[0];
    J.mode = 1;
    J.th = th;
    J.nnratio = nnratio;
    J.bnd = matcher_bounds(fe, p->img_w, p->img_h);
    J.nLast = cap;
    J.nLastPtr = cnt + 3;
    J.nCur = n_cur;
    J.mps = (const MpTrack*)(d + o_tc);
    J.mpDesc = d + o_dc;
    J.flags = d + o_fc;
    J.curKps = dev_cur_kps;
    J.curDesc = dev_cur_desc;
    J.uRight = cur_u_right_host ? (const float*)(d + o_u) : nullptr;
    J.occupied0 = cur_occupied_host ? d + o_o : nullptr;
    sbp_job_outputs(&J, d + o_scr, cap, (int32_t*)(d + o_m), cnt, cnt + 1);
    vk_search_by_projection(st, JS, 1, cap, n_cur, fe->d_init_fb, fe->tune.sbp_sequential == 1);
    HIPCHK(hipGetLastError());
    fe->lp.down(st, o_m, total - o_m); /* match table | counts | original indices */
    HIPCHK(hipGetLastError());
    fe->lp_state = 1;
    fe->lp_cap = cap;
    fe->lp_o_track = o_track;
    fe->lp_o_res = o_m;
    fe->lp_o_cnt = o_cnt;
    fe->lp_o_idx = o_idx;
    return VSLAM_OK;
}

extern "C" int vslam_search_local_points_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match,
                                              int* n_matched_against, vslam_mp_track* track_out) {
    if (!fe || fe->lp_state == 0) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (fe->lp_state >= 3) {
        g_err = "the search enqueued is a rig search (vslam_search_local_points_rig_wait)";
        return VSLAM_ERR_INVALID;
    }
    const int n_mp = fe->lp_n_mp, n_cur = fe->lp_n_cur;
    if (!nmatches || !n_to_match || !n_matched_against || (n_cur && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = *n_to_match = *n_matched_against = 0;
    if (fe->lp_state == 2) { /* n_mp == 0 or n_cur == 0: nothing was launched */
        fe->lp_state = 0;
        for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
        if (track_out && n_mp) { /* async launched nothing and kept no inputs: there are no records to hand out */
            g_err = "no records: a search without keypoints launches nothing; call vslam_frame_in_frustum for the records";
            return VSLAM_ERR_INVALID;
        }
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    fe->lp_state = 0;
    HIPCHK(vslam_stream_wait(fe->stream));
    if (fe->lp_timed) {
        float a = 0.0f, b = 0.0f;
        fe->lp_timed = false;
        HIPCHK(hipEventElapsedTime(&a, fe->ev_lp[0], fe->ev_lp[1]));
        HIPCHK(hipEventElapsedTime(&b, fe->ev_lp[1], fe->ev_lp[2]));
        fe->lp_ms[0] += a;
        fe->lp_ms[1] += b;
        fe->lp_passes++;
    }
    const uint8_t* h = fe->lp.h;
    const int32_t* cnt = (const int32_t*)(h + fe->lp_o_cnt);
    const int32_t* idx = (const int32_t*)(h + fe->lp_o_idx);
    *n_matched_against = cnt[2];
    *n_to_match = cnt[4];
    if (track_out)
        HIPCHK(hipMemcpy(track_out, fe->lp.d + fe->lp_o_track, (size_t)n_mp * sizeof(vslam_mp_track), hipMemcpyDeviceToHost));
    const int rc = vslamh_local_points_finish((const int32_t*)(h + fe->lp_o_res), n_cur, idx, cnt[2], fe->lp_cap, match_cur);
    if (rc == VSLAM_ERR_UNSUPPORTED)
        g_err = "SearchLocalPoints: more than 4096 MapPoints in view; SearchByProjection on the device takes at most 4096";
    else if (rc)
        g_err = "invalid arguments";
    else
        *nmatches = cnt[0];
    return rc;
}

extern "C" int vslam_search_local_points(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points,
                                         const uint8_t* mp_desc, int n_mp, int points_where, const vslam_kp* dev_cur_kps,
                                         const uint8_t* dev_cur_desc, int n_cur, const float* cur_u_right_host,
                                         const uint8_t* cur_occupied_host, float th, float nnratio, int32_t* match_cur,
                                         int* nmatches, int* n_to_match, int* n_matched_against, vslam_mp_track* track_out) {
    if (!nmatches || !n_to_match || !n_matched_against || (n_cur > 0 && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_search_local_points_async(fe, p, points, mp_desc, n_mp, points_where, dev_cur_kps, dev_cur_desc, n_cur,
                                             cur_u_right_host, cur_occupied_host, th, nnratio);
    if (rc) return rc;
    return vslam_search_local_points_wait(fe, match_cur, nmatches, n_to_match, n_matched_against, track_out);
}

/* with vslam_fe_set_profiling on: HIP-event time of k_frustum and of k_frustum_compact alone, summed over the searches
 * waited for since */
extern "C" int vslam_fe_get_local_points_profile(vslam_fe* fe, double* frustum_ms, double* compact_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (frustum_ms) *frustum_ms = fe->lp_ms[0];
    if (compact_ms) *compact_ms = fe->lp_ms[1];
    if (passes) *passes = fe->lp_passes;
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ SearchByProjection(F, vpMapPoints), SearchLocalPoints: rig
 * fmatcher.cpp:321-491 with Nleft != -1.  Ranking is k_sbp_rank mode 1 as two jobs of one launch (left keypoints with the
 * caller's th, right keypoints with th = 1); the coupled resolution is k_rig_resolve (vslam_projection_kernels.hip). */
static int rig_frame_check(const vslam_rig_frame* f) {
    if (!f || f->n_left < 0 || f->n_right < 0 || (f->n_left && (!f->dev_kps_left || !f->dev_desc_left)) ||
        (f->n_right && (!f->dev_kps_right || !f->dev_desc_right))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (f->n_left > 4096 || f->n_right > 4096) { /* the 12-bit index of the ordering key */
        g_err = "SearchByProjection on the device supports at most 4096 keypoints per camera";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (vslamh_rig_maps_check(f->left_to_right_host, f->n_left, f->right_to_left_host, f->n_right)) {
        g_err = "mvLeftToRightMatch / mvRightToLeftMatch: every entry is -1 or an index of the other camera's keypoints";
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

/* maps and occupancy of a rig frame into the mirror at o_l | o_r | o_o */
static void rig_frame_stage(const vslam_rig_frame& f, uint8_t* h, size_t o_l, size_t o_r, size_t o_o) {
    if (f.n_left) memcpy(h + o_l, f.left_to_right_host, (size_t)f.n_left * 4);
    if (f.n_right) memcpy(h + o_r, f.right_to_left_host, (size_t)f.n_right * 4);
    if (f.occupied_host) memcpy(h + o_o, f.occupied_host, (size_t)f.n_left + (size_t)f.n_right);
}

/* the two ranking jobs and the resolver's arguments over device arrays: records, descriptors and flags of n_mp MapPoints
 * (n_mp_ptr: their count in HBM, or null), scratch of vk_sbp_scratch_bytes(n_mp, M) per side */
static void rig_jobs(const vslam_fe* fe, int M, const vslam_rig_frame& f, int img_w, int img_h, float th, float nnratio,
                     const MpTrack* recL, const MpTrack* recR, const uint8_t* desc, const uint8_t* flags, int n_mp,
                     const int32_t* n_mp_ptr, uint8_t* scrL, uint8_t* scrR, const int32_t* d_l2r, const int32_t* d_r2l,
                     const uint8_t* d_occ, int32_t* d_match, int32_t* d_nm, SbpJobs* JS, RigResolveDev* A) {
    sbp_jobs_header(fe, M, JS);
    for (int side = 0; side < 2; side++) {
        SbpJobDev& J = JS->job[side];
        J.mode = 1;
        J.th = side == 0 ? th : 1.0f; /* fmatcher.cpp:425: the right radius is not multiplied by th */
        J.nnratio = nnratio;
        J.bnd = matcher_bounds(fe, img_w, img_h);
        J.nLast = n_mp;
        J.nLastPtr = n_mp_ptr;
        J.nCur = side == 0 ? f.n_left : f.n_right;
        J.mps = side == 0 ? recL : recR;
        J.mpDesc = desc;
        J.flags = flags;
        J.curKps = side == 0 ? f.dev_kps_left : f.dev_kps_right;
        J.curDesc = side == 0 ? f.dev_desc_left : f.dev_desc_right;
        sbp_job_outputs(&J, side == 0 ? scrL : scrR, n_mp, nullptr, nullptr, nullptr);
    }
    A->nLeft = f.n_left;
    A->nRight = f.n_right;
    A->forceSeq = fe->tune.sbp_sequential == 1;
    A->leftToRight = d_l2r;
    A->rightToLeft = d_r2l;
    A->occupied0 = d_occ;
    A->matchCur = d_match;
    A->nmatches = d_nm;
    A->fallbacks = fe->d_init_fb;
}

extern "C" int vslam_search_by_projection_mappoints_rig(vslam_fe* fe, const vslam_mp_track* track_left_host,
                                                        const vslam_mp_track* track_right_host, const uint8_t* mp_desc_host,
                                                        int n_mp, const vslam_rig_frame* frame, int img_w, int img_h, float th,
                                                        float nnratio, int32_t* match_cur, int* nmatches) {
    if (!fe || n_mp < 0 || !nmatches || (n_mp && (!track_left_host || !track_right_host || !mp_desc_host)) || img_w < 1 ||
        img_h < 1 || !std::isfinite(th)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = rig_frame_check(frame)) return rc;
    const vslam_rig_frame& f = *frame;
    const int N = f.n_left + f.n_right;
    if (N && !match_cur) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = 0;
    for (int i = 0; i < N; i++) match_cur[i] = -1;
    if (N == 0 || n_mp == 0) return VSLAM_OK;
    if (n_mp > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!(nnratio >= 0.4f)) { /* see vslam_search_by_projection_mappoints */
        g_err = "SearchByProjection on the device needs nnratio >= 0.4";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const size_t nm = (size_t)n_mp, nl = (size_t)f.n_left, nr = (size_t)f.n_right;
    /* inputs (one upload): left records | right records | descriptors | flags | L2R | R2L | occupied; then the scratch of both
     * sides | match table | nmatches */
    const auto [o_tl, o_tr, o_d, o_f, o_l, o_r, o_o, o_sl, o_sr, o_m, o_n, total] =
        vslam::layout(16, {nm * sizeof(MpTrack), nm * sizeof(MpTrack), nm * 32, nm, nl * 4, nr * 4, nl + nr,
                           vk_sbp_scratch_bytes(n_mp, M), vk_sbp_scratch_bytes(n_mp, M), (nl + nr) * 4, 16});
    if ((rc = fe->proj.ensure(total))) return rc;
    uint8_t *h = fe->proj.h, *d = fe->proj.d;
    memcpy(h + o_tl, track_left_host, nm * sizeof(MpTrack));
    memcpy(h + o_tr, track_right_host, nm * sizeof(MpTrack));
    memcpy(h + o_d, mp_desc_host, nm * 32);
    MpTrack* hr = (MpTrack*)(h + o_tr);
    for (int i = 0; i < n_mp; i++) {
        /* one MapPoint: Observations() > 0 of either record; a right record with level -1 takes no right branch (:424) */
        h[o_f + i] = (uint8_t)((track_left_host[i].flags | track_right_host[i].flags) & 2u);
        if (hr[i].level == -1) hr[i].flags &= ~1u;
    }
    rig_frame_stage(f, h, o_l, o_r, o_o);
    hipStream_t st = fe->stream;
    fe->proj.up(st, 0, o_sl);
    SbpJobs JS;
    RigResolveDev A;
    rig_jobs(fe, M, f, img_w, img_h, th, nnratio, (const MpTrack*)(d + o_tl), (const MpTrack*)(d + o_tr), d + o_d, d + o_f, n_mp,
             nullptr, d + o_sl, d + o_sr, (const int32_t*)(d + o_l), (const int32_t*)(d + o_r),
             f.occupied_host ? d + o_o : nullptr, (int32_t*)(d + o_m), (int32_t*)(d + o_n), &JS, &A);
    vk_search_rig(st, JS, A, n_mp);
    HIPCHK(hipGetLastError());
    fe->proj.down(st, o_m, total - o_m);
    HIPCHK(hipGetLastError());
    HIPCHK(vslam_stream_wait(st));
    memcpy(match_cur, h + o_m, (size_t)N * 4);
    *nmatches = *(const int32_t*)(h + o_n);
    return VSLAM_OK;
}

extern "C" int vslam_search_local_points_rig_async(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                                   const vslam_map_point* points, const uint8_t* mp_desc, int n_mp,
                                                   int points_where, const vslam_rig_frame* frame, float th, float nnratio) {
    if (!fe || !rig || n_mp < 0 || (n_mp && (!points || !mp_desc)) ||
        (points_where != VSLAM_IMGS_HOST && points_where != VSLAM_IMGS_DEVICE) || !frustum_params_ok(p) || !std::isfinite(th) ||
        !vslam_kb8::camera_ok(&rig->cam2)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(rig->Tlr[i]) || !std::isfinite(rig->Trl[i])) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    if (int rc = rig_frame_check(frame)) return rc;
    if (points_where == VSLAM_IMGS_DEVICE && n_mp && ((((uintptr_t)mp_desc) & 15) || (((uintptr_t)points) & 3))) {
        g_err = "device MapPoint descriptors must be 16-byte aligned, device MapPoints 4-byte aligned";
        return VSLAM_ERR_INVALID;
    }
    if (!fe->has_kb8) {
        g_err = "no KB8 camera set (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    if (lp_in_flight(fe)) {
        g_err = "a local-points search is already in flight (vslam_search_local_points_wait / _rig_wait)";
        return VSLAM_ERR_INVALID;
    }
    if (n_mp > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "SearchLocalPoints on the device supports at most 65536 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!(nnratio >= 0.4f)) {
        g_err = "SearchByProjection on the device needs nnratio >= 0.4";
        return VSLAM_ERR_UNSUPPORTED;
    }
    const vslam_rig_frame& f = *frame;
    const int N = f.n_left + f.n_right;
    fe->lp_n_mp = n_mp;
    fe->lp_n_cur = N;
    if (n_mp == 0 || N == 0) {
        fe->lp_state = 4;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const int cap = std::min(n_mp, VSLAM_FRUSTUM_MAX_KEPT);
    const int nchunks = (n_mp + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    /* uploaded inputs | records and depths of all points | chunk counts | compacted arrays | matcher scratch | results (one copy) */
    const size_t nm = (size_t)n_mp, nl = (size_t)f.n_left, nr = (size_t)f.n_right, host_mp = from_host ? nm : 0;
    const size_t rec = sizeof(vslam_mp_track);
    const auto [o_l, o_r, o_o, o_pts, o_desc, o_tl, o_tr, o_dl, o_dr, o_cv, o_ck, o_tlc, o_trc, o_dc, o_fc, o_sl, o_sr, o_m, o_cnt,
                o_idx, total] =
        vslam::layout(256, {nl * 4, nr * 4, nl + nr, host_mp * sizeof(vslam_map_point), host_mp * 32, nm * rec, nm * rec, nm * 4,
                            nm * 4, (size_t)nchunks * 4, (size_t)nchunks * 4, (size_t)cap * rec, (size_t)cap * rec,
                            (size_t)cap * 32, (size_t)cap, vk_sbp_scratch_bytes(cap, M), vk_sbp_scratch_bytes(cap, M),
                            (nl + nr) * 4, 256, (size_t)cap * 4});
    if ((rc = fe->lp.ensure(total))) return rc;
    uint8_t *h = fe->lp.h, *d = fe->lp.d;
    rig_frame_stage(f, h, o_l, o_r, o_o);
    if (from_host) {
        memcpy(h + o_pts, points, nm * sizeof(vslam_map_point));
        memcpy(h + o_desc, mp_desc, nm * 32);
    }
    hipStream_t st = fe->stream;
    fe->lp.up(st, 0, o_tl);
    const bool prof = fe->profiling;
    for (int i = 0; i < 3 && prof; i++)
        if (int rc = fe->ev_rig[i].ensure()) return rc;
    FrustumRigDev R;
    R.F = frustum_frame(fe, p);
    R.cam1 = fe->kb8;
    R.cam2 = rig->cam2;
    R.right = vslam_kb8::rig_right(R.F, *rig);
    R.n = n_mp;
    R.pts = from_host ? (const vslam_map_point*)(d + o_pts) : points;
    R.trackL = (vslam_mp_track*)(d + o_tl);
    R.trackR = (vslam_mp_track*)(d + o_tr);
    R.depthL = (float*)(d + o_dl);
    R.depthR = (float*)(d + o_dr);
    R.chunkInView = (int32_t*)(d + o_cv);
    vk_frustum_rig(st, R);
    int32_t* cnt = (int32_t*)(d + o_cnt); /* nmatches, - | kept, min(kept, cap), nToMatch */
    FrustumRigCompactDev K;
    K.n = n_mp;
    K.nchunks = nchunks;
    K.farPoints = p->far_points != 0;
    K.cap = cap;
    K.thFarPoints = p->th_far_points;
    K.trackL = R.trackL;
    K.trackR = R.trackR;
    K.depthL = R.depthL;
    K.desc = from_host ? d + o_desc : mp_desc;
    K.chunkKeep = (int32_t*)(d + o_ck);
    K.chunkInView = R.chunkInView;
    K.trackLC = (vslam_mp_track*)(d + o_tlc);
    K.trackRC = (vslam_mp_track*)(d + o_trc);
    K.descC = d + o_dc;
    K.flagsC = d + o_fc;
    K.indexC = (int32_t*)(d + o_idx);
    K.counts = cnt + 2;
    vk_rig_compact(st, K);
    HIPCHK(hipGetLastError());
    SbpJobs JS;
    RigResolveDev A;
    rig_jobs(fe, M, f, p->img_w, p->img_h, th, nnratio, (const MpTrack*)(d + o_tlc), (const MpTrack*)(d + o_trc), d + o_dc,
             d + o_fc, cap, cnt + 3, d + o_sl, d + o_sr, (const int32_t*)(d + o_l), (const int32_t*)(d + o_r),
             f.occupied_host ? d + o_o : nullptr, (int32_t*)(d + o_m), cnt, &JS, &A);
    if (prof) (void)hipEventRecord(fe->ev_rig[0], st);
    vk_search_rig(st, JS, A, cap, prof ? (hipEvent_t)fe->ev_rig[1] : nullptr);
    if (prof) (void)hipEventRecord(fe->ev_rig[2], st);
    fe->rig_timed = prof;
    HIPCHK(hipGetLastError());
    fe->lp.down(st, o_m, total - o_m); /* match table | counts | original indices */
    HIPCHK(hipGetLastError());
    fe->lp_state = 3;
    fe->lp_cap = cap;
    fe->lp_o_track = o_tl;
    fe->lp_o_track_r = o_tr;
    fe->lp_o_res = o_m;
    fe->lp_o_cnt = o_cnt;
    fe->lp_o_idx = o_idx;
    return VSLAM_OK;
}

extern "C" int vslam_search_local_points_rig_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match,
                                                  int* n_matched_against, vslam_mp_track* track_left,
                                                  vslam_mp_track* track_right) {
    if (!fe || fe->lp_state == 0) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (fe->lp_state < 3) {
        g_err = "the search enqueued is not a rig search (vslam_search_local_points_wait)";
        return VSLAM_ERR_INVALID;
    }
    const int n_mp = fe->lp_n_mp, N = fe->lp_n_cur;
    if (!nmatches || !n_to_match || !n_matched_against || (N && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = *n_to_match = *n_matched_against = 0;
    if (fe->lp_state == 4) { /* no MapPoints or no keypoints: nothing was launched */
        fe->lp_state = 0;
        for (int i = 0; i < N; i++) match_cur[i] = -1;
        if ((track_left || track_right) && n_mp) {
            g_err = "no records: a search without keypoints launches nothing; call vslam_frame_in_frustum_rig for the records";
            return VSLAM_ERR_INVALID;
        }
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    fe->lp_state = 0;
    HIPCHK(vslam_stream_wait(fe->stream));
    if (fe->rig_timed) {
        float a = 0.0f, b = 0.0f;
        fe->rig_timed = false;
        HIPCHK(hipEventElapsedTime(&a, fe->ev_rig[0], fe->ev_rig[1]));
        HIPCHK(hipEventElapsedTime(&b, fe->ev_rig[1], fe->ev_rig[2]));
        fe->rig_ms[0] += a;
        fe->rig_ms[1] += b;
        fe->rig_passes++;
    }
    const uint8_t* h = fe->lp.h;
    const int32_t* cnt = (const int32_t*)(h + fe->lp_o_cnt);
    const int32_t* idx = (const int32_t*)(h + fe->lp_o_idx);
    *n_matched_against = cnt[2];
    *n_to_match = cnt[4];
    const size_t bytes = (size_t)n_mp * sizeof(vslam_mp_track);
    if (track_left) HIPCHK(hipMemcpy(track_left, fe->lp.d + fe->lp_o_track, bytes, hipMemcpyDeviceToHost));
    if (track_right) HIPCHK(hipMemcpy(track_right, fe->lp.d + fe->lp_o_track_r, bytes, hipMemcpyDeviceToHost));
    const int rc = vslamh_local_points_finish((const int32_t*)(h + fe->lp_o_res), N, idx, cnt[2], fe->lp_cap, match_cur);
    if (rc == VSLAM_ERR_UNSUPPORTED)
        g_err = "SearchLocalPoints: more than 4096 MapPoints in view; SearchByProjection on the device takes at most 4096";
    else if (rc)
        g_err = "invalid arguments";
    else
        *nmatches = cnt[0];
    return rc;
}

extern "C" int vslam_search_local_points_rig(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                             const vslam_map_point* points, const uint8_t* mp_desc, int n_mp, int points_where,
                                             const vslam_rig_frame* frame, float th, float nnratio, int32_t* match_cur,
                                             int* nmatches, int* n_to_match, int* n_matched_against, vslam_mp_track* track_left,
                                             vslam_mp_track* track_right) {
    if (!nmatches || !n_to_match || !n_matched_against || (frame && frame->n_left + frame->n_right > 0 && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_search_local_points_rig_async(fe, p, rig, points, mp_desc, n_mp, points_where, frame, th, nnratio);
    if (rc) return rc;
    return vslam_search_local_points_rig_wait(fe, match_cur, nmatches, n_to_match, n_matched_against, track_left, track_right);
}

/* with vslam_fe_set_profiling on: HIP-event time of the two-job k_sbp_rank launch and of k_rig_resolve alone, summed over the
 * rig searches waited for since */
extern "C" int vslam_fe_get_local_points_rig_profile(vslam_fe* fe, double* rank_ms, double* resolve_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (rank_ms) *rank_ms = fe->rig_ms[0];
    if (resolve_ms) *resolve_ms = fe->rig_ms[1];
    if (passes) *passes = fe->rig_passes;
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ SearchByProjection(CurrentFrame, LastFrame): rig
 * fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1.  Ranking is k_sbp_rank_rig (query mode 4) as two jobs of one launch over
 * the same last-frame arrays -- job 0 against the left keypoints, job 1 against the right ones --, resolution and the joint
 * finish k_sbp_rig_resolve / k_sbp_rig_replay (vslam_projection_kernels.hip). */
extern "C" int vslam_search_by_projection_frame_rig_async(vslam_fe* fe, const vslam_proj_params* p, const vslam_kb8_rig* rig,
                                                          const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                                          const float* last_x3dw, const uint8_t* mp_desc_host,
                                                          const vslam_rig_frame* cur) {
    if (!fe || !p || !rig || !cur || n_last < 0 || cur->n_left < 0 || cur->n_right < 0 ||
        (cur->n_left && (!cur->dev_kps_left || !cur->dev_desc_left)) ||
        (cur->n_right && (!cur->dev_kps_right || !cur->dev_desc_right)) ||
        (n_last && (!last_kps_host || !last_flags || !last_x3dw || !mp_desc_host)) || p->img_w < 1 || p->img_h < 1 ||
        !std::isfinite(p->th)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(rig->Trl[i]) || !std::isfinite(p->Tcw[i])) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    if (!fe->has_kb8) {
        g_err = "no KB8 camera set (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (vslamh_frame_rig_camera_check(p, &fe->kb8)) {
        g_err = "fx, fy, cx, cy of the projection parameters differ from the KB8 camera's (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (fe->fr_state == 1) {
        g_err = "a rig frame search is already in flight (vslam_search_by_projection_frame_rig_wait)";
        return VSLAM_ERR_INVALID;
    }
    if (n_last > 4096 || cur->n_left > 4096 || cur->n_right > 4096) { /* the 12-bit index of the ordering key */
        g_err = "SearchByProjection on the device supports at most 4096 last-frame entries and 4096 keypoints per camera";
        return VSLAM_ERR_UNSUPPORTED;
    }
    const int N = cur->n_left + cur->n_right;
    fe->fr_n_cur = N;
    if (n_last == 0 || N == 0) {
        fe->fr_state = 2;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    /* inputs (one upload): kps | x3Dw | mpDesc | flags | occupied; then the scratch of both sides | match table | nmatches, needSeq */
    const size_t nl = (size_t)n_last, nc = (size_t)N;
    const auto [o_kps, o_x, o_d, o_f, o_o, o_sl, o_sr, o_m, o_n, total] =
        vslam::layout(16, {nl * sizeof(vslam_kp), nl * 12, nl * 32, nl, nc, vk_sbp_scratch_bytes(n_last, M),
                           vk_sbp_scratch_bytes(n_last, M), nc * 4, 16});
    if ((rc = fe->fr.ensure(total))) return rc;
    const bool prof = fe->profiling;
    for (int i = 0; i < 3 && prof; i++)
        if (int rc = fe->ev_fr[i].ensure()) return rc;
    uint8_t *h = fe->fr.h, *d = fe->fr.d;
    memcpy(h + o_kps, last_kps_host, nl * sizeof(vslam_kp));
    memcpy(h + o_x, last_x3dw, nl * 12);
    memcpy(h + o_d, mp_desc_host, nl * 32);
    memcpy(h + o_f, last_flags, nl);
    if (cur->occupied_host) memcpy(h + o_o, cur->occupied_host, nc);
    hipStream_t st = fe->stream;
    fe->fr.up(st, 0, o_sl);
    SbpJobs JS;
    sbp_jobs_header(fe, M, &JS);
    for (int side = 0; side < 2; side++) {
        SbpJobDev& J = JS.job[side];
        sbp_job_camera(fe, *p, &J); /* fx .. cy and mbf travel but are not read: both sides project through R.cam */
        J.mode = 4;
        J.nLast = n_last;
        J.nCur = side == 0 ? cur->n_left : cur->n_right;
        J.lastKps = (const vslam_kp*)(d + o_kps);
        J.flags = d + o_f;
        J.x3Dw = (const float*)(d + o_x);
        J.mpDesc = d + o_d;
        J.curKps = side == 0 ? cur->dev_kps_left : cur->dev_kps_right;
        J.curDesc = side == 0 ? cur->dev_desc_left : cur->dev_desc_right;
        sbp_job_outputs(&J, d + (side == 0 ? o_sl : o_sr), n_last, nullptr, nullptr, nullptr);
    }
    RigFrameDev R;
    memset(&R, 0, sizeof(R));
    R.cam = fe->kb8;
    memcpy(R.Trl, rig->Trl, sizeof(R.Trl));
    R.nLeft = cur->n_left;
    R.nRight = cur->n_right;
    R.forceSeq = fe->tune.sbp_sequential == 1;
    R.occupied0 = cur->occupied_host ? d + o_o : nullptr;
    R.matchCur = (int32_t*)(d + o_m);
    R.nmatches = (int32_t*)(d + o_n);
    R.needSeq = (int32_t*)(d + o_n) + 1;
    R.fallbacks = fe->d_init_fb;
    if (prof) (void)hipEventRecord(fe->ev_fr[0], st);
    vk_search_frame_rig(st, JS, R, n_last, prof ? (hipEvent_t)fe->ev_fr[1] : nullptr);
    if (prof) (void)hipEventRecord(fe->ev_fr[2], st);
    fe->fr_timed = prof;
    HIPCHK(hipGetLastError());
    fe->fr.down(st, o_m, total - o_m);
    HIPCHK(hipGetLastError());
    fe->fr_state = 1;
    fe->fr_o_m = o_m;
    fe->fr_o_n = o_n;
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_frame_rig_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches) {
    if (!fe || fe->fr_state == 0) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    const int N = fe->fr_n_cur;
    if (!nmatches || (N && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = 0;
    if (fe->fr_state == 2) { /* no last-frame entries or no keypoints: nothing was launched */
        fe->fr_state = 0;
        for (int i = 0; i < N; i++) match_cur[i] = -1;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    fe->fr_state = 0;
    HIPCHK(vslam_stream_wait(fe->stream));
    if (fe->fr_timed) {
        float a = 0.0f, b = 0.0f;
        fe->fr_timed = false;
        HIPCHK(hipEventElapsedTime(&a, fe->ev_fr[0], fe->ev_fr[1]));
        HIPCHK(hipEventElapsedTime(&b, fe->ev_fr[1], fe->ev_fr[2]));
        fe->fr_ms[0] += a;
        fe->fr_ms[1] += b;
        fe->fr_passes++;
    }
    memcpy(match_cur, fe->fr.h + fe->fr_o_m, (size_t)N * 4);
    *nmatches = *(const int32_t*)(fe->fr.h + fe->fr_o_n);
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_frame_rig(vslam_fe* fe, const vslam_proj_params* p, const vslam_kb8_rig* rig,
                                                    const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                                    const float* last_x3dw, const uint8_t* mp_desc_host,
                                                    const vslam_rig_frame* cur, int32_t* match_cur, int* nmatches) {
    if (!nmatches || (cur && cur->n_left + cur->n_right > 0 && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_search_by_projection_frame_rig_async(fe, p, rig, last_kps_host, n_last, last_flags, last_x3dw, mp_desc_host, cur);
    if (rc) return rc;
    return vslam_search_by_projection_frame_rig_wait(fe, match_cur, nmatches);
}

/* with vslam_fe_set_profiling on: HIP-event time of the two-job k_sbp_rank_rig launch and of k_sbp_rig_resolve + k_sbp_rig_replay,
 * summed over the rig frame searches waited for since */
extern "C" int vslam_fe_get_frame_rig_profile(vslam_fe* fe, double* rank_ms, double* resolve_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (rank_ms) *rank_ms = fe->fr_ms[0];
    if (resolve_ms) *resolve_ms = fe->fr_ms[1];
    if (passes) *passes = fe->fr_passes;
    return VSLAM_OK;
}
