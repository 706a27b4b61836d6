/* vslam_projection.hip -- the matchers that project MapPoints into a frame: the SearchByProjection family (frame, KeyFrame,
 * Sim3, map points; host-staged and device-resident), the search half of Fuse and MapPoint::ComputeDistinctiveDescriptors.
 * Frame::isInFrustum / SearchLocalPoints are in vslam_local_points.hip, the forms for a two-fisheye rig in
 * vslam_projection_rig.hip.  Every entry stages through a vslam_staging block (vslam_staging.h). */
#include "vslam_sbp_host.h" /* sbp_prepare, sbp_jobs_header, sbp_job_camera, sbp_job_outputs: shared with those two */

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

/* One job in fe->proj to its end: launch, [o_m, end) -- the match table, then at o_n nmatches | needSeq -- to the mirror,
 * wait, hand out. */
static int sbp_run_single(vslam_fe* fe, const SbpJobs& JS, int n_last, int n_cur, size_t o_m, size_t o_n, size_t end,
                          int32_t* match_cur, int* nmatches, bool kb8 = false) {
    hipStream_t st = fe->stream;
    const int force_seq = fe->tune.sbp_sequential == 1; /* cross-check path */
    if (kb8) vk_search_by_projection_kb8(st, JS, 1, n_last, n_cur, fe->d_init_fb, force_seq, fe->kb8);
    else vk_search_by_projection(st, JS, 1, n_last, n_cur, fe->d_init_fb, force_seq);
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
    bool kb8 = false; /* mode 2 of a fisheye CurrentFrame: KannalaBrandt8::project with the context's camera (k_sbp_rank_kb8) */
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
    if (kf && kf->kb8) {
        if (int rc = kb8_required(fe)) return rc;
        if (vslamh_frame_rig_camera_check(p, &fe->kb8)) {
            g_err = "fx, fy, cx, cy of the projection parameters differ from the KB8 camera's (vslam_fe_set_kb8_camera)";
            return VSLAM_ERR_INVALID;
        }
    } else if (int rc = kb8_refuse(fe)) {
        return rc;
    }
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
    return sbp_run_single(fe, JS, n_last, n_cur, o_m, o_n, total, match_cur, nmatches, kf && kf->kb8);
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

/* The same matcher with a fisheye CurrentFrame -- a monocular KB8 frame or the left camera of a two-fisheye rig, whose bRight
 * defaults to false (frame.cpp:678-744): k_sbp_rank_kb8 in front of the same resolution.  Rules, and the oddity of the
 * reference's angle read for a rig KeyFrame, in include/vslam_fe.h */
extern "C" int vslam_search_by_projection_keyframe_kb8(vslam_fe* fe, const vslam_proj_params* p, const float* Ow,
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
        g_err = "SearchByProjection on the device supports at most 4096 KeyFrame entries";
        return VSLAM_ERR_UNSUPPORTED;
    }
    SbpKfExtras kf;
    kf.min_dist = mp_min_dist;
    kf.max_dist = mp_max_dist;
    for (int i = 0; i < 3; i++) kf.ow[i] = Ow[i];
    kf.log_scale_factor = log_scale_factor;
    kf.orb_dist = orb_dist;
    kf.kb8 = true;
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
    if (int rc = sbp_nnratio_refuse(nnratio)) return rc;
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
