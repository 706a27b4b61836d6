/* vslam_projection_rig.hip -- the SearchByProjection family for a two-fisheye rig (Nleft != -1): SearchByProjection(F,
 * vpMapPoints) from caller-made records and SearchByProjection(CurrentFrame, LastFrame).  SearchLocalPoints of a rig, which
 * puts the frustum stage in front of the former, is in vslam_local_points.hip. */
#include "vslam_sbp_host.h"

/* ------------------------------------------------------------------ SearchByProjection(F, vpMapPoints): rig
 * fmatcher.cpp:321-491 with Nleft != -1.  Ranking is k_sbp_rank mode 1 as two jobs of one launch (left keypoints with the
 * caller's th, right keypoints with th = 1); the coupled resolution is k_rig_resolve (vslam_projection_kernels.hip). */
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
    if (int rc = sbp_nnratio_refuse(nnratio)) return rc;
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

/* ------------------------------------------------------------------ SearchByProjection(CurrentFrame, LastFrame): rig
 * fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1.  Ranking is k_sbp_rank_rig (query mode 4) as two jobs of one launch over
 * the same last-frame arrays -- job 0 against the left keypoints, job 1 against the right ones --, resolution and the joint
 * finish k_sbp_rig_resolve / k_sbp_rig_replay (vslam_projection_kernels.hip). */
extern "C" int vslam_search_by_projection_frame_rig_async(vslam_fe* fe, const vslam_proj_params* p, const vslam_kb8_rig* rig,
                                                          const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                                          const float* last_x3dw, const uint8_t* mp_desc_host,
                                                          const vslam_rig_frame* cur) {
    if (!fe || !p || !rig || !rig_frame_ptrs_ok(cur) || n_last < 0 ||
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
    if (int rc = kb8_required(fe)) return rc;
    if (vslamh_frame_rig_camera_check(p, &fe->kb8)) {
        g_err = "fx, fy, cx, cy of the projection parameters differ from the KB8 camera's (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->fr_op.begin("a rig frame search is already in flight (vslam_search_by_projection_frame_rig_wait)")) return rc;
    if (n_last > 4096 || cur->n_left > 4096 || cur->n_right > 4096) { /* the 12-bit index of the ordering key */
        g_err = "SearchByProjection on the device supports at most 4096 last-frame entries and 4096 keypoints per camera";
        return VSLAM_ERR_UNSUPPORTED;
    }
    const int N = cur->n_left + cur->n_right;
    fe->fr_op.n = N;
    if (n_last == 0 || N == 0) {
        fe->fr_op.set(true);
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
    if ((rc = fe->t_fr.arm(fe->profiling))) return rc;
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
    fe->t_fr.mark(0, st);
    vk_search_frame_rig(st, JS, R, n_last, fe->t_fr.event(1));
    fe->t_fr.mark(2, st);
    HIPCHK(hipGetLastError());
    fe->fr.down(st, o_m, total - o_m);
    HIPCHK(hipGetLastError());
    fe->fr_op.set(false);
    fe->fr_o_m = o_m;
    fe->fr_o_n = o_n;
    return VSLAM_OK;
}

extern "C" int vslam_search_by_projection_frame_rig_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->fr_op.ready()) return rc;
    const int N = fe->fr_op.n;
    if (!nmatches || (N && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *nmatches = 0;
    if (fe->fr_op.take()) { /* no last-frame entries or no keypoints: nothing was launched */
        for (int i = 0; i < N; i++) match_cur[i] = -1;
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    if (int rc = fe->t_fr.collect()) return rc;
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
    fe->t_fr.read({rank_ms, resolve_ms}, passes);
    return VSLAM_OK;
}
