/* vslam_sbp_host.h -- private: the host-side statics that the entry points around k_sbp_* share across files.  All are
 * `static inline`; each entry point's own helpers stay in its file.
 *   who uses what                                vslam_projection  vslam_local_points  vslam_projection_rig  vslam_bow_rig
 *   sbp_prepare, sbp_jobs_header, sbp_job_outputs        x                 x                    x
 *   sbp_job_camera                                       x                                      x
 *   sbp_nnratio_refuse                                   x                 x                    x
 *   rig_ok                                                                 x
 *   kb8_required                                                           x                    x
 *   rig_frame_ptrs_ok                                                                           x                  x
 *   rig_frame_check, rig_frame_stage, rig_jobs                             x                    x
 * vslam_fuse_rig uses sbp_prepare (the LDS limit) and kb8_required. */
#ifndef VSLAM_SBP_HOST_H
#define VSLAM_SBP_HOST_H
#include "vslam_ctx.h"
#include "vslam_kb8.h"

/* ---- what every entry point of the family does around k_sbp_* (vk_search_by_projection) ---- */
/* once per context: the kernels' LDS limit and the re-scan counters; *M_out = length of the sorted candidate prefix */
static inline int sbp_prepare(vslam_fe* fe, int* M_out) {
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
static inline void sbp_jobs_header(const vslam_fe* fe, int M, SbpJobs* JS) {
    static_assert(sizeof(SbpJobs) <= 4000, "SbpJobs travels as a kernel argument");
    memset(JS, 0, sizeof(*JS));
    for (int l = 0; l < fe->p.nlevels; l++) JS->scale[l] = fe->tab.scale[l];
    JS->nlevels = fe->p.nlevels;
    JS->M = M;
}

/* pose, camera, window and switches of a job that projects with vslam_proj_params (modes 0, 2, 3, 4) */
static inline void sbp_job_camera(const vslam_fe* fe, const vslam_proj_params& p, SbpJobDev* J) {
    memcpy(J->Tcw, p.Tcw, sizeof(J->Tcw));
    J->fx = p.fx; J->fy = p.fy; J->cx = p.cx; J->cy = p.cy; J->mbf = p.mbf; J->th = p.th;
    J->forward = p.forward != 0; J->backward = p.backward != 0; J->checkOri = p.check_orientation != 0;
    J->bnd = matcher_bounds(fe, p.img_w, p.img_h); J->gemmFloat = p.gemm_float != 0;
}

/* a job's scratch at scr (proj | topm of n_last candidates, vk_sbp_scratch_bytes) and its result words */
static inline void sbp_job_outputs(SbpJobDev* J, uint8_t* scr, int n_last, int32_t* match_cur, int32_t* nmatches, int32_t* need_seq) {
    J->proj = (SbpProj*)scr;
    J->topm = (uint32_t*)(scr + vk_sbp_proj_bytes(n_last));
    J->matchCur = match_cur;
    J->nmatches = nmatches;
    J->needSeq = need_seq;
}

/* the mode-1 matchers: keys clamp distances to 255; exact for bestDist <= 100 when 0.4 * 255 > 100 */
static inline int sbp_nnratio_refuse(float nnratio) {
    if (nnratio >= 0.4f) return VSLAM_OK;
    g_err = "SearchByProjection on the device needs nnratio >= 0.4";
    return VSLAM_ERR_UNSUPPORTED;
}

/* ---- a two-fisheye rig ---- */
/* finite Tlr / Trl and a usable right camera */
static inline bool rig_ok(const vslam_kb8_rig* rig) {
    if (!rig || !vslam_kb8::camera_ok(&rig->cam2)) return false;
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(rig->Tlr[i]) || !std::isfinite(rig->Trl[i])) return false;
    return true;
}

/* the rig entry points project the left side with the context's own KB8 camera */
static inline int kb8_required(const vslam_fe* fe) {
    if (fe->has_kb8) return VSLAM_OK;
    g_err = "no KB8 camera set (vslam_fe_set_kb8_camera)";
    return VSLAM_ERR_INVALID;
}

/* counts and device arrays of a vslam_rig_frame; sizes and maps are the caller's business */
static inline bool rig_frame_ptrs_ok(const vslam_rig_frame* f) {
    return f && f->n_left >= 0 && f->n_right >= 0 && (!f->n_left || (f->dev_kps_left && f->dev_desc_left)) &&
           (!f->n_right || (f->dev_kps_right && f->dev_desc_right));
}

/* a rig frame of the mode-1 matchers: arrays, the 12-bit index of the ordering key, the maps between the cameras */
static inline int rig_frame_check(const vslam_rig_frame* f) {
    if (!rig_frame_ptrs_ok(f)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (f->n_left > 4096 || f->n_right > 4096) {
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
static inline void rig_frame_stage(const vslam_rig_frame& f, uint8_t* h, size_t o_l, size_t o_r, size_t o_o) {
    if (f.n_left) memcpy(h + o_l, f.left_to_right_host, (size_t)f.n_left * 4);
    if (f.n_right) memcpy(h + o_r, f.right_to_left_host, (size_t)f.n_right * 4);
    if (f.occupied_host) memcpy(h + o_o, f.occupied_host, (size_t)f.n_left + (size_t)f.n_right);
}

/* the two ranking jobs and the resolver's arguments over device arrays: records, descriptors and flags of n_mp MapPoints
 * (n_mp_ptr: their count in HBM, or null), scratch of vk_sbp_scratch_bytes(n_mp, M) per side */
static inline void rig_jobs(const vslam_fe* fe, int M, const vslam_rig_frame& f, int img_w, int img_h, float th, float nnratio,
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

#endif
