/* vslam_fuse_rig.hip -- the search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame and for both
 * cameras of a two-fisheye rig (fmatcher.cpp:1918-2119 with pKF->NLeft != -1; the Scw overload :2121-2243 as sim3 = 1): one
 * MapPoint list against up to 16 (KeyFrame, camera) jobs in one enqueue.  The rules are stated in include/vslam_fe.h above
 * vslam_fuse_rig_job; the kernel is k_fuse_rank_rig (vslam_projection_kernels.hip), the host twin vslamh_fuse_search_rig
 * (vslam_match_host.cpp).  The staging block fe->fsr is this entry's own: the blocking matchers, which fill fe->proj on the host at
 * once, can run while a search is in flight. */
#include "vslam_sbp_host.h"

static bool fsr_finite(const float* v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int vslam_fuse_search_rig_async(vslam_fe* fe, const vslam_fuse_params* p, const vslam_kb8_rig* rig,
                                           const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                           const uint8_t* mp_desc, int n_points, int points_where) {
    static_assert(sizeof(vslam_fuse_point) == sizeof(FusePoint), "vslam_fuse_point layout");
    static_assert(VSLAM_FUSE_RIG_MAX_JOBS == VSLAM_MAX_FUSE_RIG_JOBS, "the argument block holds every job");
    static_assert(sizeof(FuseRigArgs) <= 4000, "FuseRigArgs travels as a kernel argument");
    if (!fe || !p || !jobs || n_jobs < 1 || n_jobs > VSLAM_FUSE_RIG_MAX_JOBS || n_points < 0 ||
        (n_points && (!points || !mp_desc)) || (points_where != VSLAM_IMGS_HOST && points_where != VSLAM_IMGS_DEVICE) ||
        p->img_w < 1 || p->img_h < 1 || !std::isfinite(p->th) || !std::isfinite(p->log_scale_factor)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    bool needs_rig = false;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        if (s.camera < 0 || s.camera > 1 || s.sim3 < 0 || s.sim3 > 1 || (s.sim3 && s.camera) || s.n_kf < 0 ||
            (s.n_kf && (!s.dev_kps || !s.dev_desc)) || !fsr_finite(s.Rcw, 9) || !fsr_finite(s.tcw, 3) || !fsr_finite(s.Ow, 3)) {
            g_err = "invalid job: camera 0 / 1, sim3 0 / 1 with camera 0, device arrays for n_kf keypoints, a finite pose";
            return VSLAM_ERR_INVALID;
        }
        if (s.n_kf && ((((uintptr_t)s.dev_desc) & 15) || (((uintptr_t)s.dev_kps) & 3))) { /* uint4 reads of the rows */
            g_err = "a job's dev_desc must be 16-byte aligned, its dev_kps 4-byte aligned";
            return VSLAM_ERR_INVALID;
        }
        needs_rig = needs_rig || s.camera == 1;
    }
    if (needs_rig && (!rig || !vslam_kb8::camera_ok(&rig->cam2))) {
        g_err = "a job names camera 1: the rig with its right camera is needed";
        return VSLAM_ERR_INVALID;
    }
    if (points_where == VSLAM_IMGS_DEVICE && n_points && ((((uintptr_t)mp_desc) & 15) || (((uintptr_t)points) & 3))) {
        g_err = "device MapPoint descriptors must be 16-byte aligned, device MapPoints 4-byte aligned";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_required(fe)) return rc;
    if (int rc = fe->fsr_op.begin("a rig Fuse search is already in flight (vslam_fuse_search_rig_wait)")) return rc;
    if (n_points > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "Fuse on the device supports at most VSLAM_LOCAL_POINTS_MAX MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    int max_kf = 0;
    for (int j = 0; j < n_jobs; j++) max_kf = std::max(max_kf, jobs[j].n_kf);
    if (max_kf > 4096) { /* the 12-bit index of the ordering key */
        g_err = "Fuse on the device supports at most 4096 keypoints per KeyFrame camera";
        return VSLAM_ERR_UNSUPPORTED;
    }
    fe->fsr_op.jobs = n_jobs;
    fe->fsr_op.n = n_points;
    if (n_points == 0 || max_kf == 0) {
        fe->fsr_op.set(true);
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M); /* the kernels' LDS limit */
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const size_t np = (size_t)n_points;
    /* inputs (one upload): points | descriptors (host points only) | validity bytes of the jobs that carry them; then best_idx |
     * best_dist of every job (one copy) */
    size_t sizes[2 + VSLAM_FUSE_RIG_MAX_JOBS + 2], off[2 + VSLAM_FUSE_RIG_MAX_JOBS + 2];
    int k = 0;
    sizes[k++] = from_host ? np * sizeof(FusePoint) : 0;
    sizes[k++] = from_host ? np * 32 : 0;
    for (int j = 0; j < n_jobs; j++) sizes[k++] = jobs[j].valid_host ? np : 0;
    const int k_bi = k;
    sizes[k++] = (size_t)n_jobs * np * 4;
    sizes[k++] = (size_t)n_jobs * np * 4;
    const size_t total = vslam::layout_parts(16, sizes, k, off);
    if ((rc = fe->fsr.ensure(total))) return rc;
    if ((rc = fe->t_fsr.arm(fe->profiling))) return rc;
    uint8_t *h = fe->fsr.h, *d = fe->fsr.d;
    if (from_host) {
        memcpy(h + off[0], points, np * sizeof(FusePoint));
        memcpy(h + off[1], mp_desc, np * 32);
    }
    FuseRigArgs A;
    memset(&A, 0, sizeof(A));
    bool any_valid = false;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        FuseRigJobDev& J = A.job[j];
        memcpy(J.Rcw, s.Rcw, sizeof(J.Rcw));
        memcpy(J.tcw, s.tcw, sizeof(J.tcw));
        memcpy(J.Ow, s.Ow, sizeof(J.Ow));
        J.camera = s.camera;
        J.sim3 = s.sim3;
        J.nKF = s.n_kf;
        J.idxOffset = s.idx_offset;
        J.kps = s.dev_kps;
        J.desc = s.dev_desc;
        if (s.valid_host) {
            memcpy(h + off[2 + j], s.valid_host, np);
            J.valid = d + off[2 + j];
            any_valid = true;
        }
    }
    A.cam[0] = fe->kb8;
    A.cam[1] = needs_rig ? rig->cam2 : fe->kb8;
    for (int l = 0; l < fe->p.nlevels; l++) {
        A.scale[l] = fe->tab.scale[l];
        A.invSigma2[l] = fe->tab.inv_sigma2[l];
    }
    A.th = p->th;
    A.logScaleFactor = p->log_scale_factor;
    A.bnd = matcher_bounds(fe, p->img_w, p->img_h);
    A.gemmFloat = p->gemm_float;
    A.nlevels = fe->p.nlevels;
    A.nPoints = n_points;
    A.pts = from_host ? (const FusePoint*)(d + off[0]) : (const FusePoint*)points;
    A.mpDesc = from_host ? d + off[1] : mp_desc;
    A.bestIdx = (int32_t*)(d + off[k_bi]);
    A.bestDist = (int32_t*)(d + off[k_bi + 1]);
    hipStream_t st = fe->stream;
    if (from_host || any_valid) fe->fsr.up(st, 0, off[k_bi]);
    fe->t_fsr.mark(0, st);
    vk_fuse_search_rig(st, A, n_jobs, max_kf);
    fe->t_fsr.mark(1, st);
    HIPCHK(hipGetLastError());
    fe->fsr.down(st, off[k_bi], total - off[k_bi]);
    HIPCHK(hipGetLastError());
    fe->fsr_op.set(false);
    fe->fsr_o_bi = off[k_bi];
    fe->fsr_o_bd = off[k_bi + 1];
    return VSLAM_OK;
}

extern "C" int vslam_fuse_search_rig_wait(vslam_fe* fe, int32_t* best_idx, int32_t* best_dist) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->fsr_op.ready()) return rc;
    const size_t n = (size_t)fe->fsr_op.jobs * (size_t)fe->fsr_op.n;
    if (n && (!best_idx || !best_dist)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (fe->fsr_op.take()) { /* no MapPoints or no keypoints: nothing was launched */
        for (size_t i = 0; i < n; i++) {
            best_idx[i] = -1;
            best_dist[i] = 256;
        }
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    if (int rc = fe->t_fsr.collect()) return rc;
    memcpy(best_idx, fe->fsr.h + fe->fsr_o_bi, n * 4);
    memcpy(best_dist, fe->fsr.h + fe->fsr_o_bd, n * 4);
    return VSLAM_OK;
}

extern "C" int vslam_fuse_search_rig(vslam_fe* fe, const vslam_fuse_params* p, const vslam_kb8_rig* rig,
                                     const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                     const uint8_t* mp_desc, int n_points, int points_where, int32_t* best_idx,
                                     int32_t* best_dist) {
    if (n_jobs >= 1 && n_points > 0) { /* what a refusal leaves behind, more than 16 jobs included: the caller sized by n_jobs */
        if (!best_idx || !best_dist) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
        const size_t n = (size_t)n_jobs * (size_t)n_points;
        for (size_t i = 0; i < n; i++) {
            best_idx[i] = -1;
            best_dist[i] = 256;
        }
    }
    int rc = vslam_fuse_search_rig_async(fe, p, rig, jobs, n_jobs, points, mp_desc, n_points, points_where);
    if (rc) return rc;
    return vslam_fuse_search_rig_wait(fe, best_idx, best_dist);
}

extern "C" int vslam_fe_get_fuse_rig_profile(vslam_fe* fe, double* rank_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    fe->t_fsr.read({rank_ms}, passes);
    return VSLAM_OK;
}
