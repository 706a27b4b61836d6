/* vslam_local_points.hip -- Frame::isInFrustum and Tracking::SearchLocalPoints on the device, for one camera and for a
 * two-fisheye rig: vslam_frame_in_frustum[_rig], vslam_search_local_points[_rig][_async / _wait] and their profile getters.
 * All of them stage through fe->lp; an enqueued search holds the block until its _wait (fe->lp_op). */
#include "vslam_sbp_host.h"
#include "vslam_frustum.h"

/* ------------------------------------------------------------------ Frame::isInFrustum + SearchLocalPoints
 * The frustum stage (vslam_frustum.hip) in front of the matcher of vslam_search_by_projection_mappoints.  k_sbp_rank,
 * k_sbpm_resolve and k_sbpm_replay read their MapPoint count as min(*nLastPtr, nLast) in mode 1 exactly as in mode 0, so the
 * matcher is enqueued behind the compaction with nLast = the capacity and nLastPtr = the clamped count in HBM: no host
 * wait between the stages. */
/* a local-points search, rig or not, holds fe->lp until its _wait: the blocking frustum entries refuse */
static int lp_busy_refuse(const vslam_fe* fe) {
    return fe->lp_op.begin("a local-points search is in flight (vslam_search_local_points_wait)");
}

/* chunks of VSLAM_FRUSTUM_CHUNK MapPoints, and the sum of their in-view counts */
static int frustum_chunks(int n) { return (n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK; }
static int chunks_in_view(const uint8_t* counts, int nchunks) {
    int nv = 0;
    for (int c = 0; c < nchunks; c++) nv += ((const int32_t*)counts)[c];
    return nv;
}

/* what both _async entries refuse about their MapPoints: misaligned device arrays, and -- behind the entry's own refusal
 * of a second search in flight -- too many */
static int lp_points_check(const vslam_map_point* points, const uint8_t* mp_desc, int n_mp, int points_where) {
    if (points_where == VSLAM_IMGS_DEVICE && n_mp && ((((uintptr_t)mp_desc) & 15) || (((uintptr_t)points) & 3))) {
        g_err = "device MapPoint descriptors must be 16-byte aligned, device MapPoints 4-byte aligned";
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}
static int lp_count_check(int n_mp) {
    if (n_mp <= VSLAM_LOCAL_POINTS_MAX) return VSLAM_OK;
    g_err = "SearchLocalPoints on the device supports at most 65536 MapPoints per call";
    return VSLAM_ERR_UNSUPPORTED;
}

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
    if (int rc = lp_busy_refuse(fe)) return rc;
    HIPCHK(hipSetDevice(fe->p.device));
    const int nchunks = frustum_chunks(n);
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
    *n_in_view = chunks_in_view(h + o_cv, nchunks);
    return VSLAM_OK;
}

/* Frame::isInFrustum of a two-fisheye rig (Nleft != -1): one upload, k_frustum_rig, one copy of both record arrays, both
 * depth arrays and the chunk counts */
extern "C" int vslam_frame_in_frustum_rig(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                          const vslam_map_point* points_host, int n, vslam_mp_track* track_left,
                                          vslam_mp_track* track_right, float* depth_left, float* depth_right, int* n_in_view) {
    if (!fe || !rig_ok(rig) || !n_in_view || n < 0 || (n && (!points_host || !track_left || !track_right)) ||
        !frustum_params_ok(p)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_required(fe)) return rc;
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    *n_in_view = 0;
    if (n == 0) return VSLAM_OK;
    if (n > VSLAM_LOCAL_POINTS_MAX) {
        g_err = "Frame::isInFrustum on the device supports at most 65536 MapPoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (int rc = lp_busy_refuse(fe)) return rc;
    HIPCHK(hipSetDevice(fe->p.device));
    const int nchunks = frustum_chunks(n);
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
    *n_in_view = chunks_in_view(h + o_cv, nchunks);
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
    if (int rc = lp_points_check(points, mp_desc, n_mp, points_where)) return rc;
    if (int rc = fe->lp_op.begin("a local-points search is already in flight (vslam_search_local_points_wait)")) return rc;
    if (int rc = lp_count_check(n_mp)) return rc;
    if (n_cur > 4096) {
        g_err = "SearchByProjection on the device supports at most 4096 keypoints per call";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (int rc = sbp_nnratio_refuse(nnratio)) return rc;
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    fe->lp_n_mp = n_mp;
    fe->lp_op.n = n_cur;
    if (n_mp == 0 || n_cur == 0) {
        fe->lp_op.set(true, LP_SINGLE);
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const int cap = std::min(n_mp, VSLAM_FRUSTUM_MAX_KEPT);
    const int nchunks = frustum_chunks(n_mp);
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
    /* vslam_fe_set_profiling: the two kernels' own spans (vslam_fe_get_local_points_profile) */
    if ((rc = fe->t_lp.arm(fe->profiling))) return rc;
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
    fe->t_lp.mark(0, st);
    frustum_launch(fe, st, A);
    fe->t_lp.mark(1, st);
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
    fe->t_lp.mark(2, st);
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
    fe->lp_op.set(false, LP_SINGLE);
    fe->lp_cap = cap;
    fe->lp_o_track = o_track;
    fe->lp_o_res = o_m;
    fe->lp_o_cnt = o_cnt;
    fe->lp_o_idx = o_idx;
    return VSLAM_OK;
}

/* The front of both waits, behind lp_op.ready() and the wait's own argument check: outputs zeroed, then either the empty
 * search's result (*done = true; want_track: the caller asked for records, which an empty search does not have) or idle,
 * the stream wait and the spans of `timer`. */
static int lp_wait_front(vslam_fe* fe, vslam_span_timer<2>& timer, int32_t* match_cur, int* nmatches, int* n_to_match,
                         int* n_matched_against, bool want_track, const char* no_records_msg, bool* done) {
    *nmatches = *n_to_match = *n_matched_against = 0;
    *done = fe->lp_op.take();
    if (*done) { /* no MapPoints or no keypoints: nothing was launched */
        for (int i = 0; i < fe->lp_op.n; i++) match_cur[i] = -1;
        if (want_track && fe->lp_n_mp) { /* async launched nothing and kept no inputs: there are no records to hand out */
            g_err = no_records_msg;
            return VSLAM_ERR_INVALID;
        }
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    return timer.collect();
}

/* The tail of both waits: counts, the records asked for (track_right: a rig search's second array), the match table in the
 * caller's indices, or the refusal of more points in view than the matcher takes. */
static int lp_wait_tail(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match, int* n_matched_against,
                        vslam_mp_track* track, vslam_mp_track* track_right) {
    const uint8_t* h = fe->lp.h;
    const int32_t* cnt = (const int32_t*)(h + fe->lp_o_cnt);
    const int32_t* idx = (const int32_t*)(h + fe->lp_o_idx);
    *n_matched_against = cnt[2];
    *n_to_match = cnt[4];
    const size_t bytes = (size_t)fe->lp_n_mp * sizeof(vslam_mp_track);
    if (track) HIPCHK(hipMemcpy(track, fe->lp.d + fe->lp_o_track, bytes, hipMemcpyDeviceToHost));
    if (track_right) HIPCHK(hipMemcpy(track_right, fe->lp.d + fe->lp_o_track_r, bytes, hipMemcpyDeviceToHost));
    const int rc = vslamh_local_points_finish((const int32_t*)(h + fe->lp_o_res), fe->lp_op.n, idx, cnt[2], fe->lp_cap, match_cur);
    if (rc == VSLAM_ERR_UNSUPPORTED)
        g_err = "SearchLocalPoints: more than 4096 MapPoints in view; SearchByProjection on the device takes at most 4096";
    else if (rc)
        g_err = "invalid arguments";
    else
        *nmatches = cnt[0];
    return rc;
}

extern "C" int vslam_search_local_points_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match,
                                              int* n_matched_against, vslam_mp_track* track_out) {
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->lp_op.ready(LP_SINGLE, "the search enqueued is a rig search (vslam_search_local_points_rig_wait)")) return rc;
    if (!nmatches || !n_to_match || !n_matched_against || (fe->lp_op.n && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    bool done;
    const int rc = lp_wait_front(fe, fe->t_lp, match_cur, nmatches, n_to_match, n_matched_against, track_out != nullptr,
                                 "no records: a search without keypoints launches nothing; call vslam_frame_in_frustum for the records",
                                 &done);
    if (rc || done) return rc;
    return lp_wait_tail(fe, match_cur, nmatches, n_to_match, n_matched_against, track_out, nullptr);
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
    fe->t_lp.read({frustum_ms, compact_ms}, passes);
    return VSLAM_OK;
}

extern "C" int vslam_search_local_points_rig_async(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                                   const vslam_map_point* points, const uint8_t* mp_desc, int n_mp,
                                                   int points_where, const vslam_rig_frame* frame, float th, float nnratio) {
    if (!fe || !rig_ok(rig) || n_mp < 0 || (n_mp && (!points || !mp_desc)) ||
        (points_where != VSLAM_IMGS_HOST && points_where != VSLAM_IMGS_DEVICE) || !frustum_params_ok(p) || !std::isfinite(th)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = rig_frame_check(frame)) return rc;
    if (int rc = lp_points_check(points, mp_desc, n_mp, points_where)) return rc;
    if (int rc = kb8_required(fe)) return rc;
    if (int rc = frustum_camera_ok(fe, p)) return rc;
    if (int rc = fe->lp_op.begin("a local-points search is already in flight (vslam_search_local_points_wait / _rig_wait)"))
        return rc;
    if (int rc = lp_count_check(n_mp)) return rc;
    if (int rc = sbp_nnratio_refuse(nnratio)) return rc;
    const vslam_rig_frame& f = *frame;
    const int N = f.n_left + f.n_right;
    fe->lp_n_mp = n_mp;
    fe->lp_op.n = N;
    if (n_mp == 0 || N == 0) {
        fe->lp_op.set(true, LP_RIG);
        return VSLAM_OK;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int M;
    int rc = sbp_prepare(fe, &M);
    if (rc) return rc;
    const bool from_host = points_where == VSLAM_IMGS_HOST;
    const int cap = std::min(n_mp, VSLAM_FRUSTUM_MAX_KEPT);
    const int nchunks = frustum_chunks(n_mp);
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
    if ((rc = fe->t_rig.arm(fe->profiling))) return rc;
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
    fe->t_rig.mark(0, st);
    vk_search_rig(st, JS, A, cap, fe->t_rig.event(1));
    fe->t_rig.mark(2, st);
    HIPCHK(hipGetLastError());
    fe->lp.down(st, o_m, total - o_m); /* match table | counts | original indices */
    HIPCHK(hipGetLastError());
    fe->lp_op.set(false, LP_RIG);
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
    if (!fe) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = fe->lp_op.ready(LP_RIG, "the search enqueued is not a rig search (vslam_search_local_points_wait)")) return rc;
    if (!nmatches || !n_to_match || !n_matched_against || (fe->lp_op.n && !match_cur)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    bool done;
    const int rc = lp_wait_front(fe, fe->t_rig, match_cur, nmatches, n_to_match, n_matched_against, track_left || track_right,
                                 "no records: a search without keypoints launches nothing; call vslam_frame_in_frustum_rig for the records",
                                 &done);
    if (rc || done) return rc;
    return lp_wait_tail(fe, match_cur, nmatches, n_to_match, n_matched_against, track_left, track_right);
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
    fe->t_rig.read({rank_ms, resolve_ms}, passes);
    return VSLAM_OK;
}
