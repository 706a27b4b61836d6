/* vslam_match_host.cpp -- see vslam_host.h: the matchers as the reference writes them, sequential.  Reference lines are
 * cited per function. */
#include "vslam_host.h"
#include "vslam_kb8.h"
#include "vslam_two_view.h"
#include "vslam_matchdev.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

/* These three are written with C names because the library's symbol list has carried them since they stood inside the C
 * block below; nothing outside this file calls them. */
extern "C" {
int rig_hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}
/* one row of R * x + t as ONE cv::gemm (double accumulation, rounded once), or in float */
float rig_gemm_row(const float* r, const float* x, float t, int flt) {
    if (!flt) {
        double s = (double)r[0] * (double)x[0];
        s = s + (double)r[1] * (double)x[1];
        s = s + (double)r[2] * (double)x[2];
        return (float)(s + (double)t);
    }
    float s = r[0] * x[0];
    s = s + r[1] * x[1];
    s = s + r[2] * x[2];
    return s + t;
}
void rig_transform(const float* T, const float* x, int flt, float* out) {
    for (int r = 0; r < 3; r++) out[r] = rig_gemm_row(T + 4 * r, x, T[4 * r + 3], flt);
}
} /* extern "C" */

namespace {
using vslam::FrameGrid;
struct RigBest {
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    void take(int dist, int level, int idx) { /* fmatcher.cpp:381-397 */
        if (dist < bestDist) {
            bestDist2 = bestDist;
            bestDist = dist;
            bestLevel2 = bestLevel;
            bestLevel = level;
            bestIdx = idx;
        } else if (dist < bestDist2) {
            bestLevel2 = level;
            bestDist2 = dist;
        }
    }
};
/* every slot unmatched; the caller's occupancy (may be NULL) as 0 / 1 */
std::vector<uint8_t> clear_matches(int32_t* match, int n, const uint8_t* occupied) {
    std::vector<uint8_t> occ((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        match[i] = -1;
        if (occupied) occ[i] = occupied[i] != 0;
    }
    return occ;
}
/* the candidate of least Hamming distance below *bestDist (the first of equals) that `skip` lets through, or -1 */
template <class Skip>
int best_candidate(const std::vector<int>& cand, const uint8_t* d, const uint8_t* desc, int* bestDist, Skip skip) {
    int bestIdx = -1;
    for (int idx : cand) {
        if (skip(idx)) continue;
        const int dist = rig_hamming(d, desc + (size_t)idx * 32);
        if (dist < *bestDist) {
            *bestDist = dist;
            bestIdx = idx;
        }
    }
    return bestIdx;
}
/* A KeyFrame's integer mnMinX, mnMaxX, mnMinY, mnMaxY: the Frame's float bounds truncated (keyframe.cpp:58-67) */
struct KfBounds {
    float b[4];
    explicit KfBounds(const float* f) : b{(float)(int)f[0], (float)(int)f[1], (float)(int)f[2], (float)(int)f[3]} {}
};
/* where a MapPoint's search window lies in a KeyFrame */
struct KfWindow {
    vslam_kb8::Uv uv;
    int level;
    float radius;
};
/* What Fuse (fmatcher.cpp:1974-2025) and SearchByProjection(pKF, Scw, ..) (:782-820) ask of a MapPoint before they open a
 * window in a fisheye KeyFrame, in their order: camera coordinates, depth, projection, KeyFrame::IsInImage, the distance range,
 * the viewing angle, the predicted level.  s: a job of either kind, for its Rcw / tcw / Ow.  false: rejected, *g is not written. */
template <class Job>
bool keyframe_gate(const Job& s, const vslam_kb8_camera& c, const KfBounds& kb, const vslam_fuse_point& mp, int gemm_float,
                   float log_scale_factor, float th, const float* scale_factors, int nlevels, KfWindow* g) {
    float pc[3];
    for (int r = 0; r < 3; r++) pc[r] = rig_gemm_row(s.Rcw + 3 * r, mp.pos, s.tcw[r], gemm_float);
    if (pc[2] < 0.0f) return false;
    const vslam_kb8::Uv uv = vslam_kb8::kb8_project(c, pc[0], pc[1], pc[2]);
    if (!(uv.u >= kb.b[0] && uv.u < kb.b[1] && uv.v >= kb.b[2] && uv.v < kb.b[3])) return false; /* KeyFrame::IsInImage */
    const float p0 = mp.pos[0] - s.Ow[0], p1 = mp.pos[1] - s.Ow[1], p2 = mp.pos[2] - s.Ow[2];
    const float dist3D = vslam_md::norm3(p0, p1, p2);
    if (dist3D < mp.min_distance || dist3D > mp.max_distance) return false;
    if (vslam_md::dot3_mat(p0, p1, p2, mp.normal) < 0.5 * (double)dist3D) return false;
    g->uv = uv;
    g->level = vslam_md::predict_level(mp.max_distance, dist3D, log_scale_factor, nlevels);
    g->radius = th * scale_factors[g->level];
    return true;
}
} // namespace

extern "C" {

/* The host end of vslam_search_local_points_wait: the matcher ran on the compacted list, so match_compact[idx] counts kept
 * points; orig_index[k] is the k-th kept point's index in the caller's array.  More kept points than the matcher's capacity:
 * nothing can be said about any keypoint -- all -1 and VSLAM_ERR_UNSUPPORTED. */
int vslamh_local_points_finish(const int32_t* match_compact, int n_cur, const int32_t* orig_index, int n_kept, int capacity,
                               int32_t* match_cur) {
    if (n_cur < 0 || n_kept < 0 || capacity < 0 || (n_cur && (!match_compact || !match_cur)) || (n_kept && !orig_index))
        return VSLAM_ERR_INVALID;
    if (n_kept > capacity) {
        for (int i = 0; i < n_cur; i++) match_cur[i] = -1;
        return VSLAM_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < n_cur; i++) {
        const int32_t k = match_compact[i];
        match_cur[i] = (k >= 0 && k < n_kept) ? orig_index[k] : -1;
    }
    return VSLAM_OK;
}

/* mvLeftToRightMatch / mvRightToLeftMatch of a rig frame: every entry -1 or an index of the other side */
int vslamh_rig_maps_check(const int32_t* left_to_right, int n_left, const int32_t* right_to_left, int n_right) {
    if (n_left < 0 || n_right < 0 || (n_left && !left_to_right) || (n_right && !right_to_left)) return VSLAM_ERR_INVALID;
    for (int i = 0; i < n_left; i++)
        if (left_to_right[i] < -1 || left_to_right[i] >= n_right) return VSLAM_ERR_INVALID;
    for (int i = 0; i < n_right; i++)
        if (right_to_left[i] < -1 || right_to_left[i] >= n_left) return VSLAM_ERR_INVALID;
    return VSLAM_OK;
}

/* FMatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th, ...) (fmatcher.cpp:321-491) as it is written, for both
 * kinds of Frame; the sequential statement the device resolver (k_rig_resolve) is tested against, CPU tests and the demo.
 * track_right == NULL: Nleft == -1 (the right arguments are not read; u_right, may be NULL, is the frame's mvuRight).
 * Otherwise a rig: slots [0, n_left) are the left keypoints, [n_left, n_left + n_right) the right ones.  Records as
 * Frame::isInFrustum leaves them, far test and isBad folded into flag bit 0; bit 1 (of either record) = Observations() > 0.
 * scale_factors: mvScaleFactors, nlevels entries; bounds: mnMinX, mnMaxX, mnMinY, mnMaxY.  occupied (may be NULL): per slot. */
int vslamh_search_by_projection_mappoints_rig(const vslam_mp_track* track_left, const vslam_mp_track* track_right,
                                              const uint8_t* mp_desc, int n_mp, const vslam_kp* kps_left,
                                              const uint8_t* desc_left, int n_left, const vslam_kp* kps_right,
                                              const uint8_t* desc_right, int n_right, const int32_t* left_to_right,
                                              const int32_t* right_to_left, const float* u_right, const uint8_t* occupied,
                                              const float* scale_factors, int nlevels, const float* bounds, float th,
                                              float nnratio, int32_t* match_cur, int* nmatches) {
    const bool rig = track_right != nullptr;
    if (!rig) n_right = 0;
    if (n_mp < 0 || n_left < 0 || n_right < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        (n_mp && (!track_left || !mp_desc)) || (n_left && (!kps_left || !desc_left)) || (n_right && (!kps_right || !desc_right)) ||
        ((n_left + n_right) && !match_cur))
        return VSLAM_ERR_INVALID;
    if (rig)
        if (int rc = vslamh_rig_maps_check(left_to_right, n_left, right_to_left, n_right)) return rc;
    const int TH_HIGH = 100;
    const int N = n_left + n_right;
    std::vector<uint8_t> occ = clear_matches(match_cur, N, occupied);
    FrameGrid gl, gr;
    gl.build(kps_left, n_left, bounds);
    gr.build(kps_right, n_right, bounds);
    std::vector<int> vIndices;
    const bool bFactor = th != 1.0f;
    int nm = 0;
    /* mvScaleFactors[level]: a caller-made record's level is clamped into the table, as k_sbp_rank does */
    auto scale_of = [&](int l) { return scale_factors[std::min(std::max(l, 0), nlevels - 1)]; };
    for (int iMP = 0; iMP < n_mp; iMP++) {
        const vslam_mp_track& L = track_left[iMP];
        const bool inL = (L.flags & 1u) != 0, inR = rig && (track_right[iMP].flags & 1u) != 0;
        if (!inL && !inR) continue;
        const uint8_t obs = ((L.flags | (rig ? track_right[iMP].flags : 0u)) & 2u) ? 1 : 0;
        const uint8_t* d = mp_desc + (size_t)iMP * 32;
        if (inL) {
            float r = (double)L.view_cos > 0.998 ? 2.5f : 4.0f;
            if (bFactor) r *= th;
            const float rs = r * scale_of(L.level);
            gl.query(L.proj_x, L.proj_y, rs, L.level - 1, L.level, vIndices);
            if (!vIndices.empty()) {
                RigBest b;
                for (int idx : vIndices) {
                    if (occ[idx]) continue;
                    if (!rig && u_right && u_right[idx] > 0) {
                        const float er = fabsf(L.proj_xr - u_right[idx]);
                        if (er > rs) continue;
                    }
                    b.take(rig_hamming(d, desc_left + (size_t)idx * 32), kps_left[idx].octave, idx);
                }
                if (b.bestDist <= TH_HIGH) {
                    if (b.bestLevel == b.bestLevel2 && (float)b.bestDist > nnratio * (float)b.bestDist2) continue;
                    match_cur[b.bestIdx] = iMP;
                    occ[b.bestIdx] = obs;
                    if (rig && left_to_right[b.bestIdx] != -1) {
                        const int s = left_to_right[b.bestIdx] + n_left;
                        match_cur[s] = iMP;
                        occ[s] = obs;
                        nm++;
                    }
                    nm++;
                }
            }
        }
        if (inR) {
            const vslam_mp_track& R = track_right[iMP];
            if (R.level == -1) continue;
            const float r = (double)R.view_cos > 0.998 ? 2.5f : 4.0f; /* no bFactor here (fmatcher.cpp:425) */
            gr.query(R.proj_x, R.proj_y, r * scale_of(R.level), R.level - 1, R.level, vIndices);
            if (vIndices.empty()) continue;
            RigBest b;
            for (int idx : vIndices) {
                if (occ[idx + n_left]) continue;
                b.take(rig_hamming(d, desc_right + (size_t)idx * 32), kps_right[idx].octave, idx);
            }
            if (b.bestDist <= TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && (float)b.bestDist > nnratio * (float)b.bestDist2) continue;
                if (right_to_left[b.bestIdx] != -1) {
                    match_cur[right_to_left[b.bestIdx]] = iMP;
                    occ[right_to_left[b.bestIdx]] = obs;
                    nm++;
                }
                match_cur[b.bestIdx + n_left] = iMP;
                occ[b.bestIdx + n_left] = obs;
                nm++;
            }
        }
    }
    *nmatches = nm;
    return VSLAM_OK;
}

/* vslam_search_by_projection_frame_rig: fx, fy, cx, cy of the projection parameters equal the KB8 camera's bit for bit */
int vslamh_frame_rig_camera_check(const vslam_proj_params* p, const vslam_kb8_camera* cam) {
    if (!p || !cam) return VSLAM_ERR_INVALID;
    return (vslam_kb8::same_bits(p->fx, cam->fx) && vslam_kb8::same_bits(p->fy, cam->fy) && vslam_kb8::same_bits(p->cx, cam->cx) &&
            vslam_kb8::same_bits(p->cy, cam->cy))
               ? VSLAM_OK
               : VSLAM_ERR_INVALID;
}

/* FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) for a two-fisheye rig
 * (fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1) as it is written, sequential: the statement the device form
 * (vslam_search_by_projection_frame_rig) is tested against, and the shim's fallback.  Same arguments with host keypoints;
 * cam = CurrentFrame.mpCamera, through which BOTH branches project; Trl = rows [R | t] of mTrl; scale_factors: mvScaleFactors,
 * nlevels entries; bounds: mnMinX, mnMaxX, mnMinY, mnMaxY; occupied (may be NULL): per slot of n_left + n_right. */
int vslamh_search_by_projection_frame_rig(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Trl,
                                          const vslam_kp* last_kps, int n_last, const uint8_t* last_flags, const float* last_x3dw,
                                          const uint8_t* mp_desc, const vslam_kp* kps_left, const uint8_t* desc_left, int n_left,
                                          const vslam_kp* kps_right, const uint8_t* desc_right, int n_right,
                                          const uint8_t* occupied, const float* scale_factors, int nlevels, const float* bounds,
                                          int32_t* match_cur, int* nmatches) {
    if (!p || !cam || !Trl || n_last < 0 || n_left < 0 || n_right < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        (n_last && (!last_kps || !last_flags || !last_x3dw || !mp_desc)) || (n_left && (!kps_left || !desc_left)) ||
        (n_right && (!kps_right || !desc_right)) || ((n_left + n_right) && !match_cur))
        return VSLAM_ERR_INVALID;
    if (vslamh_frame_rig_camera_check(p, cam)) return VSLAM_ERR_INVALID;
    const int TH_HIGH = 100, L = VSLAM_HISTO_LENGTH;
    const int N = n_left + n_right;
    std::vector<uint8_t> occ = clear_matches(match_cur, N, occupied);
    FrameGrid gl, gr;
    gl.build(kps_left, n_left, bounds);
    gr.build(kps_right, n_right, bounds);
    std::vector<int> vIndices2;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    for (int i = 0; i < n_last; i++) {
        if (!(last_flags[i] & 1)) continue; /* pMP && !LastFrame.mvbOutlier[i] */
        const uint8_t obs = (last_flags[i] & 2) ? 1 : 0;
        float x3Dc[3];
        rig_transform(p->Tcw, last_x3dw + 3 * i, p->gemm_float, x3Dc);
        const float invzc = (float)(1.0 / (double)x3Dc[2]);
        if (invzc < 0) continue;
        const vslam_kb8::Uv uv = vslam_kb8::kb8_project(*cam, x3Dc[0], x3Dc[1], x3Dc[2]);
        if (uv.u < bounds[0] || uv.u > bounds[1]) continue;
        if (uv.v < bounds[2] || uv.v > bounds[3]) continue;
        const int nLastOctave = last_kps[i].octave; /* keypoints_[i] | keypointsRight_[i - Nleft]: the caller's one array */
        const float radius = p->th * scale_factors[std::min(std::max(nLastOctave, 0), nlevels - 1)];
        const int minLevel = p->forward ? nLastOctave : p->backward ? 0 : nLastOctave - 1;
        const int maxLevel = p->forward ? -1 : p->backward ? nLastOctave : nLastOctave + 1;
        gl.query(uv.u, uv.v, radius, minLevel, maxLevel, vIndices2);
        if (vIndices2.empty()) continue;
        const uint8_t* dMP = mp_desc + (size_t)i * 32;
        {
            int bestDist = 256;
            const int bestIdx2 = best_candidate(vIndices2, dMP, desc_left, &bestDist, [&](int i2) { return occ[i2] != 0; });
            if (bestDist <= TH_HIGH) {
                match_cur[bestIdx2] = i;
                occ[bestIdx2] = obs;
                nm++;
                if (p->check_orientation)
                    rotHist[vslam_md::rot_bin(last_kps[i].angle, kps_left[bestIdx2].angle, L)].push_back(bestIdx2);
            }
        }
        { /* :2593-2658: no depth test, no in-frame test, no empty-window `continue`; the LEFT camera's model */
            float x3Dr[3];
            rig_transform(Trl, x3Dc, p->gemm_float, x3Dr);
            const vslam_kb8::Uv uvr = vslam_kb8::kb8_project(*cam, x3Dr[0], x3Dr[1], x3Dr[2]);
            gr.query(uvr.u, uvr.v, radius, minLevel, maxLevel, vIndices2);
            int bestDist = 256;
            const int bestIdx2 =
                best_candidate(vIndices2, dMP, desc_right, &bestDist, [&](int i2) { return occ[i2 + n_left] != 0; });
            if (bestDist <= TH_HIGH) {
                match_cur[bestIdx2 + n_left] = i;
                occ[bestIdx2 + n_left] = obs;
                nm++;
                if (p->check_orientation)
                    rotHist[vslam_md::rot_bin(last_kps[i].angle, kps_right[bestIdx2].angle, L)].push_back(bestIdx2 + n_left);
            }
        }
    }
    if (p->check_orientation)
        for (int s : vslam::rotation_losers(rotHist)) {
            match_cur[s] = -1;
            nm--;
        }
    *nmatches = nm;
    return VSLAM_OK;
}

/* The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame / a two-fisheye rig
 * (fmatcher.cpp:1918-2119; the Scw overload :2121-2243 as sim3 = 1) as it is written, job after job and point after point:
 * the statement the device form (vslam_fuse_search_rig) is tested against, and what the shim's walk calls with ONE point to
 * redo a search whose MapPoint descriptor was recomputed.  Same arguments; every pointer a HOST pointer, a job's dev_kps /
 * dev_desc included; any number of jobs and points.  cam = mpCamera, rig (may be NULL when no job has camera 1) gives
 * mpCamera2; scale_factors / inv_sigma2: mvScaleFactors / mvInvLevelSigma2, nlevels entries; bounds: the Frame's float mnMinX,
 * mnMaxX, mnMinY, mnMaxY, which the KeyFrame truncates for its window origin and IsInImage.  best_idx / best_dist: n_jobs *
 * n_points entries each, job-major. */
int vslamh_fuse_search_rig(const vslam_fuse_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                           const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points, const uint8_t* mp_desc,
                           int n_points, const float* scale_factors, const float* inv_sigma2, int nlevels, const float* bounds,
                           int32_t* best_idx, int32_t* best_dist) {
    if (!p || !vslam_kb8::camera_ok(cam) || !jobs || n_jobs < 1 || n_points < 0 || nlevels < 1 || !scale_factors || !inv_sigma2 ||
        !bounds || (n_points && (!points || !mp_desc || !best_idx || !best_dist)))
        return VSLAM_ERR_INVALID;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        if (s.camera < 0 || s.camera > 1 || s.sim3 < 0 || s.sim3 > 1 || (s.sim3 && s.camera) || s.n_kf < 0 ||
            (s.n_kf && (!s.dev_kps || !s.dev_desc)) || (s.camera == 1 && (!rig || !vslam_kb8::camera_ok(&rig->cam2))))
            return VSLAM_ERR_INVALID;
    }
    const KfBounds kb(bounds);
    std::vector<int> vIndices;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_fuse_rig_job& s = jobs[j];
        const vslam_kb8_camera& c = s.camera ? rig->cam2 : *cam;
        FrameGrid grid;
        grid.build_keyframe(s.dev_kps, s.n_kf, bounds);
        int32_t* bi = best_idx + (size_t)j * n_points;
        int32_t* bd = best_dist + (size_t)j * n_points;
        for (int i = 0; i < n_points; i++) {
            bi[i] = -1;
            bd[i] = 256;
            const vslam_fuse_point& mp = points[i];
            if (!mp.valid || (s.valid_host && !s.valid_host[i])) continue;
            KfWindow w;
            if (!keyframe_gate(s, c, kb, mp, p->gemm_float, p->log_scale_factor, p->th, scale_factors, nlevels, &w)) continue;
            grid.query(w.uv.u, w.uv.v, w.radius, -1, -1, vIndices);
            int bestDist = s.sim3 ? INT_MAX : 256; /* :2203 against :2039 */
            const int bestIdx = best_candidate(vIndices, mp_desc + (size_t)i * 32, s.dev_desc, &bestDist, [&](int idx) {
                const int kpLevel = s.dev_kps[idx].octave;
                if (kpLevel < w.level - 1 || kpLevel > w.level) return true;
                if (s.sim3) return false; /* the Scw overload has no chi-square test (:2205-2222) */
                /* mvuRight is -1 throughout: the monocular branch */
                const float ex = w.uv.u - s.dev_kps[idx].x, ey = w.uv.v - s.dev_kps[idx].y;
                const float e2 = ex * ex + ey * ey;
                return (double)(e2 * inv_sigma2[std::min(kpLevel, nlevels - 1)]) > 5.99;
            });
            if (bestIdx >= 0) {
                bi[i] = bestIdx + s.idx_offset;
                bd[i] = bestDist;
            }
        }
    }
    return VSLAM_OK;
}

/* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (fmatcher.cpp:2689-2811) with a
 * fisheye CurrentFrame as it is written, sequential: the statement vslam_search_by_projection_keyframe_kb8 is tested against.
 * Same arguments with host keypoints; cam = CurrentFrame.mpCamera; cur_kps / cur_desc: keypoints_ and the descriptor rows
 * [0, n_cur), of a rig the LEFT camera's (bRight defaults to false); kf_kps: mvKeys followed by mvKeysRight -- the reference
 * reads pKF->mvKeysUn[i].angle past the end for i >= NLeft, the restatement the right keypoint's angle. */
int vslamh_search_by_projection_keyframe_kb8(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Ow,
                                             float log_scale_factor, int orb_dist, const vslam_kp* kf_kps, int n_kf,
                                             const uint8_t* mp_flags, const float* mp_x3dw, const float* mp_min_dist,
                                             const float* mp_max_dist, const uint8_t* mp_desc, const vslam_kp* cur_kps,
                                             const uint8_t* cur_desc, int n_cur, const uint8_t* cur_occupied,
                                             const float* scale_factors, int nlevels, const float* bounds, int32_t* match_cur,
                                             int* nmatches) {
    if (!p || !vslam_kb8::camera_ok(cam) || !Ow || n_kf < 0 || n_cur < 0 || nlevels < 1 || !scale_factors || !bounds || !nmatches ||
        orb_dist < 1 || orb_dist > 255 ||
        (n_kf && (!kf_kps || !mp_flags || !mp_x3dw || !mp_min_dist || !mp_max_dist || !mp_desc)) ||
        (n_cur && (!cur_kps || !cur_desc || !match_cur)))
        return VSLAM_ERR_INVALID;
    if (vslamh_frame_rig_camera_check(p, cam)) return VSLAM_ERR_INVALID;
    const int L = VSLAM_HISTO_LENGTH;
    std::vector<uint8_t> occ = clear_matches(match_cur, n_cur, cur_occupied);
    FrameGrid grid;
    grid.build(cur_kps, n_cur, bounds);
    std::vector<int> vIndices2;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    for (int i = 0; i < n_kf; i++) {
        if (!(mp_flags[i] & 1)) continue; /* pMP && !pMP->isBad() && !sAlreadyFound.count(pMP) */
        const float* x3Dw = mp_x3dw + 3 * i;
        float x3Dc[3];
        rig_transform(p->Tcw, x3Dw, p->gemm_float, x3Dc);
        const vslam_kb8::Uv uv = vslam_kb8::kb8_project(*cam, x3Dc[0], x3Dc[1], x3Dc[2]); /* no depth test */
        if (uv.u < bounds[0] || uv.u > bounds[1]) continue;
        if (uv.v < bounds[2] || uv.v > bounds[3]) continue;
        const float dist3D = vslam_md::norm3(x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]);
        if (dist3D < mp_min_dist[i] || dist3D > mp_max_dist[i]) continue;
        const int level = vslam_md::predict_level(mp_max_dist[i], dist3D, log_scale_factor, nlevels);
        const float radius = p->th * scale_factors[level];
        grid.query(uv.u, uv.v, radius, level - 1, level + 1, vIndices2);
        if (vIndices2.empty()) continue;
        const uint8_t* dMP = mp_desc + (size_t)i * 32;
        int bestDist = 256;
        const int bestIdx2 = best_candidate(vIndices2, dMP, cur_desc, &bestDist, [&](int i2) { return occ[i2] != 0; });
        if (bestDist <= orb_dist) {
            match_cur[bestIdx2] = i;
            occ[bestIdx2] = 1;
            nm++;
            if (p->check_orientation) rotHist[vslam_md::rot_bin(kf_kps[i].angle, cur_kps[bestIdx2].angle, L)].push_back(bestIdx2);
        }
    }
    if (p->check_orientation)
        for (int s : vslam::rotation_losers(rotHist)) {
            match_cur[s] = -1;
            nm--;
        }
    *nmatches = nm;
    return VSLAM_OK;
}

/* FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863) for fisheye KeyFrames as
 * it is written, job after job and point after point: the statement vslam_search_by_projection_sim3_kb8 is tested against, and
 * what the shim runs for a job the device refused.  Same arguments; every pointer a HOST pointer, a job's dev_kps / dev_desc
 * included; any number of jobs, points and survivors.  n_gated[j] (may be NULL): the points that pass every gate up to the
 * radius.  bounds: the Frame's float mnMinX, mnMaxX, mnMinY, mnMaxY, truncated for the KeyFrame. */
int vslamh_search_by_projection_sim3_kb8(const vslam_sim3_kb8_params* p, const vslam_kb8_camera* cam,
                                         const vslam_sim3_kb8_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                         const uint8_t* mp_desc, int n_points, const float* scale_factors, int nlevels,
                                         const float* bounds, int32_t* const* match_kf, int* nmatches, int* n_gated) {
    if (!p || !vslam_kb8::camera_ok(cam) || !jobs || n_jobs < 1 || n_points < 0 || nlevels < 1 || !scale_factors || !bounds ||
        !match_kf || !nmatches || (n_points && (!points || !mp_desc)) || p->th < 0 || !(p->ratio_hamming >= 0.0f))
        return VSLAM_ERR_INVALID;
    for (int j = 0; j < n_jobs; j++)
        if (jobs[j].n_kf < 0 || (jobs[j].n_kf && (!jobs[j].dev_kps || !jobs[j].dev_desc || !match_kf[j]))) return VSLAM_ERR_INVALID;
    const KfBounds kb(bounds);
    const float lim = 50 * p->ratio_hamming; /* bestDist <= TH_LOW * ratioHamming with an integer bestDist */
    const int thr = lim >= 255.0f ? 255 : std::max(0, (int)floorf(lim));
    const float th = (float)p->th;
    std::vector<int> vIndices;
    for (int j = 0; j < n_jobs; j++) {
        const vslam_sim3_kb8_job& s = jobs[j];
        FrameGrid grid;
        grid.build_keyframe(s.dev_kps, s.n_kf, bounds);
        std::vector<uint8_t> matched = clear_matches(match_kf[j], s.n_kf, s.kf_matched_host);
        int nm = 0, gated = 0;
        for (int iMP = 0; iMP < n_points; iMP++) {
            const vslam_fuse_point& mp = points[iMP];
            if (!mp.valid || (s.valid_host && !s.valid_host[iMP])) continue;
            KfWindow w;
            if (!keyframe_gate(s, *cam, kb, mp, p->gemm_float, p->log_scale_factor, th, scale_factors, nlevels, &w)) continue;
            gated++;
            grid.query(w.uv.u, w.uv.v, w.radius, -1, -1, vIndices);
            if (vIndices.empty()) continue;
            int bestDist = 256;
            const int bestIdx = best_candidate(vIndices, mp_desc + (size_t)iMP * 32, s.dev_desc, &bestDist, [&](int idx) {
                const int kpLevel = s.dev_kps[idx].octave;
                return matched[idx] || kpLevel < w.level - 1 || kpLevel > w.level;
            });
            if (bestDist <= thr) {
                match_kf[j][bestIdx] = iMP;
                matched[bestIdx] = 1;
                nm++;
            }
        }
        nmatches[j] = nm;
        if (n_gated) n_gated[j] = gated;
    }
    return VSLAM_OK;
}

/* FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (fmatcher.cpp:546-748) with F.Nleft != -1 as it is
 * written, sequential, for one keyframe: the statement vslam_search_by_bow_rig is tested against, and the shim's fallback
 * beyond the device limits (there are none here).  Descriptor rows and FeatureVector indices of either side run over
 * [0, n_left + n_right), left first; kf_kps is ONE array (mvKeys then mvKeysRight), the frame's keypoints come per camera.
 * The right branch is nested in `bestDist1 <= TH_LOW` and its ratio test is `|| true`; one histogram takes both sides. */
int vslamh_search_by_bow_rig(const vslam_kp* kf_kps, const uint8_t* kf_desc_left, int kf_n_left, const uint8_t* kf_desc_right,
                             int kf_n_right, const uint8_t* kf_flags, const int32_t* kf_fv_nodes, const int32_t* kf_fv_off,
                             const int32_t* kf_fv_feat, int n_kf_nodes, const vslam_kp* f_kps_left, const uint8_t* f_desc_left,
                             int n_left, const vslam_kp* f_kps_right, const uint8_t* f_desc_right, int n_right,
                             const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat, int n_f_nodes,
                             float nnratio, int check_orientation, int32_t* match_f, int* nmatches) {
    const int nKF = kf_n_left + kf_n_right, N = n_left + n_right;
    if (kf_n_left < 0 || kf_n_right < 0 || n_left < 0 || n_right < 0 || n_kf_nodes < 0 || n_f_nodes < 0 || !nmatches ||
        (nKF && (!kf_kps || !kf_flags)) || (kf_n_left && !kf_desc_left) || (kf_n_right && !kf_desc_right) ||
        (n_left && (!f_kps_left || !f_desc_left)) || (n_right && (!f_kps_right || !f_desc_right)) || (N && !match_f) ||
        (n_kf_nodes && (!kf_fv_nodes || !kf_fv_off || !kf_fv_feat)) || (n_f_nodes && (!f_fv_nodes || !f_fv_off || !f_fv_feat)))
        return VSLAM_ERR_INVALID;
    *nmatches = 0;
    for (int i = 0; i < N; i++) match_f[i] = -1;
    for (int side = 0; side < 2; side++) {
        const int32_t *off = side ? f_fv_off : kf_fv_off, *feat = side ? f_fv_feat : kf_fv_feat;
        const int nn = side ? n_f_nodes : n_kf_nodes, n = side ? N : nKF;
        if (nn && off[0] != 0) return VSLAM_ERR_INVALID;
        for (int j = 0; j < nn; j++) {
            if (off[j + 1] < off[j]) return VSLAM_ERR_INVALID;
            for (int a = off[j]; a < off[j + 1]; a++)
                if (feat[a] < 0 || feat[a] >= n) return VSLAM_ERR_INVALID;
        }
    }
    const int TH_LOW = 50, L = VSLAM_HISTO_LENGTH;
    std::vector<int> rotHist[VSLAM_HISTO_LENGTH];
    int nm = 0;
    int KFit = 0, Fit = 0;
    while (KFit != n_kf_nodes && Fit != n_f_nodes) {
        if (kf_fv_nodes[KFit] == f_fv_nodes[Fit]) {
            for (int a = kf_fv_off[KFit]; a < kf_fv_off[KFit + 1]; a++) {
                const int realIdxKF = kf_fv_feat[a];
                if (!kf_flags[realIdxKF]) continue; /* !pMP || pMP->isBad() */
                const uint8_t* dKF = realIdxKF < kf_n_left ? kf_desc_left + (size_t)realIdxKF * 32
                                                           : kf_desc_right + (size_t)(realIdxKF - kf_n_left) * 32;
                int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
                int bestDist1R = 256, bestIdxFR = -1;
                for (int b = f_fv_off[Fit]; b < f_fv_off[Fit + 1]; b++) {
                    const int realIdxF = f_fv_feat[b];
                    if (match_f[realIdxF] >= 0) continue;
                    const uint8_t* dF = realIdxF < n_left ? f_desc_left + (size_t)realIdxF * 32
                                                          : f_desc_right + (size_t)(realIdxF - n_left) * 32;
                    const int dist = rig_hamming(dKF, dF);
                    if (realIdxF < n_left && dist < bestDist1) {
                        bestDist2 = bestDist1;
                        bestDist1 = dist;
                        bestIdxF = realIdxF;
                    } else if (realIdxF < n_left && dist < bestDist2) {
                        bestDist2 = dist;
                    }
                    if (realIdxF >= n_left && dist < bestDist1R) {
                        bestDist1R = dist;
                        bestIdxFR = realIdxF;
                    }
                }
                if (bestDist1 <= TH_LOW) {
                    const float angKF = kf_kps[realIdxKF].angle;
                    if ((float)bestDist1 < nnratio * (float)bestDist2) {
                        match_f[bestIdxF] = realIdxKF;
                        if (check_orientation) rotHist[vslam_md::rot_bin(angKF, f_kps_left[bestIdxF].angle, L)].push_back(bestIdxF);
                        nm++;
                    }
                    if (bestDist1R <= TH_LOW) { /* `|| true`, :682 */
                        match_f[bestIdxFR] = realIdxKF;
                        if (check_orientation)
                            rotHist[vslam_md::rot_bin(angKF, f_kps_right[bestIdxFR - n_left].angle, L)].push_back(bestIdxFR);
                        nm++;
                    }
                }
            }
            KFit++;
            Fit++;
        } else if (kf_fv_nodes[KFit] < f_fv_nodes[Fit]) {
            KFit = (int)(std::lower_bound(kf_fv_nodes, kf_fv_nodes + n_kf_nodes, f_fv_nodes[Fit]) - kf_fv_nodes);
        } else {
            Fit = (int)(std::lower_bound(f_fv_nodes, f_fv_nodes + n_f_nodes, kf_fv_nodes[KFit]) - f_fv_nodes);
        }
    }
    if (check_orientation)
        for (int s : vslam::rotation_losers(rotHist)) {
            match_f[s] = -1;
            nm--;
        }
    *nmatches = nm;
    return VSLAM_OK;
}

/* vslam_two_view_score on the host, every pointer of the job a HOST pointer (the placement fields are not read): the pair
 * list, CheckHomography / CheckFundamental for every hypothesis by the shared vslam_two_view.h code, the selection.  Same
 * limits, error codes and results as the device entry (include/vslam_fe.h).  CPU tests and the stand-alone demo; the
 * product runs k_tv_pairs / k_tv_score / k_tv_select. */
int vslamh_two_view_score(const vslam_two_view_job* job, vslam_two_view_result* result) {
    if (!job || !result) return VSLAM_ERR_INVALID;
    const vslam_two_view_job& q = *job;
    if (q.n1 < 0 || q.n1 > 65536 || q.n2 < 0 || q.nH < 0 || q.nH > VSLAM_TWO_VIEW_MAX_HYP || q.nF < 0 ||
        q.nF > VSLAM_TWO_VIEW_MAX_HYP || (q.n1 && (!q.kps1 || !q.matches12)) || (q.n1 && q.n2 && !q.kps2) ||
        (q.nH && (!q.H21 || !q.H12)) || (q.nF && !q.F21) || !std::isfinite(q.sigma) || q.sigma == 0.0f)
        return VSLAM_ERR_INVALID;
    vslam_two_view_result& R = *result;
    const int cap = std::min(q.n1, VSLAM_TWO_VIEW_MAX_PAIRS);
    std::vector<float> pts;
    std::vector<int32_t> pairs;
    int n = 0;
    bool err = false;
    for (int i = 0; i < q.n1; i++) { /* motion_estimation.cpp:2020-2029 */
        const int32_t m = q.matches12[i];
        if (m >= q.n2) err = true;
        if (m < 0 || m >= q.n2) continue;
        if (n < cap) {
            pairs.insert(pairs.end(), {i, m});
            pts.insert(pts.end(), {q.kps1[i].x, q.kps1[i].y, q.kps2[m].x, q.kps2[m].y});
        }
        n++;
    }
    const int used = (err || n > cap) ? 0 : n;
    const float inv = vslam_tv::inv_sigma_square(q.sigma);
    R.n_pairs = n;
    if (R.pairs && !pairs.empty()) memcpy(R.pairs, pairs.data(), pairs.size() * 4);
    std::vector<uint8_t> cur((size_t)used);
    for (int model = 0; model < 2; model++) {
        const int nhyp = model ? q.nF : q.nH;
        float* scores = model ? R.scores_f : R.scores_h;
        uint8_t* mask = model ? R.inliers_f : R.inliers_h;
        vslam_tv::Best best = vslam_tv::best_none();
        if (mask && used) memset(mask, 0, (size_t)used);
        for (int it = 0; it < nhyp; it++) {
            const vslam_tv::Mat3 A = vslam_tv::load_mat3((model ? q.F21 : q.H21) + (size_t)it * 9);
            const vslam_tv::Mat3 B = model ? A : vslam_tv::load_mat3(q.H12 + (size_t)it * 9);
            float score = 0.0f;
            for (int p = 0; p < used; p++) {
                const float* x = &pts[4 * (size_t)p];
                const vslam_tv::Terms t = model ? vslam_tv::check_f(A, x[0], x[1], x[2], x[3], inv)
                                                : vslam_tv::check_h(A, B, x[0], x[1], x[2], x[3], inv);
                score = vslam_tv::fadd(score, t.t1);
                score = vslam_tv::fadd(score, t.t2);
                cur[p] = t.in ? 1 : 0;
            }
            score = vslam_tv::report_score(score);
            if (scores) scores[it] = score;
            const vslam_tv::Best was = best;
            best = vslam_tv::best_take(best, score, it);
            if (best.index != was.index && mask && used) memcpy(mask, cur.data(), (size_t)used);
        }
        (model ? R.best_f : R.best_h) = best.index;
        (model ? R.score_f : R.score_h) = best.index >= 0 ? best.score : 0.0f;
    }
    return err ? VSLAM_ERR_INVALID : n > cap ? VSLAM_ERR_UNSUPPORTED : VSLAM_OK;
}

} /* extern "C" */
