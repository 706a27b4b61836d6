/* vslam_frustum.h -- Frame::isInFrustum (frame.cpp:529-595, the pinhole branch Nleft == -1) and MapPoint::PredictScale
 * (mappoint.cpp:523-538) for one MapPoint, written once for the device (k_frustum, vslam_frustum.hip) and the host
 * (vslamh_in_frustum in vslam_camera_host.cpp: CPU tests and the stand-alone demo, not a fallback of the product).
 * The same test with the fisheye projection (mpCamera = KannalaBrandt8) and the two-camera branch Nleft != -1
 * (isInFrustumChecks) are in vslam_kb8.h, built from the pieces of this header.
 *
 * What the reference evaluates, in its order:
 *   Pc = mRcwx * Px + mtcwx        cv::Matx algebra: Matx never goes through cv::gemm.  MatxMultiply (OpenCV 4.2
 *                                  modules/core/include/opencv2/core/matx.hpp, Matx(const Matx&, const Matx&, Matx_MatMulOp):
 *                                  `_Tp s = 0; for k: s += a(i,k) * b(k,j)`) accumulates in FLOAT from zero, then the
 *                                  Matx addition adds t: (((0 + r0*X) + r1*Y) + r2*Z) + t
 *   Pc_dist = cv::norm(Pc)         norm(const Matx&) = std::sqrt(normL2Sqr<float, double>(val, 3)): squares accumulated in
 *                                  DOUBLE in index order, double sqrt, rounded to float on assignment
 *   invz = 1.0f / PcZ              before the depth test; the test is PcZ < 0.0f, so PcZ == +0 passes it
 *   uv = Pinhole::project(Pc)      (fx*x)/z + cx (pinhole.cpp:13-16); does not use invz
 *   uv.x < mnMinX || uv.x > mnMaxX closed interval over the Frame's float grid bounds; mTrackProjX / Y are written as soon as
 *                                  it passes (:557-558), whatever the later tests say
 *   dist = cv::norm(Px - mOwx)     as above
 *   dist < min || dist > max
 *   viewCos = PO.dot(Pn) / dist    Matx::dot (matx.hpp, `_Tp s = 0; for i: s += val[i] * M.val[i]`): FLOAT accumulation from
 *                                  zero -- unlike cv::Mat::dot, which the Sim3 form (k_sbp_rank mode 3) accumulates in double
 *   PredictScale(dist, Frame*)     vslam_md::predict_level (vslam_matchdev.h), as in k_sbp_rank modes 2 and 3
 *   mTrackProjXR = uv.x - mbf * invz,  mTrackDepth = Pc_dist
 * The matx.hpp loops are quoted as recalled from OpenCV 4.2, not pinned against a build of it (oracle section).
 *
 * Deviations and limits, documented in include/vslam_fe.h:
 *   - a point that is not in view gets flags bit 0 clear, proj_x / proj_y = -1 or uv (what the reference leaves) and ZERO in
 *     every other field and in its depth; the reference leaves whatever an earlier frame wrote there
 *   - 0/0 projections (PcZ == 0 with x == 0 or y == 0) are NaN, pass the reference's bounds test and reach a float-to-int
 *     cast there, which is undefined; not modelled
 *   - `max` of PredictScale is the record's max_dist, as in every other matcher of this library (vslam_fuse_point, the
 *     KeyFrame and Sim3 forms)
 *
 * Contraction: on the device every operation goes through the _rn intrinsics; host builds rely on -ffp-contract=off
 * (vi_slam_amd/csrc/Makefile).
 */
#ifndef VSLAM_FRUSTUM_H
#define VSLAM_FRUSTUM_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>

#include "../../include/vslam_fe.h"
#include "vslam_matchdev.h"

namespace vslam_fr {

using namespace vslam_md; /* fmul .. fdvd, norm3, dot3_matx, predict_level */

/* what one call of Frame::isInFrustum reads of the Frame */
struct Frame {
    float Tcw[12]; /* rows [mRcwx | mtcwx] */
    float Ow[3];
    float fx, fy, cx, cy, mbf;
    float viewingCosLimit, logScaleFactor;
    float minX, maxX, minY, maxY; /* mnMinX .. */
    int32_t nlevels;
};

/* the Frame of a call: its parameters, the grid bounds in force (minX, maxX, minY, maxY) and the extractor's level count */
static inline Frame make_frame(const vslam_frustum_params& p, const float* bounds, int nlevels) {
    Frame F;
    for (int i = 0; i < 12; i++) F.Tcw[i] = p.Tcw[i];
    for (int i = 0; i < 3; i++) F.Ow[i] = p.Ow[i];
    F.fx = p.fx;
    F.fy = p.fy;
    F.cx = p.cx;
    F.cy = p.cy;
    F.mbf = p.mbf;
    F.viewingCosLimit = p.viewing_cos_limit;
    F.logScaleFactor = p.log_scale_factor;
    F.minX = bounds[0];
    F.maxX = bounds[1];
    F.minY = bounds[2];
    F.maxY = bounds[3];
    F.nlevels = nlevels;
    return F;
}

/* The record Frame::isInFrustum leaves in one MapPoint and its mTrackDepth.  mp.flags bit 0 is the caller's
 * "mnLastFrameSeen != frame id && !isBad()" (Tracking::SearchLocalPoints, tracking.cpp:3221-3224: the function is not
 * called otherwise); out->flags bit 0 = mbTrackInView, bit 1 = mp.flags bit 1 (Observations() > 0). */
VSLAM_HD void in_frustum(const Frame& F, const vslam_map_point& mp, vslam_mp_track* out, float* depth) {
    vslam_mp_track t;
    t.proj_x = -1.0f;
    t.proj_y = -1.0f;
    t.proj_xr = 0.0f;
    t.view_cos = 0.0f;
    t.level = 0;
    t.flags = mp.flags & 2u;
    *depth = 0.0f;
    *out = t;
    if (!(mp.flags & 1u)) return;
    const float X = mp.pos[0], Y = mp.pos[1], Z = mp.pos[2];
    const float PcX = fadd(dot3_matx(F.Tcw + 0, X, Y, Z), F.Tcw[3]);
    const float PcY = fadd(dot3_matx(F.Tcw + 4, X, Y, Z), F.Tcw[7]);
    const float PcZ = fadd(dot3_matx(F.Tcw + 8, X, Y, Z), F.Tcw[11]);
    const float Pc_dist = norm3(PcX, PcY, PcZ);
    const float invz = fdvd(1.0f, PcZ);
    if (PcZ < 0.0f) return;
    const float u = fadd(fdvd(fmul(F.fx, PcX), PcZ), F.cx);
    const float v = fadd(fdvd(fmul(F.fy, PcY), PcZ), F.cy);
    if (u < F.minX || u > F.maxX) return;
    if (v < F.minY || v > F.maxY) return;
    t.proj_x = u;
    t.proj_y = v;
    *out = t;
    const float PO[3] = {fsub(X, F.Ow[0]), fsub(Y, F.Ow[1]), fsub(Z, F.Ow[2])};
    const float dist = norm3(PO[0], PO[1], PO[2]);
    if (dist < mp.min_dist || dist > mp.max_dist) return;
    const float viewCos = fdvd(dot3_matx(PO, mp.normal[0], mp.normal[1], mp.normal[2]), dist);
    if (viewCos < F.viewingCosLimit) return;
    const int level = predict_level(mp.max_dist, dist, F.logScaleFactor, F.nlevels);
    t.proj_xr = fsub(u, fmul(F.mbf, invz));
    t.view_cos = viewCos;
    t.level = level;
    t.flags |= 1u;
    *depth = Pc_dist;
    *out = t;
}

} // namespace vslam_fr

/* The two launches of the frustum stage (vslam_frustum.hip); by-value kernel arguments, every pointer a DEVICE pointer.
 * One workgroup covers VSLAM_FRUSTUM_CHUNK points; VSLAM_FRUSTUM_MAX_POINTS / VSLAM_FRUSTUM_CHUNK = 256 chunk counts is what
 * one workgroup of k_frustum_compact sums with one load per lane. */
#define VSLAM_FRUSTUM_CHUNK 256
#define VSLAM_FRUSTUM_MAX_POINTS 65536
#define VSLAM_FRUSTUM_MAX_KEPT 4096 /* capacity of the matcher behind it (k_sbpm_resolve) */
struct FrustumArgsDev {
    vslam_fr::Frame F;
    int32_t n, farPoints;
    float thFarPoints;
    const vslam_map_point* pts; /* n */
    vslam_mp_track* track;      /* out: n records */
    float* depth;               /* out: n x mTrackDepth */
    int32_t* chunkKeep;         /* out: per chunk, points that go on to the matcher */
    int32_t* chunkInView;       /* out: per chunk, points with mbTrackInView (nToMatch) */
};
struct FrustumCompactDev {
    int32_t n, nchunks, farPoints, cap; /* cap: slots of the compacted arrays, <= VSLAM_FRUSTUM_MAX_KEPT */
    float thFarPoints;
    const vslam_mp_track* track;
    const float* depth;
    const uint8_t* desc; /* n x 32, 16-byte aligned */
    const int32_t* chunkKeep;
    const int32_t* chunkInView;
    vslam_mp_track* trackC; /* out, cap slots each: records, descriptors, matcher flags, original indices */
    uint8_t* descC;
    uint8_t* flagsC;
    int32_t* indexC;
    int32_t* counts; /* out: [0] kept, [1] min(kept, cap), [2] nToMatch */
};
/* the rig's compaction (k_rig_keep, k_rig_compact): two record arrays in, two compacted ones out; chunkKeep is its own scratch */
struct FrustumRigCompactDev {
    int32_t n, nchunks, farPoints, cap;
    float thFarPoints;
    const vslam_mp_track *trackL, *trackR;
    const float* depthL; /* mTrackDepth: the far test reads the left depth for every point */
    const uint8_t* desc;
    int32_t* chunkKeep;          /* scratch: nchunks */
    const int32_t* chunkInView;  /* per chunk, left || right (k_frustum_rig) */
    vslam_mp_track *trackLC, *trackRC;
    uint8_t* descC;
    uint8_t* flagsC;
    int32_t* indexC;
    int32_t* counts; /* out: [0] kept, [1] min(kept, cap), [2] nToMatch */
};
#endif
