/* vslam_camera_host.cpp -- see vslam_host.h: the camera models on the host (undistortion, image bounds, isInFrustum, the
 * libm restatements, KannalaBrandt8) by the headers the kernels share.  CPU tests and the stand-alone demo. */
#include "vslam_host.h"
#include "vslam_undistort.h"
#include "vslam_frustum.h"
#include "vslam_kb8.h"

#include <cmath>

extern "C" {

/* cv::undistortPoints as Frame::UndistortKeyPoints applies it (k1 == 0: unchanged), the shared vslam_undistort.h code:
 * cam = fx, fy, cx, cy; dist = ndist (4 or 5) coefficients; xy / out = n interleaved points */
int vslamh_undistort_points(const float* cam, const float* dist, int ndist, const float* xy, int n, float* out) {
    if (ndist != 4 && ndist != 5) return -1;
    float d[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; i++) d[i] = dist[i];
    for (int i = 0; i < n; i++) vslam_ud::frame_undistort(xy[2 * i], xy[2 * i + 1], cam, d, &out[2 * i], &out[2 * i + 1]);
    return 0;
}

/* Frame::ComputeImageBounds of a cols x rows image: minX, maxX, minY, maxY */
int vslamh_image_bounds(const float* cam, const float* dist, int ndist, int cols, int rows, float* b) {
    if (ndist != 4 && ndist != 5) return -1;
    float d[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; i++) d[i] = dist[i];
    vslam_ud::image_bounds(cam, d, cols, rows, b);
    return 0;
}

/* Frame::isInFrustum over n MapPoints, the shared vslam_frustum.h code (CPU tests, the stand-alone demo; the product runs
 * k_frustum).  Beside the parameters and the points it takes what the product reads from its context: the grid bounds in
 * force (bounds = minX, maxX, minY, maxY or NULL for {0, img_w, 0, img_h}) and the extractor's level count (the clamp of
 * PredictScale); depth_out may be NULL.  Returns nToMatch,
 * -1 for bad arguments. */
int vslamh_in_frustum(const vslam_frustum_params* p, const float* bounds, int nlevels, const vslam_map_point* points, int n,
                      vslam_mp_track* track_out, float* depth_out) {
    if (!p || n < 0 || nlevels < 1 || (n && (!points || !track_out))) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float depth;
        vslam_fr::in_frustum(F, points[i], &track_out[i], &depth);
        if (depth_out) depth_out[i] = depth;
        in_view += (int)(track_out[i].flags & 1u);
    }
    return in_view;
}

/* ---- fisheye cameras: the shared vslam_kb8.h code on the host (CPU tests, the stand-alone demo; the product runs the kernels
 * of vslam_kb8.hip) ---- */
static bool libm_args_ok(int fn, const float* a, const float* b, int n, const float* out) {
    return fn >= 0 && fn <= 4 && n >= 0 && (!n || (a && out && (fn != 4 || b)));
}
/* the libm restatements over n arguments: fn 0 atanf, 1 tanf, 2 sinf, 3 cosf (a, out), 4 atan2f (a = y, b = x) */
int vslamh_libm_twin(int fn, const float* a, const float* b, int n, float* out) {
    if (!libm_args_ok(fn, a, b, n, out)) return -1;
    for (int i = 0; i < n; i++)
        out[i] = fn == 0 ? vslam_kb8::glibc_atanf(a[i]) : fn == 1 ? vslam_kb8::glibc_tanf(a[i])
               : fn == 2 ? vslam_trig::glibc_sinf(a[i]) : fn == 3 ? vslam_trig::glibc_cosf(a[i])
                         : vslam_kb8::glibc_atan2f(a[i], b[i]);
    return 0;
}
/* the PLATFORM libm over the same arguments, for comparing large samples without a foreign call per value */
int vslamh_libm_platform(int fn, const float* a, const float* b, int n, float* out) {
    if (!libm_args_ok(fn, a, b, n, out)) return -1;
    for (int i = 0; i < n; i++)
        out[i] = fn == 0 ? ::atanf(a[i]) : fn == 1 ? ::tanf(a[i]) : fn == 2 ? ::sinf(a[i]) : fn == 3 ? ::cosf(a[i])
                                                                                                    : ::atan2f(a[i], b[i]);
    return 0;
}
float vslamh_atanf(float x) { return vslam_kb8::glibc_atanf(x); }
float vslamh_atan2f(float y, float x) { return vslam_kb8::glibc_atan2f(y, x); }
float vslamh_tanf(float x) { return vslam_kb8::glibc_tanf(x); }
float vslamh_sinf(float x) { return vslam_trig::glibc_sinf(x); }
float vslamh_cosf(float x) { return vslam_trig::glibc_cosf(x); }

int vslamh_kb8_project(const vslam_kb8_camera* cam, const float* xyz, int n, float* uv) {
    if (!vslam_kb8::camera_ok(cam) || n < 0 || (n && (!xyz || !uv))) return -1;
    for (int i = 0; i < n; i++) {
        const vslam_kb8::Uv o = vslam_kb8::kb8_project(*cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        uv[2 * i] = o.u;
        uv[2 * i + 1] = o.v;
    }
    return 0;
}
/* steps (may be NULL): Newton steps taken per pixel, 0 where theta_d <= 1e-8 */
int vslamh_kb8_unproject(const vslam_kb8_camera* cam, const float* uv, int n, float* xyz, int32_t* steps) {
    if (!vslam_kb8::camera_ok(cam) || n < 0 || (n && (!uv || !xyz))) return -1;
    for (int i = 0; i < n; i++) {
        int st = 0;
        const vslam_kb8::Ray r = vslam_kb8::kb8_unproject(*cam, uv[2 * i], uv[2 * i + 1], &st);
        xyz[3 * i] = r.x;
        xyz[3 * i + 1] = r.y;
        xyz[3 * i + 2] = r.z;
        if (steps) steps[i] = st;
    }
    return 0;
}
/* vslamh_in_frustum with KannalaBrandt8::project; the intrinsics of p must equal the camera's.  Returns nToMatch, -1 for bad
 * arguments. */
int vslamh_in_frustum_kb8(const vslam_frustum_params* p, const vslam_kb8_camera* cam, const float* bounds, int nlevels,
                          const vslam_map_point* points, int n, vslam_mp_track* track_out, float* depth_out) {
    if (!p || !vslam_kb8::camera_ok(cam) || n < 0 || nlevels < 1 || (n && (!points || !track_out))) return -1;
    if (!vslam_kb8::intrinsics_match(*p, *cam)) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float depth;
        vslam_kb8::in_frustum_kb8(F, *cam, points[i], &track_out[i], &depth);
        if (depth_out) depth_out[i] = depth;
        in_view += (int)(track_out[i].flags & 1u);
    }
    return in_view;
}
/* vslam_frame_in_frustum_rig on the host: returns the number of points either camera sees, -1 for bad arguments */
int vslamh_in_frustum_kb8_rig(const vslam_frustum_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                              const float* bounds, int nlevels, const vslam_map_point* points, int n,
                              vslam_mp_track* track_left, vslam_mp_track* track_right, float* depth_left,
                              float* depth_right) {
    if (!p || !rig || !vslam_kb8::camera_ok(cam) || !vslam_kb8::camera_ok(&rig->cam2) || n < 0 || nlevels < 1 ||
        (n && (!points || !track_left || !track_right)))
        return -1;
    if (!vslam_kb8::intrinsics_match(*p, *cam)) return -1;
    const float whole[4] = {0.0f, (float)p->img_w, 0.0f, (float)p->img_h};
    const vslam_fr::Frame F = vslam_fr::make_frame(*p, bounds ? bounds : whole, nlevels);
    const vslam_kb8::RigRight R = vslam_kb8::rig_right(F, *rig);
    int in_view = 0;
    for (int i = 0; i < n; i++) {
        float dl, dr;
        const bool l = vslam_kb8::in_frustum_check(F, F.Tcw, F.Ow, *cam, points[i], &track_left[i], &dl);
        const bool r = vslam_kb8::in_frustum_check(F, R.T, R.twc, rig->cam2, points[i], &track_right[i], &dr);
        if (depth_left) depth_left[i] = dl;
        if (depth_right) depth_right[i] = dr;
        in_view += (int)(l || r);
    }
    return in_view;
}
int vslamh_kb8_exclusive(int other_set, float k1) { /* either way round: the other kind is set and the pinhole one distorts */
    return (other_set && k1 != 0.0f) ? VSLAM_ERR_INVALID : VSLAM_OK;
}
int vslamh_kb8_frustum_check(const vslam_frustum_params* p, const vslam_kb8_camera* cam) {
    if (!p) return VSLAM_ERR_INVALID;
    if (!cam) return VSLAM_OK;
    return vslam_kb8::intrinsics_match(*p, *cam) ? VSLAM_OK : VSLAM_ERR_INVALID;
}
int vslamh_kb8_projecting_entry(int has_kb8) { return has_kb8 ? VSLAM_ERR_UNSUPPORTED : VSLAM_OK; }

} /* extern "C" */
