/* vslam_undistort.hip -- Frame::UndistortKeyPoints (frame.cpp:758-790) and Frame::ComputeImageBounds (:793-821) for
 * distorted pinhole cameras: the kernel behind every extraction pass of a context with a camera, and the camera ABI.
 *
 * k_undistort_kps: one lane per keypoint slot position over all slots of a pass; a lane whose position is below its
 * slot's count (read from HBM: the counts of the pass are not known on the host) copies the 28-byte keypoint and
 * replaces x, y by cv::undistortPoints (vslam_undistort.h, FP64, five iterations).  32 slots x N = 1000 is a few MFLOP.
 */
#include "vslam_ctx.h"
#include "vslam_undistort.h"

#ifndef UD_NT
#define UD_NT 256 /* lanes per workgroup */
#endif

__global__ void __launch_bounds__(UD_NT)
k_undistort_kps(const vslam_kp* __restrict__ kps, const int32_t* __restrict__ counts, vslam_kp* __restrict__ ukps, int cap,
                UdCam cam) {
    const int s = blockIdx.y;
    const int i = blockIdx.x * UD_NT + threadIdx.x;
    const int n = min(counts[s * 4], cap);
    if (i >= n) return;
    const size_t at = (size_t)s * cap + i;
    vslam_kp k = kps[at];
    vslam_ud::undistort_point(k.x, k.y, cam.cam, cam.dist, &k.x, &k.y);
    ukps[at] = k;
}

__global__ void __launch_bounds__(UD_NT) k_undistort_xy(const float* __restrict__ xy, int n, float* __restrict__ out, UdCam cam) {
    const int i = blockIdx.x * UD_NT + threadIdx.x;
    if (i >= n) return;
    vslam_ud::frame_undistort(xy[2 * i], xy[2 * i + 1], cam.cam, cam.dist, &out[2 * i], &out[2 * i + 1]);
}

void vk_undistort_kps(hipStream_t st, const vslam_kp* kps, const int32_t* counts, vslam_kp* ukps, int cap, int nimg,
                      const UdCam& cam) {
    if (nimg <= 0 || cap <= 0) return;
    hipLaunchKernelGGL(k_undistort_kps, dim3((cap + UD_NT - 1) / UD_NT, nimg), dim3(UD_NT), 0, st, kps, counts, ukps, cap,
                       cam);
}

void vk_undistort_xy(hipStream_t st, const float* xy, int n, float* out, const UdCam& cam) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_undistort_xy, dim3((n + UD_NT - 1) / UD_NT), dim3(UD_NT), 0, st, xy, n, out, cam);
}

static bool ud_active(const vslam_fe* fe) { return fe->has_cam && fe->ud.dist[0] != 0.0f; }

int vslam_enqueue_undistort(vslam_fe* fe, int nimg) {
    if (!ud_active(fe)) return VSLAM_OK; /* no camera, or k1 == 0: ukeypoints_ = keypoints_, nothing to launch */
    vk_undistort_kps(fe->stream, fe->d_kps, fe->d_counts, fe->d_ukps, fe->cap, nimg, fe->ud);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

extern "C" int vslam_fe_set_camera(vslam_fe* fe, const vslam_camera* cam) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (cam) {
        bool ok = (cam->ndist == 4 || cam->ndist == 5) && std::isfinite(cam->fx) && std::isfinite(cam->fy) &&
                  std::isfinite(cam->cx) && std::isfinite(cam->cy) && cam->fx != 0.0f && cam->fy != 0.0f;
        for (int i = 0; ok && i < cam->ndist; i++) ok = std::isfinite(cam->dist[i]);
        if (!ok) {
            g_err = "invalid camera (ndist 4 or 5, finite values, fx and fy not zero)";
            return VSLAM_ERR_INVALID;
        }
        if (vslamh_kb8_exclusive(fe->has_kb8, cam->dist[0])) {
            g_err = "a KB8 camera is set (vslam_fe_set_kb8_camera): fisheye frames have zero mDistCoef";
            return VSLAM_ERR_INVALID;
        }
    }
    HIPCHK(hipSetDevice(fe->p.device));
    if (fe->stream) HIPCHK(hipStreamSynchronize(fe->stream)); /* a pass in flight may still read the old camera */
    /* the coefficients are arguments of the captured k_undistort_kps (and a context without a camera captured no such
     * launch): drop the graph, the next host-image pass captures again */
    if (fe->graph_exec) {
        (void)hipGraphExecDestroy(fe->graph_exec);
        fe->graph_exec = nullptr;
        fe->graph_key = 0;
    }
    if (!cam) {
        fe->has_cam = false;
        return VSLAM_OK;
    }
    UdCam u;
    u.cam[0] = cam->fx;
    u.cam[1] = cam->fy;
    u.cam[2] = cam->cx;
    u.cam[3] = cam->cy;
    for (int i = 0; i < 5; i++) u.dist[i] = i < cam->ndist ? cam->dist[i] : 0.0f;
    if (u.dist[0] != 0.0f) /* lazily: contexts without such a camera keep their footprint */
        if (int rc = fe->d_ukps.ensure((size_t)fe->B * fe->cap)) return rc;
    fe->ud = u;
    fe->has_cam = true;
    return VSLAM_OK;
}

extern "C" int vslam_fe_slot_ukps(vslam_fe* fe, int slot, const vslam_kp** dev_ukps) {
    if (!fe || slot < 0 || slot >= fe->B || !dev_ukps) return VSLAM_ERR_INVALID;
    if (!fe->has_cam) {
        g_err = "no camera set (vslam_fe_set_camera)";
        return VSLAM_ERR_INVALID;
    }
    *dev_ukps = (ud_active(fe) ? fe->d_ukps : fe->d_kps) + (size_t)slot * fe->cap;
    return VSLAM_OK;
}

extern "C" int vslam_fe_ukps_copy(vslam_fe* fe, int slot, vslam_kp* dst, int cap, int* n) {
    const vslam_kp* src = nullptr;
    int rc = vslam_fe_slot_ukps(fe, slot, &src);
    if (rc) return rc;
    if (!n || cap < 0 || (cap && !dst)) return VSLAM_ERR_INVALID;
    HIPCHK(vslam_stream_wait(fe->stream));
    int32_t cnt = 0; /* the pass's own count (host copies of it are only refreshed by the waits) */
    HIPCHK(hipMemcpy(&cnt, fe->d_counts + (size_t)slot * 4, 4, hipMemcpyDeviceToHost));
    cnt = std::max(0, std::min(cnt, fe->cap));
    *n = cnt;
    if (cnt > cap) {
        g_err = "caller keypoint capacity too small";
        return VSLAM_ERR_CAPACITY;
    }
    if (cnt) HIPCHK(hipMemcpy(dst, src, (size_t)cnt * sizeof(vslam_kp), hipMemcpyDeviceToHost));
    return VSLAM_OK;
}

extern "C" int vslam_undistort_points(vslam_fe* fe, const float* xy, int n, float* out_xy) {
    if (!fe || n < 0 || (n && (!xy || !out_xy))) return VSLAM_ERR_INVALID;
    if (!fe->has_cam) {
        g_err = "no camera set (vslam_fe_set_camera)";
        return VSLAM_ERR_INVALID;
    }
    if (!n) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    int rc = fe->d_tmp_desc[1].ensure((size_t)n * 16);
    if (rc) return rc;
    float* d_in = (float*)fe->d_tmp_desc[1];
    float* d_out = d_in + 2 * (size_t)n;
    HIPCHK(hipMemcpyAsync(d_in, xy, (size_t)n * 8, hipMemcpyHostToDevice, fe->stream));
    vk_undistort_xy(fe->stream, d_in, n, d_out, fe->ud);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xy, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_fe_image_bounds(vslam_fe* fe, float bounds[4]) {
    if (!fe || !bounds) return VSLAM_ERR_INVALID;
    if (!fe->has_cam) {
        bounds[0] = 0.0f;
        bounds[1] = (float)fe->p.width;
        bounds[2] = 0.0f;
        bounds[3] = (float)fe->p.height;
        return VSLAM_OK;
    }
    vslam_ud::image_bounds(fe->ud.cam, fe->ud.dist, fe->p.width, fe->p.height, bounds);
    return VSLAM_OK;
}
