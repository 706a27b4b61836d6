/* vslam_kb8.hip -- fisheye cameras on the device: KannalaBrandt8::project / unproject over loose points and over a slot's
 * keypoints, Frame::isInFrustum with the fisheye projection, and the two-camera rig's frustum test (vslam_kb8.h), with the
 * camera ABI.
 *
 * k_kb8_project        one lane per point: two atan2f (one division and one polynomial each), one sqrt, sinf / cosf in FP64
 * k_kb8_unproject      one lane per pixel: at most ten Newton steps (one division each), one tanf
 * k_kb8_unproject_slot the same over a slot's keypoints; the count is read from HBM, no host wait
 * k_frustum_kb8        k_frustum (vslam_frustum.hip) with KannalaBrandt8::project: same arguments, same outputs, so
 *                      k_frustum_compact and the matcher behind it do not know the camera.  A second kernel: the pinhole
 *                      kernel's code is not touched.
 * k_frustum_rig        isInFrustumChecks for both cameras of a rig: two records and two depths per point, per chunk the number
 *                      of points either camera sees
 * All plain loads and stores, a few hundred FP32 operations per lane; no LDS beyond the chunk counts.
 */
#include "vslam_ctx.h"
#include "vslam_kb8.h"

#define KB8_NT 256 /* lanes per workgroup of the point kernels */

__global__ void __launch_bounds__(KB8_NT) k_kb8_project(const float* __restrict__ xyz, int n, float* __restrict__ uv,
                                                         vslam_kb8_camera cam) {
    const int i = blockIdx.x * KB8_NT + threadIdx.x;
    if (i >= n) return;
    const vslam_kb8::Uv o = vslam_kb8::kb8_project(cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    uv[2 * i] = o.u;
    uv[2 * i + 1] = o.v;
}

__global__ void __launch_bounds__(KB8_NT) k_kb8_unproject(const float* __restrict__ uv, int n, float* __restrict__ xyz,
                                                           vslam_kb8_camera cam) {
    const int i = blockIdx.x * KB8_NT + threadIdx.x;
    if (i >= n) return;
    const vslam_kb8::Ray r = vslam_kb8::kb8_unproject(cam, uv[2 * i], uv[2 * i + 1], nullptr);
    xyz[3 * i] = r.x;
    xyz[3 * i + 1] = r.y;
    xyz[3 * i + 2] = r.z;
}

__global__ void __launch_bounds__(KB8_NT) k_kb8_unproject_slot(const vslam_kp* __restrict__ kps,
                                                                const int32_t* __restrict__ count, int cap,
                                                                float* __restrict__ rays, vslam_kb8_camera cam) {
    const int i = blockIdx.x * KB8_NT + threadIdx.x;
    const int n = min(max(*count, 0), cap);
    if (i >= n) return;
    const vslam_kb8::Ray r = vslam_kb8::kb8_unproject(cam, kps[i].x, kps[i].y, nullptr);
    rays[3 * i] = r.x;
    rays[3 * i + 1] = r.y;
    rays[3 * i + 2] = r.z;
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK) k_frustum_kb8(FrustumArgsDev A, vslam_kb8_camera cam) {
    __shared__ int s_view[4], s_keep[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * VSLAM_FRUSTUM_CHUNK + tid;
    bool view = false, keep = false;
    if (i < A.n) {
        const vslam_map_point mp = A.pts[i];
        vslam_mp_track t;
        float depth;
        vslam_kb8::in_frustum_kb8(A.F, cam, mp, &t, &depth);
        A.track[i] = t;
        A.depth[i] = depth;
        view = (t.flags & 1u) != 0;
        keep = view && !(A.farPoints && depth > A.thFarPoints);
    }
    const unsigned long long bv = __ballot(view), bk = __ballot(keep);
    if (lane == 0) {
        s_view[wave] = __popcll(bv);
        s_keep[wave] = __popcll(bk);
    }
    __syncthreads();
    if (tid == 0) {
        A.chunkInView[blockIdx.x] = s_view[0] + s_view[1] + s_view[2] + s_view[3];
        A.chunkKeep[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
    }
}

__global__ void __launch_bounds__(VSLAM_FRUSTUM_CHUNK) k_frustum_rig(FrustumRigDev A) {
    __shared__ int s_view[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * VSLAM_FRUSTUM_CHUNK + tid;
    bool view = false;
    if (i < A.n) {
        const vslam_map_point mp = A.pts[i];
        vslam_mp_track tl, tr;
        float dl, dr;
        const bool l = vslam_kb8::in_frustum_check(A.F, A.F.Tcw, A.F.Ow, A.cam1, mp, &tl, &dl);
        const bool r = vslam_kb8::in_frustum_check(A.F, A.right.T, A.right.twc, A.cam2, mp, &tr, &dr);
        A.trackL[i] = tl;
        A.trackR[i] = tr;
        A.depthL[i] = dl;
        A.depthR[i] = dr;
        view = l || r;
    }
    const unsigned long long bv = __ballot(view);
    if (lane == 0) s_view[wave] = __popcll(bv);
    __syncthreads();
    if (tid == 0) A.chunkInView[blockIdx.x] = s_view[0] + s_view[1] + s_view[2] + s_view[3];
}

void vk_frustum_kb8(hipStream_t st, const FrustumArgsDev& A, const vslam_kb8_camera& cam) {
    if (A.n <= 0) return;
    const int nchunks = (A.n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    hipLaunchKernelGGL(k_frustum_kb8, dim3(nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A, cam);
}

void vk_frustum_rig(hipStream_t st, const FrustumRigDev& A) {
    if (A.n <= 0) return;
    const int nchunks = (A.n + VSLAM_FRUSTUM_CHUNK - 1) / VSLAM_FRUSTUM_CHUNK;
    hipLaunchKernelGGL(k_frustum_rig, dim3(nchunks), dim3(VSLAM_FRUSTUM_CHUNK), 0, st, A);
}

/* ------------------------------------------------------------------ ABI */
extern "C" int vslam_fe_set_kb8_camera(vslam_fe* fe, const vslam_kb8_camera* cam) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (cam && !vslam_kb8::camera_ok(cam)) {
        g_err = "invalid KB8 camera (finite values, fx and fy not zero)";
        return VSLAM_ERR_INVALID;
    }
    if (cam && vslamh_kb8_exclusive(fe->has_cam, fe->has_cam ? fe->ud.dist[0] : 0.0f)) {
        g_err = "a distorted pinhole camera (k1 != 0) is set: fisheye frames have zero mDistCoef";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    if (fe->stream) HIPCHK(hipStreamSynchronize(fe->stream)); /* a launch in flight took the old camera by value; be plain */
    fe->has_kb8 = cam != nullptr;
    if (cam) fe->kb8 = *cam;
    return VSLAM_OK;
}

static int kb8_need(const vslam_fe* fe) {
    if (!fe->has_kb8) {
        g_err = "no KB8 camera set (vslam_fe_set_kb8_camera)";
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

/* n_in floats per point up, kernel, n_out floats per point down, on the context's stream; blocking */
template <typename Launch>
static int kb8_points(vslam_fe* fe, const float* in, int n, int n_in, int n_out, float* out, Launch launch) {
    if (!fe || n < 0 || (n && (!in || !out))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_need(fe)) return rc;
    if (!n) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    if (int rc = fe->d_tmp_desc[1].ensure((size_t)n * (n_in + n_out) * 4)) return rc;
    float* d_in = (float*)fe->d_tmp_desc[1];
    float* d_out = d_in + (size_t)n_in * n;
    HIPCHK(hipMemcpyAsync(d_in, in, (size_t)n * n_in * 4, hipMemcpyHostToDevice, fe->stream));
    launch(d_in, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n * n_out * 4, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_kb8_project(vslam_fe* fe, const float* xyz_host, int n, float* uv_out) {
    return kb8_points(fe, xyz_host, n, 3, 2, uv_out, [&](const float* d_in, float* d_out) {
        hipLaunchKernelGGL(k_kb8_project, dim3((n + KB8_NT - 1) / KB8_NT), dim3(KB8_NT), 0, fe->stream, d_in, n, d_out, fe->kb8);
    });
}

extern "C" int vslam_kb8_unproject(vslam_fe* fe, const float* uv_host, int n, float* xyz_out) {
    return kb8_points(fe, uv_host, n, 2, 3, xyz_out, [&](const float* d_in, float* d_out) {
        hipLaunchKernelGGL(k_kb8_unproject, dim3((n + KB8_NT - 1) / KB8_NT), dim3(KB8_NT), 0, fe->stream, d_in, n, d_out,
                           fe->kb8);
    });
}

extern "C" int vslam_kb8_unproject_slot_async(vslam_fe* fe, int slot, float* dev_rays) {
    if (!fe || slot < 0 || slot >= fe->B || !dev_rays) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (int rc = kb8_need(fe)) return rc;
    HIPCHK(hipSetDevice(fe->p.device));
    hipLaunchKernelGGL(k_kb8_unproject_slot, dim3((fe->cap + KB8_NT - 1) / KB8_NT), dim3(KB8_NT), 0, fe->stream,
                       fe->d_kps + (size_t)slot * fe->cap, fe->d_counts + slot * 4, fe->cap, dev_rays, fe->kb8);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}
