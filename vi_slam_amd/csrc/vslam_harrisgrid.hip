/* vslam_harrisgrid.hip -- the grid Harris / Shi-Tomasi detector, vilib::HarrisGPU (include/vslam_harrisgrid.h): the
 * response stage, the threshold step and the C ABI.  Pyramid, window, suppression, arg-max, level merge and host object:
 * vslam_griddet.h.
 *
 * What the reference runs for the response (CUDA, one launch per pyramid level and stage, five float images in global memory):
 *   K9 conv_filter_col_gpu_shm_kernel  (x2)     .../preprocess/conv_filter_col.cu:58-150 {.25,.5,.25} | {-1,0,1} down a column
 *   K8 conv_filter_row_gpu_shm_kernel  (x2)     .../preprocess/conv_filter_row.cu:58-146 {-1,0,1} | {.25,.5,.25} along a row, * 1/255
 *   K6 array_multiply_kernel           (x3)     .../feature_detection/harris/harris_gpu_cuda_tools.cu:91-121   DxDy, Dx2, Dy2
 *   K7 harris_gpu_calc_corner_response_kernel   .../harris_gpu_cuda_tools.cu:174-260    3x3 box sums, Harris | Shi-Tomasi
 *   host: processGridAndThreshold               .../feature_detection/detector_base_gpu.cpp:228-248
 * What runs here, inside k_hg_detect: the window carries a 3-pixel halo (1 NMS + 1 box + 1 filter) with the filter's
 * border rule applied to it; Dx, Dy of the cell + 2 px and the response of the cell + 1 px go into LDS.
 * Border rule on the window: the reference applies its rule per axis and per pass to an index one step outside the
 * image.  For the four index maps, T(map_x(x), y) of the column pass reads I(map_x(x), map_y(y +- 1)); for BORDER_ZERO
 * (and BORDER_SKIP, which runs the same kernels) either pass reads 0.  Both are one rule on the byte window:
 * win(x, y) = I(map_x(x), map_y(y)), or 0.  Indices two and three steps outside feed only derivatives outside the
 * image, which feed only responses outside [m, w-1-m] x [m, h-1-m], which are written as 0.
 * Products are recomputed from Dx, Dy at every box tap instead of being kept as three planes: 18 LDS reads per
 * response instead of 27, and two float planes in LDS instead of three (59 KB instead of 78 KB for a 64x64 cell);
 * the 27 multiplies are the cheapest thing on the CU.  The box sums keep the reference's raster association.
 * Every float operation is rounded on its own (the library builds with -ffp-contract=off; the intrinsics say so again).
 */
#include "../../include/vslam_harrisgrid.h"
#include "vslam_griddet.h"

struct HgDet { /* HgPolicy::Params */
    int32_t m, border, harris;
    float k;
};

struct vslam_hg : GdHost {
    HgDet D;
    float quality_level = 0.0f;
};

/* ---------------------------------------------------------------------------------------------- */
/* The source index of index i of an axis of n pixels (conv_filter_row.cu:81-123); -1: the value 0.  Exact one step
 * outside, which is all the 3-tap filters reach; merely inside the image further out. */
__device__ __forceinline__ int hg_border_index(int i, int n, int border) {
    if (i >= 0 && i < n) return i;
    int j;
    switch (border) {
        case VSLAM_HG_BORDER_REPLICATE: j = i; break;                                  /* clamped below */
        case VSLAM_HG_BORDER_REFLECT: j = i < 0 ? -i - 1 : 2 * n - 1 - i; break;
        case VSLAM_HG_BORDER_WRAP: j = i < 0 ? i + n : i - n; break;
        case VSLAM_HG_BORDER_REFLECT_101: j = i < 0 ? -i : 2 * n - 2 - i; break;
        default: return -1; /* BORDER_SKIP, BORDER_ZERO */
    }
    return min(max(j, 0), n - 1);
}
__device__ __forceinline__ uint8_t hg_border_px(const uint8_t* img, const FgLevel& lg, int gx, int gy, int border) {
    const int sx = hg_border_index(gx, lg.w, border), sy = hg_border_index(gy, lg.h, border);
    return (sx < 0 || sy < 0) ? (uint8_t)0 : img[(size_t)sy * lg.pitch + sx];
}

/* sum = 0.0f; sum += f[j] * v[j], j = 0, 1, 2 (conv_filter_row.cu:131-136, conv_filter_col.cu alike) */
__device__ __forceinline__ float hg_tap3(float f0, float f1, float f2, float v0, float v1, float v2) {
    float s = 0.0f;
    s = __fadd_rn(s, __fmul_rn(f0, v0));
    s = __fadd_rn(s, __fmul_rn(f1, v1));
    s = __fadd_rn(s, __fmul_rn(f2, v2));
    return s;
}

struct HgPolicy {
    typedef HgDet Params;
    static constexpr int kRowsAbove = 3; /* 1 NMS + 1 box + 1 filter */
    __host__ __device__ static int plane(int cwl, int chl) { return (cwl + 4) * (chl + 4); } /* floats of Dx, of Dy: the cell + 2 px */
    __host__ __device__ static size_t own_lds(int cwl, int chl) { return (size_t)plane(cwl, chl) * 8; }
    /* a pixel can be reported only in [m+1, w-2-m] x [m+1, h-2-m] */
    __device__ __forceinline__ static bool searchable(const FgLevel& lg, const HgDet& D) { return lg.w >= 2 * D.m + 3 && lg.h >= 2 * D.m + 3; }
    /* what the window holds outside the image is put right */
    template <int NT>
    __device__ __forceinline__ static void finish_window(const GdTile& t, const HgDet& D, int tid) {
        if (t.x0 < 4 || t.y0 < 3 || t.x0 + t.cwl + 4 > t.lg.w || t.y0 + t.chl + 3 > t.lg.h) { /* the window leaves the image */
            __syncthreads();
            for (int i = tid; i < t.WP * t.WH; i += NT) {
                const int wy = i / t.WP, wx = i - wy * t.WP;
                const int gx = t.x0 - 4 + wx, gy = t.y0 - 3 + wy;
                if (gx < 0 || gy < 0 || gx >= t.lg.w || gy >= t.lg.h) t.win[i] = hg_border_px(t.img, t.lg, gx, gy, D.border);
            }
        }
    }
    template <int NT>
    __device__ __forceinline__ static void response(const GdTile& t, const HgDet& D, int tid) {
        const int WP = t.WP, RP = t.RP, DP = t.cwl + 4, DH = t.chl + 4, m = D.m;
        const uint8_t* win = t.win;
        float* respS = t.respS;
        float* dxS = (float*)t.own;
        float* dyS = dxS + plane(t.cwl, t.chl);
        const float inv255 = 1.0f / 255.f, inv9 = 1.0f / 9.0f;
        /* K9 + K8: Dx, Dy of the cell + 2 px.  Element (ex, ey) is pixel (x0 - 2 + ex, y0 - 2 + ey). */
        const uint32_t mDP = ((1u << 20) + DP - 1) / DP;
        for (int i = tid; i < DP * DH; i += NT) {
            const int ey = (int)(mad24u((uint32_t)i, mDP, 0u) >> 20), ex = i - (int)mad24u((uint32_t)ey, (uint32_t)DP, 0u);
            const uint8_t* p = win + mad24u((uint32_t)(ey + 1), (uint32_t)WP, (uint32_t)(ex + 2));
            float ts[3], td[3]; /* column pass (scale 1.0f) at x - 1, x, x + 1: smoothing for Dx, difference for Dy */
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float tp = (float)p[c - 1 - WP], mid = (float)p[c - 1], b = (float)p[c - 1 + WP];
                ts[c] = __fmul_rn(hg_tap3(0.25f, 0.5f, 0.25f, tp, mid, b), 1.0f);
                td[c] = __fmul_rn(hg_tap3(-1.0f, 0.0f, 1.0f, tp, mid, b), 1.0f);
            }
            dxS[i] = __fmul_rn(hg_tap3(-1.0f, 0.0f, 1.0f, ts[0], ts[1], ts[2]), inv255);
            dyS[i] = __fmul_rn(hg_tap3(0.25f, 0.5f, 0.25f, td[0], td[1], td[2]), inv255);
        }
        __syncthreads();
        /* K6 + K7: the response of the cell + 1 px.  Element (rx, ry) is pixel (x0 - 1 + rx, y0 - 1 + ry). */
        const uint32_t mRP = ((1u << 20) + RP - 1) / RP;
        for (int i = tid; i < RP * t.RH; i += NT) {
            const int ry = (int)(mad24u((uint32_t)i, mRP, 0u) >> 20), rx = i - (int)mad24u((uint32_t)ry, (uint32_t)RP, 0u);
            const int gx = t.x0 - 1 + rx, gy = t.y0 - 1 + ry;
            float r = 0.0f;
            if (gx >= m && gy >= m && gx <= t.lg.w - 1 - m && gy <= t.lg.h - 1 - m) {
                const int o = (int)mad24u((uint32_t)ry, (uint32_t)DP, (uint32_t)rx); /* top-left tap: (rx + 1 - 1, ry + 1 - 1) */
                float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
                for (int dy = 0; dy < 3; dy++)
#pragma unroll
                    for (int dx = 0; dx < 3; dx++) { /* raster order from 0.0f, harris_gpu_cuda_tools.cu:183-205 */
                        const float vx = dxS[o + dy * DP + dx], vy = dyS[o + dy * DP + dx];
                        a = __fadd_rn(a, __fmul_rn(vx, vx));
                        b = __fadd_rn(b, __fmul_rn(vx, vy));
                        c = __fadd_rn(c, __fmul_rn(vy, vy));
                    }
                a = __fmul_rn(a, inv9);
                b = __fmul_rn(b, inv9);
                c = __fmul_rn(c, inv9);
                if (D.harris) { /* a*c - b*b - k*(a+c)*(a+c) */
                    const float tr = __fadd_rn(a, c);
                    r = __fsub_rn(__fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b)), __fmul_rn(__fmul_rn(D.k, tr), tr));
                } else { /* (a+c) - sqrtf((a-c)*(a-c) + 4*b*b) */
                    const float d = __fsub_rn(a, c);
                    /* sqrtf, not __fsqrt_rn: the latter is the approximate native square root unless OCML's rounded operations
                     * are compiled in; sqrtf is correctly rounded (no fast-math, fp32 correctly-rounded sqrt is hipcc's default) */
                    r = __fsub_rn(__fadd_rn(a, c), sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(__fmul_rn(4.0f, b), b))));
                }
            }
            respS[i] = r;
        }
    }
};

template <int NT>
__global__ void __launch_bounds__(NT)
k_hg_detect(const uint8_t* __restrict__ pyr, GdGeom G, HgDet D, uint8_t* grid, float* resp_out, int resp_level, int resp_slot) {
    gd_detect<NT, HgPolicy>(pyr, G, D, grid, resp_out, resp_level, resp_slot);
}

/* ---------------------------------------------------------------------------------------------- host */
static void hg_launch(const GdHost* h, int n, float* resp_out, int resp_level, int resp_slot) {
    gd_launch<HgPolicy>(*h, k_hg_detect<64>, k_hg_detect<128>, k_hg_detect<256>, static_cast<const vslam_hg*>(h)->D, n, resp_out,
                        resp_level, resp_slot);
}

extern "C" int vslam_hg_create(const vslam_hg_params* p, vslam_hg** out) {
    if (!p || !out) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    const int rc = gd_validate(*p, p->filter_border_type >= VSLAM_HG_BORDER_SKIP && p->filter_border_type <= VSLAM_HG_BORDER_REFLECT_101 &&
                                       p->quality_level >= 0.0f && p->harris_k == p->harris_k, "vslam_hg_create");
    if (rc != VSLAM_OK) return rc;
    vslam_hg* hg = new vslam_hg();
    hg->D.m = p->filter_border_type == VSLAM_HG_BORDER_SKIP ? 2 : 1; /* harris_gpu_cuda_tools.cu:284-287 */
    gd_fill(*hg, *p, hg->D.m + 1);                                    /* MINIMUM_BORDER, harris_gpu.cpp:58-59,81-82 */
    hg->launch = hg_launch;
    hg->D.border = p->filter_border_type;
    hg->D.harris = p->use_harris ? 1 : 0;
    hg->D.k = p->harris_k;
    hg->quality_level = p->quality_level;
    if (gd_alloc(*hg) != VSLAM_OK) {
        vslam_hg_destroy(hg);
        return VSLAM_ERR_HIP;
    }
    *out = hg;
    return VSLAM_OK;
}

extern "C" void vslam_hg_destroy(vslam_hg* hg) {
    if (!hg) return;
    gd_free(*hg);
    delete hg;
}

extern "C" int vslam_hg_grid(const vslam_hg* hg, int* n_cols, int* n_rows) { return gd_grid(hg, n_cols, n_rows); }

extern "C" int vslam_hg_detect_batch(vslam_hg* hg, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos,
                                     float* score, int32_t* level, uint8_t* keep, int32_t* n_keep) {
    const int rc = gd_detect_batch(hg, n, imgs, pitch, on_device, pos, score, level);
    if (rc != VSLAM_OK || (!keep && !n_keep)) return rc;
    const int C = hg->cells;
    for (int s = 0; s < n; s++) {
        /* processGridAndThreshold (detector_base_gpu.cpp:228-248), on the host after the one grid copy as there */
        const float* sc = score + (size_t)s * C;
        const float threshold = *std::max_element(sc, sc + C) * hg->quality_level;
        int32_t cnt = 0;
        for (int i = 0; i < C; i++) {
            const bool k = sc[i] > threshold;
            if (keep) keep[(size_t)s * C + i] = k ? 1 : 0;
            cnt += k ? 1 : 0;
        }
        if (n_keep) n_keep[s] = cnt;
    }
    return VSLAM_OK;
}

extern "C" int vslam_hg_detect(vslam_hg* hg, const uint8_t* img_host, size_t pitch, float* pos, float* score, int32_t* level,
                               uint8_t* keep, int32_t* n_keep) {
    const uint8_t* one[1] = {img_host};
    return vslam_hg_detect_batch(hg, 1, one, pitch, 0, pos, score, level, keep, n_keep);
}

extern "C" int vslam_hg_level_copy(vslam_hg* hg, int slot, int level, uint8_t* dst, size_t dst_pitch, int* w, int* h) {
    return gd_level_copy(hg, slot, level, dst, dst_pitch, w, h);
}

extern "C" int vslam_hg_response_copy(vslam_hg* hg, int slot, int level, float* dst) { return gd_response_copy(hg, slot, level, dst); }
