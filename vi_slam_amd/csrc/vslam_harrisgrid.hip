/* vslam_harrisgrid.hip -- the grid Harris / Shi-Tomasi detector, vilib::HarrisGPU (include/vslam_harrisgrid.h).
 *
 * What the reference runs (all CUDA, one launch per pyramid level and stage, five float images in global memory):
 *   K5 image_halfsample_gpu_kernel              thirdparty/vilib/visual_lib/src/preprocess/pyramid_gpu.cu:76-96
 *   K9 conv_filter_col_gpu_shm_kernel  (x2)     .../preprocess/conv_filter_col.cu:58-150 {.25,.5,.25} | {-1,0,1} down a column
 *   K8 conv_filter_row_gpu_shm_kernel  (x2)     .../preprocess/conv_filter_row.cu:58-146 {-1,0,1} | {.25,.5,.25} along a row, * 1/255
 *   K6 array_multiply_kernel           (x3)     .../feature_detection/harris/harris_gpu_cuda_tools.cu:91-121   DxDy, Dx2, Dy2
 *   K7 harris_gpu_calc_corner_response_kernel   .../harris_gpu_cuda_tools.cu:174-260    3x3 box sums, Harris | Shi-Tomasi
 *   K3 detector_base_gpu_grid_nms_kernel        .../feature_detection/detector_base_gpu_cuda_tools.cu:700-878
 *   host: processGridAndThreshold               .../feature_detection/detector_base_gpu.cpp:228-248
 * What runs here:
 *   k_fg_gather / k_fg_halfsample   the pyramid of vslam_fastgrid.hip, through vslam_gridpyr.h
 *   k_hg_detect   ONE launch for every level, cell and image: a workgroup owns a grid cell, walks the levels, stages
 *                 the cell's byte window with a 3-pixel halo (1 NMS + 1 box + 1 filter) in LDS with the filter's border
 *                 rule applied while staging, computes Dx, Dy of the cell + 2 px and the response of the cell + 1 px
 *                 into LDS, then does K3's suppression and arg-max there and merges the levels in registers.  No float
 *                 image exists in HBM.
 * Border rule while staging: the reference applies its rule per axis and per pass to an index one step outside the
 * image.  For the four index maps, T(map_x(x), y) of the column pass reads I(map_x(x), map_y(y +- 1)); for BORDER_ZERO
 * (and BORDER_SKIP, which runs the same kernels) either pass reads 0.  Both are one rule on the byte window:
 * win(x, y) = I(map_x(x), map_y(y)), or 0.  Indices two and three steps outside feed only derivatives outside the
 * image, which feed only responses outside [m, w-1-m] x [m, h-1-m], which are written as 0.
 * Products are recomputed from Dx, Dy at every box tap instead of being kept as three planes: 18 LDS reads per
 * response instead of 27, and two float planes in LDS instead of three (59 KB instead of 78 KB for a 64x64 cell);
 * the 27 multiplies are the cheapest thing on the CU.  The box sums keep the reference's raster association.
 * Every float operation is rounded on its own (the library builds with -ffp-contract=off; the intrinsics say so again).
 * The K3 tail is k_fg_detect's, tie key included: see the header comment of vslam_fastgrid.hip.
 */
#include "../../include/vslam_harrisgrid.h"
#include "vslam_ctx.h"
#include "vslam_gridpyr.h"
#include "vslam_wave.h"

struct HgGeom {
    FgLevel lv[FG_MAX_LEVELS]; /* the pyramid of vslam_gridpyr.h */
    int32_t cw, ch, n_cols, n_rows, min_level, max_level, hb, vb, m, border, harris, tie;
    float k;
};

struct vslam_hg {
    vslam_hg_params p;
    HgGeom G;
    int cells = 0;
    size_t pyr_bytes = 0;
    hipStream_t stream = nullptr;
    uint8_t *d_pyr = nullptr, *h_img = nullptr, *d_grid = nullptr, *h_grid = nullptr;
    float* d_resp = nullptr;
    int last_n = 0;
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

__device__ __forceinline__ uint32_t hg_brev5(uint32_t v) { return __brev(v) >> 27; }

template <int NT>
__global__ void __launch_bounds__(NT)
k_hg_detect(const uint8_t* __restrict__ pyr, HgGeom G, uint8_t* grid, float* resp_out, int resp_level, int resp_slot) {
    extern __shared__ __align__(16) uint8_t hgsm[];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x, slot = blockIdx.y;
    const int ncell = G.n_cols * G.n_rows;
    const int per_xcd = (ncell + 7) >> 3; /* workgroups b and b+8 share an XCD: neighbouring cells per L2 */
    const int cell = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (cell >= ncell) return;
    const int cy = cell / G.n_cols, cx = cell - cy * G.n_cols;
    const int m = G.m;
    const float inv255 = 1.0f / 255.f, inv9 = 1.0f / 9.0f;
    float bestS = 0.0f, bestX = 0.0f, bestY = 0.0f;
    int bestL = -1;
    for (int l = G.min_level; l < G.max_level; l++) { /* every condition below is workgroup-uniform */
        const FgLevel lg = G.lv[l];
        const int cwl = G.cw >> l, chl = G.ch >> l;
        if (cwl < 1 || chl < 1) break;
        const int x0 = cwl * cx, y0 = chl * cy;
        /* a pixel can be reported only in [m+1, w-2-m] x [m+1, h-2-m] */
        if (lg.w < 2 * m + 3 || lg.h < 2 * m + 3 || x0 >= lg.w || y0 >= lg.h) continue;
        const uint8_t* img = pyr + lg.base + (size_t)slot * lg.bytes;
        /* window: origin (x0 - 4, y0 - 3), the 3-pixel halo plus one column each side for aligned dwords */
        const int WP = cwl + 8, WH = chl + 6, DP = cwl + 4, DH = chl + 4, RP = cwl + 2, RH = chl + 2;
        uint8_t* win = hgsm;
        float* dxS = (float*)(hgsm + ((WP * WH + 15) & ~15));
        float* dyS = dxS + DP * DH;
        float* respS = dyS + DP * DH;
        if (cwl >= 4) {
            /* x0 - 4 is a multiple of 4 (cell widths are), rows are 64-byte aligned: aligned dwords, their indices
             * clamped into the allocation; what lies outside the image is put right below */
            const int WD = WP >> 2, maxd = (lg.pitch >> 2) - 1, d0 = (x0 - 4) >> 2; /* arithmetic shift: -1 for x0 = 0 */
            const uint32_t mD = ((1u << 20) + WD - 1) / WD; /* i / WD == (i * mD) >> 20 for i < 2^20 / WD */
            for (int i = tid; i < WD * WH; i += NT) {
                const int wy = (int)(mad24u((uint32_t)i, mD, 0u) >> 20), wd = i - (int)mad24u((uint32_t)wy, (uint32_t)WD, 0u);
                const int gy = min(max(y0 - 3 + wy, 0), lg.h - 1), gd = min(max(d0 + wd, 0), maxd);
                ((uint32_t*)win)[i] = *(const uint32_t*)(img + mad24u((uint32_t)gy, (uint32_t)lg.pitch, 4u * (uint32_t)gd));
            }
            if (x0 < 4 || y0 < 3 || x0 + cwl + 4 > lg.w || y0 + chl + 3 > lg.h) { /* the window leaves the image */
                __syncthreads();
                for (int i = tid; i < WP * WH; i += NT) {
                    const int wy = i / WP, wx = i - wy * WP;
                    const int gx = x0 - 4 + wx, gy = y0 - 3 + wy;
                    if (gx < 0 || gy < 0 || gx >= lg.w || gy >= lg.h) win[i] = hg_border_px(img, lg, gx, gy, G.border);
                }
            }
        } else { /* 1- and 2-pixel cells of very coarse levels */
            for (int i = tid; i < WP * WH; i += NT) {
                const int wy = i / WP, wx = i - wy * WP;
                win[i] = hg_border_px(img, lg, x0 - 4 + wx, y0 - 3 + wy, G.border);
            }
        }
        if (tid == 0) s_best = 0ull;
        __syncthreads();
        /* K9 + K8: Dx, Dy of the cell + 2 px.  Element (ex, ey) is pixel (x0 - 2 + ex, y0 - 2 + ey). */
        const uint32_t mDP = ((1u << 20) + DP - 1) / DP;
        for (int i = tid; i < DP * DH; i += NT) {
            const int ey = (int)(mad24u((uint32_t)i, mDP, 0u) >> 20), ex = i - (int)mad24u((uint32_t)ey, (uint32_t)DP, 0u);
            const uint8_t* p = win + mad24u((uint32_t)(ey + 1), (uint32_t)WP, (uint32_t)(ex + 2));
            float ts[3], td[3]; /* column pass (scale 1.0f) at x - 1, x, x + 1: smoothing for Dx, difference for Dy */
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float t = (float)p[c - 1 - WP], mid = (float)p[c - 1], b = (float)p[c - 1 + WP];
                ts[c] = __fmul_rn(hg_tap3(0.25f, 0.5f, 0.25f, t, mid, b), 1.0f);
                td[c] = __fmul_rn(hg_tap3(-1.0f, 0.0f, 1.0f, t, mid, b), 1.0f);
            }
            dxS[i] = __fmul_rn(hg_tap3(-1.0f, 0.0f, 1.0f, ts[0], ts[1], ts[2]), inv255);
            dyS[i] = __fmul_rn(hg_tap3(0.25f, 0.5f, 0.25f, td[0], td[1], td[2]), inv255);
        }
        __syncthreads();
        /* K6 + K7: the response of the cell + 1 px.  Element (rx, ry) is pixel (x0 - 1 + rx, y0 - 1 + ry). */
        const uint32_t mRP = ((1u << 20) + RP - 1) / RP;
        for (int i = tid; i < RP * RH; i += NT) {
            const int ry = (int)(mad24u((uint32_t)i, mRP, 0u) >> 20), rx = i - (int)mad24u((uint32_t)ry, (uint32_t)RP, 0u);
            const int gx = x0 - 1 + rx, gy = y0 - 1 + ry;
            float r = 0.0f;
            if (gx >= m && gy >= m && gx <= lg.w - 1 - m && gy <= lg.h - 1 - m) {
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
                if (G.harris) { /* a*c - b*b - k*(a+c)*(a+c) */
                    const float tr = __fadd_rn(a, c);
                    r = __fsub_rn(__fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b)), __fmul_rn(__fmul_rn(G.k, tr), tr));
                } else { /* (a+c) - sqrtf((a-c)*(a-c) + 4*b*b) */
                    const float d = __fsub_rn(a, c);
                    /* sqrtf, not __fsqrt_rn: the latter is the approximate native square root unless OCML's rounded operations
                     * are compiled in; sqrtf is correctly rounded (no fast-math, fp32 correctly-rounded sqrt is hipcc's default) */
                    r = __fsub_rn(__fadd_rn(a, c), sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(__fmul_rn(4.0f, b), b))));
                }
            }
            respS[i] = r;
        }
        __syncthreads();
        if (resp_out && l == resp_level && slot == resp_slot)
            for (int i = tid; i < RP * RH; i += NT) {
                const int ry = i / RP, rx = i - ry * RP;
                const int gx = x0 - 1 + rx, gy = y0 - 1 + ry;
                if (rx >= 1 && rx <= cwl && ry >= 1 && ry <= chl && gx < lg.w && gy < lg.h) resp_out[(size_t)gy * lg.w + gx] = respS[i];
            }
        /* K3: 3x3 suppression (strictly_greater) + cell arg-max with the reference's tie order */
        const int bdx = cwl, bdy = max(1, min(128 / cwl, chl)); /* K3's block, detector_base_gpu_cuda_tools.cu:898-903 */
        const int yoff = max(0, G.vb - chl * cy);
        const int cshift = 31 - __clz(cwl); /* cell widths are powers of two */
        for (int i = tid; i < cwl * chl; i += NT) {
            const int py = i >> cshift, px = i & (cwl - 1);
            const int gx = x0 + px, gy = y0 + py;
            if (py < yoff || gx < G.hb || gx >= lg.w - G.hb || gy >= lg.h - G.vb) continue;
            const float* rp = respS + mad24u((uint32_t)(py + 1), (uint32_t)RP, (uint32_t)(px + 1));
            float c = rp[0];
            if (!(c > 0.0f)) continue; /* a non-positive response stays non-positive below and never beats 0 */
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++)
                    if (dx || dy) c = __fmul_rn(c, __fmul_rn(-0.5f, __fadd_rn(-1.0f, copysignf(1.0f, __fsub_rn(rp[dy * RP + dx], c)))));
            if (!(c > 0.0f)) continue;
            uint32_t prio;
            if (G.tie == 0) {
                const int ty = (py - yoff) & (bdy - 1); /* bdy is a power of two */
                const uint32_t t = (uint32_t)(px + bdx * ty);
                prio = ((t >> 5) << 17) | (hg_brev5(t & 31u) << 12) | (uint32_t)py;
            } else {
                prio = ((uint32_t)py << 12) | (uint32_t)px;
            }
            atomicMax(&s_best, ((unsigned long long)__float_as_uint(c) << 32) | (unsigned long long)(0xFFFFFFFFu - prio));
        }
        __syncthreads();
        if (tid == 0 && s_best) {
            const float r = __uint_as_float((uint32_t)(s_best >> 32));
            const uint32_t prio = 0xFFFFFFFFu - (uint32_t)s_best;
            int px, py;
            if (G.tie == 0) {
                const uint32_t t = ((prio >> 17) << 5) | hg_brev5((prio >> 12) & 31u);
                px = (int)(t % (uint32_t)bdx);
                py = (int)(prio & 0xFFFu);
            } else {
                px = (int)(prio & 0xFFFu);
                py = (int)(prio >> 12);
            }
            if (bestS < r) { /* levels in ascending order, strict: the finer level keeps a tie (:871-876) */
                const float scale = (float)(1 << l);
                bestS = r;
                bestX = __fmul_rn((float)(x0 + px), scale);
                bestY = __fmul_rn((float)(y0 + py), scale);
                bestL = l;
            }
        }
        __syncthreads();
    }
    if (tid == 0) { /* DetectorBaseGPU's SoA grid: pos (float2) | score | level */
        uint8_t* g = grid + (size_t)slot * ncell * 16;
        ((float2*)g)[cell] = make_float2(bestX, bestY);
        ((float*)(g + (size_t)ncell * 8))[cell] = bestS;
        ((int32_t*)(g + (size_t)ncell * 12))[cell] = bestL;
    }
}

/* ---------------------------------------------------------------------------------------------- host */
static size_t hg_lds_bytes(const HgGeom& G) {
    size_t m = 0;
    for (int l = G.min_level; l < G.max_level; l++) {
        const int cwl = G.cw >> l, chl = G.ch >> l;
        if (cwl < 1 || chl < 1) break;
        m = std::max(m, (size_t)(((cwl + 8) * (chl + 6) + 15) & ~15) + (size_t)(cwl + 4) * (chl + 4) * 8 + (size_t)(cwl + 2) * (chl + 2) * 4);
    }
    return m;
}

extern "C" int vslam_hg_create(const vslam_hg_params* p, vslam_hg** out) {
    if (!p || !out) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    if (p->image_width < 16 || p->image_height < 16 || p->image_width > 16384 || p->image_height > 16384 ||
        (p->cell_size_width != 32 && p->cell_size_width != 64) || (p->cell_size_height != 32 && p->cell_size_height != 64) ||
        p->min_level < 0 || p->max_level <= p->min_level || p->max_level > FG_MAX_LEVELS || p->horizontal_border < 0 ||
        p->vertical_border < 0 || p->filter_border_type < VSLAM_HG_BORDER_SKIP || p->filter_border_type > VSLAM_HG_BORDER_REFLECT_101 ||
        p->tie_rule < 0 || p->tie_rule > 1 || p->max_batch < 1 || p->max_batch > FG_MAX_BATCH || !(p->quality_level >= 0.0f) ||
        !(p->harris_k == p->harris_k)) {
        g_err = "vslam_hg_create: unsupported parameters";
        return VSLAM_ERR_INVALID;
    }
    /* the reference's own assertions: pyramid_pool.cpp:58-59, detector_base_gpu.cpp:62 */
    if ((p->image_width % (1 << (p->max_level - 1))) || (p->image_height % (1 << (p->max_level - 1))) ||
        (p->cell_size_height % (1 << (p->max_level - 1)))) {
        g_err = "vslam_hg_create: image and cell sizes must be divisible by 2^(max_level-1)";
        return VSLAM_ERR_INVALID;
    }
    vslam_hg* hg = new vslam_hg();
    hg->p = *p;
    HgGeom& G = hg->G;
    memset(&G, 0, sizeof(G));
    G.cw = p->cell_size_width;
    G.ch = p->cell_size_height;
    G.n_cols = (p->image_width + G.cw - 1) / G.cw; /* detector_base.cpp:54-55 */
    G.n_rows = (p->image_height + G.ch - 1) / G.ch;
    G.min_level = p->min_level;
    G.max_level = p->max_level;
    G.m = p->filter_border_type == VSLAM_HG_BORDER_SKIP ? 2 : 1; /* harris_gpu_cuda_tools.cu:284-287 */
    G.hb = std::max(G.m + 1, p->horizontal_border);              /* MINIMUM_BORDER, harris_gpu.cpp:58-59,81-82 */
    G.vb = std::max(G.m + 1, p->vertical_border);
    G.border = p->filter_border_type;
    G.harris = p->use_harris ? 1 : 0;
    G.tie = p->tie_rule;
    G.k = p->harris_k;
    hg->cells = G.n_cols * G.n_rows;
    hg->pyr_bytes = fg_pyramid_layout(G.lv, p->image_width, p->image_height, G.max_level, p->max_batch);
#define HG_TRY(call)                                                      \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                           \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);    \
            vslam_hg_destroy(hg);                                         \
            return VSLAM_ERR_HIP;                                         \
        }                                                                 \
    } while (0)
    HG_TRY(hipSetDevice(p->device));
    HG_TRY(hipStreamCreateWithFlags(&hg->stream, hipStreamNonBlocking));
    HG_TRY(hipMalloc((void**)&hg->d_pyr, hg->pyr_bytes));
    HG_TRY(hipMemset(hg->d_pyr, 0, hg->pyr_bytes));
    HG_TRY((hipError_t)vslam_pinned_alloc((void**)&hg->h_img, G.lv[0].bytes * p->max_batch));
    memset(hg->h_img, 0, G.lv[0].bytes * p->max_batch);
    HG_TRY(hipMalloc((void**)&hg->d_grid, (size_t)hg->cells * 16 * p->max_batch));
    HG_TRY((hipError_t)vslam_pinned_alloc((void**)&hg->h_grid, (size_t)hg->cells * 16 * p->max_batch));
    HG_TRY(hipMalloc((void**)&hg->d_resp, (size_t)p->image_width * p->image_height * 4));
    HG_TRY(hipDeviceSynchronize());
#undef HG_TRY
    *out = hg;
    return VSLAM_OK;
}

extern "C" void vslam_hg_destroy(vslam_hg* hg) {
    if (!hg) return;
    (void)hipSetDevice(hg->p.device);
    if (hg->stream) (void)hipStreamSynchronize(hg->stream);
    if (hg->d_pyr) (void)hipFree(hg->d_pyr);
    if (hg->h_img) (void)hipHostFree(hg->h_img);
    if (hg->d_grid) (void)hipFree(hg->d_grid);
    if (hg->h_grid) (void)hipHostFree(hg->h_grid);
    if (hg->d_resp) (void)hipFree(hg->d_resp);
    if (hg->stream) (void)hipStreamDestroy(hg->stream);
    delete hg;
}

extern "C" int vslam_hg_grid(const vslam_hg* hg, int* n_cols, int* n_rows) {
    if (!hg) return VSLAM_ERR_INVALID;
    if (n_cols) *n_cols = hg->G.n_cols;
    if (n_rows) *n_rows = hg->G.n_rows;
    return VSLAM_OK;
}

static int hg_nt() { /* threads per cell: the grid detectors share the process-wide fg_threads */
    const int v = vslam_process_tuning().fg_threads;
    return (v == 64 || v == 128 || v == 256) ? v : 128;
}

static void hg_launch_detect(vslam_hg* hg, int n, float* resp_out, int resp_level, int resp_slot) {
    const HgGeom& G = hg->G;
    const dim3 grid(((hg->cells + 7) / 8) * 8, n);
    const size_t lds = hg_lds_bytes(G);
    switch (hg_nt()) {
        case 64:
            hipLaunchKernelGGL(k_hg_detect<64>, grid, dim3(64), lds, hg->stream, hg->d_pyr, G, hg->d_grid, resp_out, resp_level,
                               resp_slot);
            break;
        case 128:
            hipLaunchKernelGGL(k_hg_detect<128>, grid, dim3(128), lds, hg->stream, hg->d_pyr, G, hg->d_grid, resp_out,
                               resp_level, resp_slot);
            break;
        default:
            hipLaunchKernelGGL(k_hg_detect<256>, grid, dim3(256), lds, hg->stream, hg->d_pyr, G, hg->d_grid, resp_out,
                               resp_level, resp_slot);
    }
}

extern "C" int vslam_hg_detect_batch(vslam_hg* hg, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos,
                                     float* score, int32_t* level, uint8_t* keep, int32_t* n_keep) {
    if (!hg || n < 1 || n > hg->p.max_batch || !imgs || !pos || !score || !level || pitch < (size_t)hg->p.image_width) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int s = 0; s < n; s++)
        if (!imgs[s]) {
            g_err = "null image";
            return VSLAM_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(hg->p.device));
    const HgGeom& G = hg->G;
    const FgLevel& L0 = G.lv[0];
    hipStream_t st = hg->stream;
    if (on_device) {
        fg_pyramid_gather(st, imgs, n, pitch, hg->d_pyr, L0);
    } else { /* pageable rows -> pinned staging in the device layout -> one copy kernel (see vslam_fe.hip) */
        for (int s = 0; s < n; s++)
            for (int y = 0; y < L0.h; y++) memcpy(hg->h_img + (size_t)s * L0.bytes + (size_t)y * L0.pitch, imgs[s] + (size_t)y * pitch, L0.w);
        CopyRanges R;
        memset(&R, 0, sizeof(R));
        R.dst[0] = hg->d_pyr + L0.base;
        R.src[0] = hg->h_img;
        R.bytes[0] = L0.bytes * n;
        R.n = 1;
        vk_copy_ranges(st, R);
    }
    fg_pyramid_halfsample(st, hg->d_pyr, G.lv, G.max_level, n);
    hg_launch_detect(hg, n, nullptr, -1, -1);
    CopyRanges R;
    memset(&R, 0, sizeof(R));
    R.dst[0] = hg->h_grid;
    R.src[0] = hg->d_grid;
    R.bytes[0] = (size_t)hg->cells * 16 * n;
    R.n = 1;
    vk_copy_ranges(st, R);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    hg->last_n = n;
    const int C = hg->cells;
    for (int s = 0; s < n; s++) {
        const uint8_t* g = hg->h_grid + (size_t)s * C * 16;
        memcpy(pos + (size_t)s * C * 2, g, (size_t)C * 8);
        memcpy(score + (size_t)s * C, g + (size_t)C * 8, (size_t)C * 4);
        memcpy(level + (size_t)s * C, g + (size_t)C * 12, (size_t)C * 4);
        if (!keep && !n_keep) continue;
        /* processGridAndThreshold (detector_base_gpu.cpp:228-248), on the host after the one grid copy as there */
        const float* sc = score + (size_t)s * C;
        const float threshold = *std::max_element(sc, sc + C) * hg->p.quality_level;
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
    if (!hg || slot < 0 || slot >= hg->last_n || level < 0 || level >= hg->G.max_level) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const FgLevel& L = hg->G.lv[level];
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (!dst) return VSLAM_OK;
    if (dst_pitch < (size_t)L.w) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(hg->p.device));
    HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, hg->d_pyr + L.base + (size_t)slot * L.bytes, L.pitch, L.w, L.h, hipMemcpyDeviceToHost,
                            hg->stream));
    HIPCHK(hipStreamSynchronize(hg->stream));
    return VSLAM_OK;
}

extern "C" int vslam_hg_response_copy(vslam_hg* hg, int slot, int level, float* dst) {
    if (!hg || !dst || slot < 0 || slot >= hg->last_n || level < hg->G.min_level || level >= hg->G.max_level) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const FgLevel& L = hg->G.lv[level];
    HIPCHK(hipSetDevice(hg->p.device));
    HIPCHK(hipMemsetAsync(hg->d_resp, 0, (size_t)L.w * L.h * 4, hg->stream));
    hg_launch_detect(hg, hg->last_n, hg->d_resp, level, slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, hg->d_resp, (size_t)L.w * L.h * 4, hipMemcpyDeviceToHost, hg->stream));
    HIPCHK(hipStreamSynchronize(hg->stream));
    return VSLAM_OK;
}
