/* vslam_fastgrid.hip -- the grid FAST detector behind vi_slam::geometry::FAST::detect (include/vslam_fastgrid.h): the
 * response stage and the C ABI.  Pyramid, window, suppression, arg-max, level merge and host object: vslam_griddet.h.
 *
 * What the reference runs for the response (CUDA, one launch per pyramid level and stage):
 *   K1 fast_gpu_calculate_lut_kernel          .../feature_detection/fast/fast_gpu_cuda_tools.cu:142-166   (64 Ki-entry LUT)
 *   K2 fast_gpu_calc_corner_response_kernel   .../fast_gpu_cuda_tools.cu:244-420    (float response image in global memory)
 * What runs here, inside k_fg_detect: the window carries the 1 px NMS halo + the 3 px Bresenham ring; the response of
 * the cell and its halo goes into LDS.  K1's table is replaced by a shift-and-AND run test on the 16-bit mask (same
 * predicate).
 */
#include "../../include/vslam_fastgrid.h"
#include "vslam_griddet.h"

struct FgDet { /* FgPolicy::Params */
    int32_t dhb, dvb, arc, score;
    float thr;
};

struct vslam_fg : GdHost {
    FgDet D;
};

/* ---------------------------------------------------------------------------------------------- */
/* a circular run of >= arc ones in the low 16 bits (fast_gpu_is_corner, fast_gpu_cuda_tools.cu:97-114) */
__device__ __forceinline__ bool fg_is_corner(uint32_t m, int arc) {
    if (__popc(m) < arc) return false;
    const uint32_t d = m | (m << 16);
    uint32_t r = d;
    for (int k = 1; k < arc; k++) r &= d >> k;
    return (r & 0xFFFFu) != 0;
}
__device__ __forceinline__ uint32_t fg_sign(float v) { return __float_as_uint(v) >> 31; } /* signbit() */

/* fast_gpu_prechecks (fast_gpu_cuda_tools.cu:116-139): true = cannot be a corner.  Exact for arcs >= 9 (which
 * the constructor asserts): an arc of 9 contains one pixel of every opposite pair. */
__device__ __forceinline__ bool fg_precheck_fails(const uint8_t* p, int wp, float thr) {
    const float c = (float)p[0];
    const float ct = __fadd_rn(c, thr), c_t = __fsub_rn(c, thr);
    float a = (float)p[-3], b = (float)p[3];
    if ((fg_sign(__fsub_rn(a, c_t)) | fg_sign(__fsub_rn(b, c_t)) | fg_sign(__fsub_rn(ct, a)) | fg_sign(__fsub_rn(ct, b))) == 0) return true;
    a = (float)p[3 * wp];
    b = (float)p[-3 * wp];
    return (fg_sign(__fsub_rn(a, c_t)) | fg_sign(__fsub_rn(b, c_t)) | fg_sign(__fsub_rn(ct, a)) | fg_sign(__fsub_rn(ct, b))) == 0;
}

/* K2 for one pixel that passed the prechecks; its window address is p (LDS, pitch wp).  Forced inline: left to itself
 * hipcc calls it from FgPolicy::response, and the detector takes 8-9 % longer */
__device__ __forceinline__ float fg_response_px(const uint8_t* p, int wp, float thr, int arc, int score) {
    const float c = (float)p[0];
    const float ct = __fadd_rn(c, thr), c_t = __fsub_rn(c, thr);
    /* ring order of bresenham_circle_offset_pitch (:41-95) */
    const int off[16] = {3 * wp,      3 * wp - 1,  2 * wp - 2,  wp - 3,  -3,     -wp - 3,    -2 * wp - 2, -3 * wp - 1,
                         -3 * wp,     -3 * wp + 1, -2 * wp + 2, -wp + 3, 3,      wp + 3,     2 * wp + 2,  3 * wp + 1};
    float px[16];
    uint32_t dark = 0, bright = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        px[i] = (float)p[off[i]];
        dark |= fg_sign(__fsub_rn(px[i], c_t)) << i;
        bright |= fg_sign(__fsub_rn(ct, px[i])) << i;
    }
    if (!(fg_is_corner(dark, arc) || fg_is_corner(bright, arc))) return 0.0f;
    if (score == VSLAM_FG_SUM_OF_ABS_DIFF_ALL) {
        float r = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; i++) r = __fadd_rn(r, fabsf(__fsub_rn(px[i], c)));
        return r;
    }
    if (score == VSLAM_FG_SUM_OF_ABS_DIFF_ON_ARC) {
        float rb = 0.0f, rd = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float ad = __fsub_rn(fabsf(__fsub_rn(px[i], c)), thr);
            rd = __fadd_rn(rd, (dark >> i) & 1u ? ad : 0.0f);
            rb = __fadd_rn(rb, (bright >> i) & 1u ? ad : 0.0f);
        }
        return fmaxf(rb, rd);
    }
    float mn = __fadd_rn(thr, 1.0f), mx = 255.0f; /* MAX_THRESHOLD: binary search, :386-415 */
    while (mn <= mx) {
        const float med = floorf(__fmul_rn(__fadd_rn(mn, mx), 0.5f));
        const float mct = __fadd_rn(c, med), mc_t = __fsub_rn(c, med);
        uint32_t dk = 0, br = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            dk |= fg_sign(__fsub_rn(px[i], mc_t)) << i;
            br |= fg_sign(__fsub_rn(mct, px[i])) << i;
        }
        if (fg_is_corner(dk, arc) || fg_is_corner(br, arc)) mn = __fadd_rn(med, 1.0f);
        else mx = __fsub_rn(med, 1.0f);
    }
    return mx;
}

__device__ __forceinline__ int& fg_nlist() { /* the survivor counter */
    __shared__ int s_nlist;
    return s_nlist;
}

struct FgPolicy {
    typedef FgDet Params;
    static constexpr int kRowsAbove = 4;                                                                  /* 1 halo + 3 ring */
    __host__ __device__ static size_t own_lds(int cwl, int chl) { return (size_t)(cwl + 2) * (chl + 2) * 2; } /* the list */
    __device__ __forceinline__ static bool searchable(const FgLevel& lg, const FgDet&) { return lg.w >= 7 && lg.h >= 7; }
    /* Bytes outside the image are never used by a pixel inside the detection border: the window stays as staged */
    template <int NT>
    __device__ __forceinline__ static void finish_window(const GdTile&, const FgDet&, int tid) {
        if (tid == 0) fg_nlist() = 0;
    }
    /* K2 on the cell and its 1-px halo, in two passes: the cheap prechecks on every pixel, the survivors
     * (a quarter of the pixels on textured images) compacted into a list so that the expensive part -- ring
     * gather, masks, arc test, score -- runs on dense lanes */
    template <int NT>
    __device__ __forceinline__ static void response(const GdTile& t, const FgDet& D, int tid) {
        const int WP = t.WP, RP = t.RP;
        const uint8_t* win = t.win;
        float* respS = t.respS;
        uint16_t* list = (uint16_t*)t.own;
        const uint32_t mRP = ((1u << 20) + RP - 1) / RP; /* i / RP == (i * mRP) >> 20 for i < 2^20 / RP */
        for (int i = tid; i < RP * t.RH; i += NT) {
            const int ry = (int)(mad24u((uint32_t)i, mRP, 0u) >> 20), rx = i - (int)mad24u((uint32_t)ry, (uint32_t)RP, 0u);
            const int gx = t.x0 - 1 + rx, gy = t.y0 - 1 + ry;
            respS[i] = 0.0f;
            const bool cand = gx >= D.dhb && gy >= D.dvb && gx < t.lg.w - D.dhb && gy < t.lg.h - D.dvb &&
                              !fg_precheck_fails(win + mad24u((uint32_t)(ry + 3), (uint32_t)WP, (uint32_t)(rx + 3)), WP, D.thr);
            const unsigned long long m = __ballot(cand);
            if (m) { /* wave-uniform */
                const int lane = tid & 63;
                int base = 0;
                if (lane == 0) base = atomicAdd(&fg_nlist(), __popcll(m));
                base = __shfl(base, 0, 64);
                if (cand) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
            }
        }
        __syncthreads();
        const int nlist = fg_nlist();
        for (int k = tid; k < nlist; k += NT) {
            const int i = list[k];
            const int ry = (int)(mad24u((uint32_t)i, mRP, 0u) >> 20), rx = i - (int)mad24u((uint32_t)ry, (uint32_t)RP, 0u);
            respS[i] = fg_response_px(win + mad24u((uint32_t)(ry + 3), (uint32_t)WP, (uint32_t)(rx + 3)), WP, D.thr, D.arc, D.score);
        }
    }
};

template <int NT>
__global__ void __launch_bounds__(NT)
k_fg_detect(const uint8_t* __restrict__ pyr, GdGeom G, FgDet D, uint8_t* grid, float* resp_out, int resp_level, int resp_slot) {
    gd_detect<NT, FgPolicy>(pyr, G, D, grid, resp_out, resp_level, resp_slot);
}

/* ---------------------------------------------------------------------------------------------- host */
static void fg_launch(const GdHost* h, int n, float* resp_out, int resp_level, int resp_slot) {
    gd_launch<FgPolicy>(*h, k_fg_detect<64>, k_fg_detect<128>, k_fg_detect<256>, static_cast<const vslam_fg*>(h)->D, n, resp_out,
                        resp_level, resp_slot);
}

extern "C" int vslam_fg_create(const vslam_fg_params* p, vslam_fg** out) {
    if (!p || !out) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    const int rc = gd_validate(*p, p->min_arc_length >= 9 && p->min_arc_length <= 12 && p->score >= 0 && p->score <= 2 && p->threshold >= 0.0f,
                               "vslam_fg_create");
    if (rc != VSLAM_OK) return rc;
    vslam_fg* fg = new vslam_fg();
    gd_fill(*fg, *p, 3); /* fast_gpu.cpp:66-67 */
    fg->launch = fg_launch;
    fg->D.dhb = std::max(3, p->horizontal_border - 1); /* fast_gpu.cpp:72-73 (DETECTOR_BASE_NMS_SIZE / 2 = 1) */
    fg->D.dvb = std::max(3, p->vertical_border - 1);
    fg->D.arc = p->min_arc_length;
    fg->D.score = p->score;
    fg->D.thr = p->threshold;
    if (gd_alloc(*fg) != VSLAM_OK) {
        vslam_fg_destroy(fg);
        return VSLAM_ERR_HIP;
    }
    *out = fg;
    return VSLAM_OK;
}

extern "C" void vslam_fg_destroy(vslam_fg* fg) {
    if (!fg) return;
    gd_free(*fg);
    delete fg;
}

extern "C" int vslam_fg_grid(const vslam_fg* fg, int* n_cols, int* n_rows) { return gd_grid(fg, n_cols, n_rows); }

extern "C" int vslam_fg_detect_batch(vslam_fg* fg, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos,
                                     float* score, int32_t* level) {
    return gd_detect_batch(fg, n, imgs, pitch, on_device, pos, score, level);
}

extern "C" int vslam_fg_detect(vslam_fg* fg, const uint8_t* img_host, size_t pitch, float* pos, float* score, int32_t* level) {
    const uint8_t* one[1] = {img_host};
    return gd_detect_batch(fg, 1, one, pitch, 0, pos, score, level);
}

extern "C" int vslam_fg_level_copy(vslam_fg* fg, int slot, int level, uint8_t* dst, size_t dst_pitch, int* w, int* h) {
    return gd_level_copy(fg, slot, level, dst, dst_pitch, w, h);
}

extern "C" int vslam_fg_response_copy(vslam_fg* fg, int slot, int level, float* dst) { return gd_response_copy(fg, slot, level, dst); }
