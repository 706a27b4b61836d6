/* vslam_griddet.h -- what the grid detectors share, as vilib's DetectorBaseGPU shares it: the half-sampled pyramid
 * (vilib::Frame over a PyramidPool: thirdparty/vilib/visual_lib/src/common/frame.cpp:49-57), the cell-to-workgroup
 * mapping, the LDS window, the 3x3 suppression with the cell arg-max, the level merge, the feature grid and the host
 * object.  vslam_fastgrid.hip and vslam_harrisgrid.hip each add a response stage as a policy; vslam_griddet.hip holds
 * the pyramid kernels and the host functions declared at the end.
 *
 * What the reference runs around a detector's response kernels (all CUDA, warp = 32, one launch per level and stage):
 *   K5 image_halfsample_gpu_kernel           thirdparty/vilib/visual_lib/src/preprocess/pyramid_gpu.cu:76-96
 *   K3 detector_base_gpu_grid_nms_kernel     .../feature_detection/detector_base_gpu_cuda_tools.cu:700-878 (reads the
 *                                            response image in global memory 9x per pixel)
 * What runs here:
 *   k_fg_halfsample  one thread = 4 output pixels from two 8-byte loads per source row, whole batch per launch
 *   gd_detect<NT, Pol>, behind k_fg_detect<NT> and k_hg_detect<NT>: ONE launch for every level, cell and image.  A
 *                    workgroup owns a grid cell, walks the levels, stages the cell's byte window in LDS, has the policy
 *                    compute the response of the cell and its 1-px halo into LDS (no float image exists in HBM), does
 *                    K3's suppression and the cell arg-max there and merges the levels in registers.
 * A policy Pol supplies: Params (its block of kernel arguments), kRowsAbove (window rows above and below the cell; the
 * window always has 4 columns each side, for aligned dwords), own_lds (the LDS it needs behind window | respS),
 * searchable (can this level hold a feature at all), finish_window (runs between the window's stores and the barrier
 * that publishes them) and response (fills respS).
 * Which of several equal maxima of a cell is reported is decided in the reference by K3's launch geometry: a thread
 * per column keeps its topmost maximum, a 32-lane __shfl_down_sync tree prefers the lane whose 5-bit index reads
 * smallest when bit-reversed, warps and then levels are merged in ascending order with strict '>'.  The arg-max
 * key below carries exactly that priority (tie_rule 0); tie_rule 1 is plain raster order (rosten::FASTCPU<true>).
 */
#ifndef VSLAM_GRIDDET_H
#define VSLAM_GRIDDET_H

#include "vslam_ctx.h"
#include "vslam_wave.h"

#define FG_MAX_LEVELS 8
#define FG_MAX_BATCH 64
#define GD_MAX_CELL 64 /* cells are 32 or 64 pixels wide and high */
static_assert(GD_MAX_CELL <= 0xFFF, "the arg-max key gives a cell's row and column 12 bits each");

struct FgLevel {
    int32_t w, h, pitch;
    uint32_t pad;
    size_t base, bytes; /* level-major layout: image s of level l starts at base + s * bytes */
};
struct FgPtrs {
    const uint8_t* p[FG_MAX_BATCH];
};
struct GdGeom { /* a detector's kernels take this and the policy's Params */
    FgLevel lv[FG_MAX_LEVELS];
    int32_t cw, ch, n_cols, n_rows, min_level, max_level, hb, vb, tie;
};
struct GdTile { /* one cell on one level; every member is workgroup-uniform */
    FgLevel lg;
    const uint8_t* img;
    int x0, y0, cwl, chl; /* the cell's origin and size on this level */
    int WP, WH, RP, RH;   /* window (origin x0 - 4, y0 - kRowsAbove) and response (origin x0 - 1, y0 - 1) sizes */
    uint8_t* win;
    float* respS;
    uint8_t* own;
};

/* the LDS layout window | respS | policy's own, for the kernel and for the host's sizing */
__host__ __device__ inline int gd_win_bytes(int cwl, int chl, int rows) { return ((cwl + 8) * (chl + 2 * rows) + 15) & ~15; }
template <class Pol>
size_t gd_lds_bytes(const GdGeom& G) {
    size_t m = 0;
    for (int l = G.min_level; l < G.max_level; l++) {
        const int cwl = G.cw >> l, chl = G.ch >> l;
        if (cwl < 1 || chl < 1) break;
        m = std::max(m, (size_t)gd_win_bytes(cwl, chl, Pol::kRowsAbove) + (size_t)(cwl + 2) * (chl + 2) * 4 + Pol::own_lds(cwl, chl));
    }
    return m;
}

__device__ __forceinline__ uint32_t gd_brev5(uint32_t v) { return __brev(v) >> 27; }

template <int NT, class Pol>
__device__ __forceinline__ void gd_detect(const uint8_t* __restrict__ pyr, const GdGeom& G, const typename Pol::Params& D,
                                          uint8_t* grid, float* resp_out, int resp_level, int resp_slot) {
    extern __shared__ __align__(16) uint8_t gdsm[];
    __shared__ unsigned long long s_best;
    constexpr int RA = Pol::kRowsAbove;
    const int tid = threadIdx.x, slot = blockIdx.y;
    const int ncell = G.n_cols * G.n_rows;
    const int per_xcd = (ncell + 7) >> 3; /* workgroups b and b+8 share an XCD: neighbouring cells per L2 */
    const int cell = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (cell >= ncell) return;
    const int cy = cell / G.n_cols, cx = cell - cy * G.n_cols;
    float bestS = 0.0f, bestX = 0.0f, bestY = 0.0f;
    int bestL = -1;
    for (int l = G.min_level; l < G.max_level; l++) { /* every condition below is workgroup-uniform */
        const FgLevel lg = G.lv[l];
        const int cwl = G.cw >> l, chl = G.ch >> l;
        if (cwl < 1 || chl < 1) break;
        const int x0 = cwl * cx, y0 = chl * cy;
        if (!Pol::searchable(lg, D) || x0 >= lg.w || y0 >= lg.h) continue;
        const uint8_t* img = pyr + lg.base + (size_t)slot * lg.bytes;
        const int WP = cwl + 8, WH = chl + 2 * RA, RP = cwl + 2, RH = chl + 2;
        uint8_t* win = gdsm;
        float* respS = (float*)(gdsm + gd_win_bytes(cwl, chl, RA));
        const GdTile t = {lg, img, x0, y0, cwl, chl, WP, WH, RP, RH, win, respS, (uint8_t*)(respS + RP * RH)};
        /* window origin x0 - 4 is a multiple of 4 (cell widths are), rows are 64-byte aligned: aligned dwords.
         * The dword and row indices are merely clamped into the allocation: a policy that uses bytes outside the
         * image puts them right in finish_window. */
        if (cwl >= 4) {
            const int WD = WP >> 2, maxd = (lg.pitch >> 2) - 1, d0 = (x0 - 4) >> 2; /* arithmetic shift: -1 for x0 = 0 */
            const uint32_t mD = ((1u << 20) + WD - 1) / WD; /* i / WD == (i * mD) >> 20 for i < 2^20 / WD */
            for (int i = tid; i < WD * WH; i += NT) {
                /* 24-bit multiply-adds throughout (i < 2^20, the magic numbers < 2^21, rows and pitches < 2^24): one
                 * instruction where the 32-bit / size_t forms take a multiply plus adds or a 64-bit chain */
                const int wy = (int)(mad24u((uint32_t)i, mD, 0u) >> 20), wd = i - (int)mad24u((uint32_t)wy, (uint32_t)WD, 0u);
                const int gy = min(max(y0 - RA + wy, 0), lg.h - 1), gd = min(max(d0 + wd, 0), maxd);
                ((uint32_t*)win)[i] = *(const uint32_t*)(img + mad24u((uint32_t)gy, (uint32_t)lg.pitch, 4u * (uint32_t)gd));
            }
        } else { /* 1- and 2-pixel cells of very coarse levels; the address as above */
            for (int i = tid; i < WP * WH; i += NT) {
                const int wy = i / WP, wx = i - wy * WP;
                const int gx = min(max(x0 - 4 + wx, 0), lg.w - 1), gy = min(max(y0 - RA + wy, 0), lg.h - 1);
                win[i] = img[mad24u((uint32_t)gy, (uint32_t)lg.pitch, (uint32_t)gx)];
            }
        }
        Pol::template finish_window<NT>(t, D, tid);
        if (tid == 0) s_best = 0ull;
        __syncthreads();
        Pol::template response<NT>(t, D, tid);
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
                const uint32_t t5 = (uint32_t)(px + bdx * ty);
                prio = ((t5 >> 5) << 17) | (gd_brev5(t5 & 31u) << 12) | (uint32_t)py;
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
                const uint32_t t5 = ((prio >> 17) << 5) | gd_brev5((prio >> 12) & 31u);
                px = (int)(t5 % (uint32_t)bdx);
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
/* Fills lv[0 .. levels) for max_batch images of w x h (level sizes are original >> l, pyramid_pool.cpp:61-62; pitches
 * are multiples of 64 with at least 8 bytes behind a row) and returns the bytes to allocate. */
size_t fg_pyramid_layout(FgLevel* lv, int w, int h, int levels, int max_batch);
/* n device images of pitch src_pitch -> level 0 (k_fg_gather) */
void fg_pyramid_gather(hipStream_t st, const uint8_t* const* imgs, int n, size_t src_pitch, uint8_t* pyr, const FgLevel& L0);
/* level l - 1 -> level l for l = 1 .. levels - 1 of n images (k_fg_halfsample, one launch per level) */
void fg_pyramid_halfsample(hipStream_t st, uint8_t* pyr, const FgLevel* lv, int levels, int n);

struct GdHost { /* vslam_fg and vslam_hg derive from this */
    GdGeom G;
    int device = 0, max_batch = 0, cells = 0, last_n = 0;
    size_t pyr_bytes = 0;
    hipStream_t stream = nullptr;
    vslam_dbuf<uint8_t> d_pyr, d_grid;
    vslam_hbuf<uint8_t> h_img, h_grid;
    vslam_dbuf<float> d_resp;
    const uint8_t* search_pyr = nullptr; /* view: the pyramid the launch searches -- d_pyr, or a caller's in this layout (gd_detect_pyramid) */
    void (*launch)(const GdHost*, int n, float* resp_out, int resp_level, int resp_slot) = nullptr; /* the detect kernel */
};

/* the parameters every vslam_*_params has; own_ok: the detector's checks of the rest.  fn names the caller in g_err */
template <class P>
int gd_validate(const P& p, bool own_ok, const char* fn) {
    if (p.image_width < 16 || p.image_height < 16 || p.image_width > 16384 || p.image_height > 16384 ||
        (p.cell_size_width != 32 && p.cell_size_width != GD_MAX_CELL) || (p.cell_size_height != 32 && p.cell_size_height != GD_MAX_CELL) ||
        p.min_level < 0 || p.max_level <= p.min_level || p.max_level > FG_MAX_LEVELS || p.horizontal_border < 0 ||
        p.vertical_border < 0 || p.tie_rule < 0 || p.tie_rule > 1 || p.max_batch < 1 || p.max_batch > FG_MAX_BATCH || !own_ok) {
        g_err = std::string(fn) + ": unsupported parameters";
        return VSLAM_ERR_INVALID;
    }
    /* the reference's own assertions: pyramid_pool.cpp:58-59, detector_base_gpu.cpp:62 */
    if ((p.image_width % (1 << (p.max_level - 1))) || (p.image_height % (1 << (p.max_level - 1))) ||
        (p.cell_size_height % (1 << (p.max_level - 1)))) {
        g_err = std::string(fn) + ": image and cell sizes must be divisible by 2^(max_level-1)";
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}
/* geometry and pyramid layout from validated parameters; min_border: the detector's smallest hb, vb */
template <class P>
void gd_fill(GdHost& h, const P& p, int min_border) {
    GdGeom& G = h.G;
    memset(&G, 0, sizeof(G));
    G.cw = p.cell_size_width;
    G.ch = p.cell_size_height;
    G.n_cols = (p.image_width + G.cw - 1) / G.cw; /* detector_base.cpp:54-55 */
    G.n_rows = (p.image_height + G.ch - 1) / G.ch;
    G.min_level = p.min_level;
    G.max_level = p.max_level;
    G.hb = std::max(min_border, p.horizontal_border);
    G.vb = std::max(min_border, p.vertical_border);
    G.tie = p.tie_rule;
    h.device = p.device;
    h.max_batch = p.max_batch;
    h.cells = G.n_cols * G.n_rows;
    h.pyr_bytes = fg_pyramid_layout(G.lv, p.image_width, p.image_height, G.max_level, p.max_batch);
}
int gd_alloc(GdHost& h); /* stream and buffers; on failure the caller destroys the object */
void gd_free(GdHost& h); /* waits for the stream and destroys it; the buffers go with the object */
int gd_grid(const GdHost* h, int* n_cols, int* n_rows);
/* upload or gather, halfsample, launch, grid copy, unpack into pos / score / level */
int gd_detect_batch(GdHost* h, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos, float* score,
                    int32_t* level);
/* The two halves of gd_detect_batch, for a caller that brings a pyramid of its own in h's layout (the feature tracker,
 * whose pyramid has more levels): n images -> level 0 of pyr, and the bound detector's launch, grid copy and unpacking
 * on an already built pyramid.  Both work on h's stream; the second waits for it. */
void gd_stage_images(GdHost* h, int n, const uint8_t* const* imgs, size_t pitch, int on_device, uint8_t* pyr);
int gd_detect_pyramid(GdHost* h, int n, uint8_t* pyr, float* pos, float* score, int32_t* level);
int gd_level_copy(GdHost* h, int slot, int level, uint8_t* dst, size_t dst_pitch, int* w, int* h_out);
int gd_response_copy(GdHost* h, int slot, int level, float* dst);
int gd_nt(); /* threads per cell, see vk_fast_cells_v3; VSLAM_FG_NT = 64 | 128 | 256 for A/B runs, for both detectors */

/* GdHost::launch of a detector: k64, k128, k256 are its kernel for the three values of gd_nt() */
template <class Pol, class K>
void gd_launch(const GdHost& h, K* k64, K* k128, K* k256, const typename Pol::Params& D, int n, float* resp_out, int resp_level,
               int resp_slot) {
    const int nt = gd_nt();
    hipLaunchKernelGGL(nt == 64 ? k64 : nt == 128 ? k128 : k256, dim3(((h.cells + 7) / 8) * 8, n), dim3(nt), gd_lds_bytes<Pol>(h.G),
                       h.stream, h.search_pyr, h.G, D, h.d_grid, resp_out, resp_level, resp_slot);
}

#endif
