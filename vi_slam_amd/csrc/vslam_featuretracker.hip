/* vslam_featuretracker.hip -- the pyramidal Lucas-Kanade feature tracker, vilib::FeatureTrackerGPU
 * (include/vslam_featuretracker.h): the two kernels, the per-frame sequence and the C ABI.  The bookkeeping (track list,
 * buffer ids, feature list, occupancy, best-N) is vslam_ftbook.cpp's vslam_ftbook; pyramid and detector: vslam_griddet.h.
 *
 * What the reference runs (CUDA, warp = 32, thirdparty/vilib/visual_lib/src/feature_tracker/feature_tracker_cuda_tools.cu):
 *   K10 update_tracks_kernel    :624-690  3 candidates per block; the int template patches with a 1-px rim and the inverse of
 *                                         the 2x2 / 3x3 / 4x4 Gauss-Newton Hessian per level (load_ref_patch, calc_hessian)
 *   K11 track_features_kernel   :189-304  2 candidates per block; inverse-compositional LK from the coarsest level down
 *                                         (perform_lk), at most 30 iterations per level
 *   over track metadata in mapped host memory (feature_tracker_gpu.cpp:418-470).
 * What runs here:
 *   k_ft_update<offset, gain, bundle>, k_ft_track<offset, gain, bundle>: one wave64 per workgroup, one candidate per
 *     32-lane half.  The two halves diverge in level, iteration count and exit -- and, in a bundle, in the camera --; every
 *     cross-lane read stays inside its half (__shfl_xor and __shfl_down with width 32), and all 32 lanes of a half are
 *     uniform in control flow by construction: the reduced Jres is the same word in every lane of the half, and
 *     everything else that steers a branch is per candidate.
 *   A tracker object serves C cameras (a FrameBundle) that share the detector, its stream and the options.  Each step of
 *     the reference's track() runs once for the bundle: one pyramid build over C image slots, one k_ft_track launch over
 *     the cameras' live tracks one camera after the other, one result copy, one detector launch over the slots [0, hi),
 *     one upload, one k_ft_update launch.  A candidate is one word (FT_CAND_*): its camera slot and its buffer id within
 *     that camera's block of max_ftr buffers; the image of slot s on a level is base + s * bytes.
 *   Track metadata lives in HBM (64 bytes per buffer id, the reference's layout).  Per call there is one upload -- the
 *     candidate words of both kernels and the positions of the new tracks; k_ft_update initialises their metadata -- and
 *     one result copy (cur_px, disparity per candidate).  Whether kernels that read and write pinned host memory
 *     directly, as the reference's do, would be faster is unmeasured.
 *   Templates are int32 in the reference's layout (max_area per level, max_level first), so vslam_ft_template_copy is a
 *     plain copy.  k_ft_update sums the Hessian from the image bytes it has just copied rather than from the patch in
 *     global memory: the same integers, and no store-to-load round trip inside a wave.
 * Arithmetic: every float operation is rounded on its own, left to right as the reference's C expressions read (the
 * library builds with -ffp-contract=off; the intrinsics say so again).  Lane t owns patch pixels i*32 + t in raster order
 * and adds them in ascending i; Jres goes through the xor butterfly 16, 8, 4, 2, 1, H through the shift-down tree with the
 * same offsets, lane 0 of the half inverts.  1.0f / det is __fdiv_rn, sqrtf the correctly rounded one (see k_hg_detect).
 */
#include "../../include/vslam_featuretracker.h"
#include "vslam_griddet.h"

/* floats per buffer id (METADATA_ELEMENT_BYTES 64): cur_f[4] | template_px | first_px | cur_px | alpha_beta | disparity | pad */
#define FT_META 16
enum { FT_TEMPLATE = 4, FT_FIRST = 6, FT_CUR = 8, FT_AB = 10, FT_DISP = 12 };
#define FT_NAN 0x7fffffffu
/* BUNDLE: the object has more than one camera.  With one, the slot is the constant 0 and the kernels are, register for
 * register, the single-camera kernels they were; with the slot a per-candidate value, two of the four k_ft_track and one
 * of the k_ft_update variants would give up a wave of occupancy, which a single camera need not pay.
 * A candidate word: bits 0-19 the buffer id within its camera (vslam_ftbook_create caps max_ftr at 2^20), bits 20-25 the
 * camera slot (FG_MAX_BATCH = 64), bit 31 (k_ft_update only) a new track, whose position is newpx[candidate]. */
#define FT_CAND_ID 0xFFFFFu
#define FT_CAND_SLOT_SHIFT 20
#define FT_CAND_SLOT 63u
#define FT_CAND_NEW 0x80000000u
static_assert(FG_MAX_BATCH - 1 <= FT_CAND_SLOT, "a candidate word has six bits for the camera slot");

struct FtGeom {
    FgLevel lv[FG_MAX_LEVELS];
    int32_t ps[FG_MAX_LEVELS];
    int32_t min_level, max_level, max_area, nlev;
    float min_update_squared;
    int32_t max_ftr; /* buffers per camera: camera s owns buffers s * max_ftr .. */
};

/* int u = floorf(v): the conversion saturates, as CUDA's does.  A clamped value fails every bounds test below just as
 * INT_MIN and INT_MAX do; the tests are written so that they cannot overflow. */
__device__ __forceinline__ int ft_floor_int(float v) { return (int)fminf(fmaxf(floorf(v), -2147483648.0f), 2147483520.0f); }

__device__ __forceinline__ float ft_mac(float acc, float a, float b) { return __fadd_rn(acc, __fmul_rn(a, b)); } /* acc += a * b */

/* lane 0 of calc_hessian (:583-620): the closed-form inverse of the symmetric matrix whose upper triangle is H, row-major.
 * A product is taken left to right (a leading 2 first), the terms are summed left to right.  Term for term the tables
 * DET4 / INV4 / DET3 / INV3 / DET2 of tests/lk_ref.py. */
#define P2(a, b) __fmul_rn(H[a], H[b])
#define P3(a, b, c) __fmul_rn(P2(a, b), H[c])
#define P4(a, b, c, d) __fmul_rn(P3(a, b, c), H[d])
#define D3(a, b, c) __fmul_rn(__fmul_rn(__fmul_rn(2.0f, H[a]), H[b]), H[c])
#define D4(a, b, c, d) __fmul_rn(D3(a, b, c), H[d])
#define ADD(x) s = __fadd_rn(s, x)
#define SUB(x) s = __fsub_rn(s, x)
template <bool OFF, bool GAIN>
__device__ __forceinline__ void ft_invert(const float* H, float* o) {
    float s;
    if (OFF && GAIN) {
        s = P4(0,4,7,9); ADD(D4(0,5,6,8)); ADD(P4(1,1,8,8)); ADD(D4(1,2,5,9)); ADD(D4(1,3,6,7)); ADD(D4(2,3,4,8));
        ADD(P4(2,2,6,6)); ADD(P4(3,3,5,5)); SUB(P4(0,4,8,8)); SUB(P4(0,5,5,9)); SUB(P4(0,6,6,7)); SUB(P4(1,1,7,9));
        SUB(D4(1,3,5,8)); SUB(D4(1,2,6,8)); SUB(P4(2,2,4,9)); SUB(D4(2,3,5,6)); SUB(P4(3,3,4,7));
        const float inv = __fdiv_rn(1.0f, s);
        s = P3(4,7,9); ADD(D3(5,6,8)); SUB(P3(4,8,8)); SUB(P3(5,5,9)); SUB(P3(6,6,7)); o[0] = __fmul_rn(s, inv);
        s = P3(1,8,8); ADD(P3(2,5,9)); ADD(P3(3,6,7)); SUB(P3(1,7,9)); SUB(P3(2,6,8)); SUB(P3(3,5,8));
        o[1] = __fmul_rn(s, inv);
        s = P3(1,5,9); ADD(P3(2,6,6)); ADD(P3(3,4,8)); SUB(P3(1,6,8)); SUB(P3(2,4,9)); SUB(P3(3,5,6));
        o[2] = __fmul_rn(s, inv);
        s = P3(1,6,7); ADD(P3(2,4,8)); ADD(P3(3,5,5)); SUB(P3(1,5,8)); SUB(P3(2,6,5)); SUB(P3(3,4,7));
        o[3] = __fmul_rn(s, inv);
        s = P3(0,7,9); ADD(D3(2,3,8)); SUB(P3(0,8,8)); SUB(P3(2,2,9)); SUB(P3(3,3,7)); o[4] = __fmul_rn(s, inv);
        s = P3(0,6,8); ADD(P3(1,2,9)); ADD(P3(3,3,5)); SUB(P3(0,5,9)); SUB(P3(2,3,6)); SUB(P3(1,3,8));
        o[5] = __fmul_rn(s, inv);
        s = P3(0,5,8); ADD(P3(2,2,6)); ADD(P3(1,3,7)); SUB(P3(0,6,7)); SUB(P3(1,2,8)); SUB(P3(2,3,5));
        o[6] = __fmul_rn(s, inv);
        s = P3(0,4,9); ADD(D3(1,3,6)); SUB(P3(0,6,6)); SUB(P3(1,1,9)); SUB(P3(3,3,4)); o[7] = __fmul_rn(s, inv);
        s = P3(0,5,6); ADD(P3(1,1,8)); ADD(P3(2,3,4)); SUB(P3(0,4,8)); SUB(P3(1,2,6)); SUB(P3(1,3,5));
        o[8] = __fmul_rn(s, inv);
        s = P3(0,4,7); ADD(D3(1,2,5)); SUB(P3(0,5,5)); SUB(P3(1,1,7)); SUB(P3(2,2,4)); o[9] = __fmul_rn(s, inv);
    } else if (OFF || GAIN) {
        s = P3(0,3,5); ADD(D3(1,4,2)); SUB(P3(0,4,4)); SUB(P3(2,3,2)); SUB(P3(1,1,5));
        const float inv = __fdiv_rn(1.0f, s);
        s = P2(3,5); SUB(P2(4,4)); o[0] = __fmul_rn(s, inv);
        s = P2(2,4); SUB(P2(1,5)); o[1] = __fmul_rn(s, inv);
        s = P2(1,4); SUB(P2(2,3)); o[2] = __fmul_rn(s, inv);
        s = P2(0,5); SUB(P2(2,2)); o[3] = __fmul_rn(s, inv);
        s = P2(1,2); SUB(P2(0,4)); o[4] = __fmul_rn(s, inv);
        s = P2(0,3); SUB(P2(1,1)); o[5] = __fmul_rn(s, inv);
    } else {
        s = P2(0,2); SUB(P2(1,1));
        const float inv = __fdiv_rn(1.0f, s);
        o[0] = __fmul_rn(H[2], inv);
        o[1] = __fmul_rn(__fmul_rn(-1.0f, H[1]), inv);
        o[2] = __fmul_rn(H[0], inv);
    }
}
#undef P2
#undef P3
#undef P4
#undef D3
#undef D4
#undef ADD
#undef SUB

template <bool OFF, bool GAIN>
struct FtDim { /* parameters of the update, entries of the symmetric Hessian */
    static constexpr int NP = (OFF && GAIN) ? 4 : (OFF || GAIN) ? 3 : 2;
    static constexpr int NH = NP * (NP + 1) / 2;
};

/* K10.  Candidates 0 .. n-1 are cand[0 .. n), every camera's "last n" tracks one camera after the other.  A word with
 * FT_CAND_NEW is a new track whose metadata is set up here from newpx[candidate], the others
 * (klt_template_is_first_observation == false) take their converged position as the new template. */
template <bool OFF, bool GAIN, bool BUNDLE>
__global__ void __launch_bounds__(64)
k_ft_update(int n, const uint32_t* __restrict__ cand, const float2* __restrict__ newpx, const uint8_t* __restrict__ pyr, FtGeom G,
            float* __restrict__ meta, int32_t* __restrict__ patches, float* __restrict__ invh) {
    constexpr int NH = FtDim<OFF, GAIN>::NH;
    const int t = threadIdx.x & 31, cx = blockIdx.x * 2 + (threadIdx.x >> 5);
    if (cx >= n) return; /* an idle half */
    const uint32_t cw = cand[cx];
    const int slot = BUNDLE ? (int)((cw >> FT_CAND_SLOT_SHIFT) & FT_CAND_SLOT) : 0, bx = slot * G.max_ftr + (int)(cw & FT_CAND_ID);
    float* m = meta + (size_t)bx * FT_META;
    float2 ref;
    if (cw & FT_CAND_NEW) { /* addTrack, feature_tracker_gpu.cpp:338-350 */
        ref = newpx[cx];
        if (t == 0) {
            m[FT_TEMPLATE] = m[FT_FIRST] = m[FT_CUR] = ref.x;
            m[FT_TEMPLATE + 1] = m[FT_FIRST + 1] = m[FT_CUR + 1] = ref.y;
            m[FT_AB] = m[FT_AB + 1] = m[FT_DISP] = 0.0f;
        }
    } else { /* :166-172 */
        ref = make_float2(m[FT_CUR], m[FT_CUR + 1]);
        if (t == 0) {
            m[FT_TEMPLATE] = ref.x;
            m[FT_TEMPLATE + 1] = ref.y;
        }
    }
    int32_t* pb = patches + (size_t)bx * G.nlev * G.max_area;
    float* hb = invh + (size_t)bx * G.nlev * 10;
    for (int level = G.max_level; level >= G.min_level; --level, pb += G.max_area, hb += 10) {
        const float inv_scale = __fdiv_rn(1.0f, (float)(1 << level));
        const FgLevel lg = G.lv[level];
        const int ps = G.ps[level], half = ps >> 1, stride = ps + 2;
        /* load_ref_patch (:405-465), REFERENCE_PATCH_INTERPOLATION 0 */
        const int x_tl = ft_floor_int(__fsub_rn(__fmul_rn(ref.x, inv_scale), (float)(half + 1)));
        const int y_tl = ft_floor_int(__fsub_rn(__fmul_rn(ref.y, inv_scale), (float)(half + 1)));
        if (x_tl < 0 || y_tl < 0 || x_tl >= lg.w - ps - 1 || y_tl >= lg.h - ps - 1) { /* (x_tl + ps + 1) >= w, without the sum */
            if (t == 0) hb[0] = __uint_as_float(FT_NAN);
            continue;
        }
        /* image `slot` of the level starts slot * bytes = slot * h rows behind the level's base (fg_pyramid_layout) */
        const uint8_t* tl = pyr + lg.base + (size_t)(slot * lg.h + y_tl) * lg.pitch + x_tl;
        for (int id = t; id < stride * stride; id += 32) {
            const int yy = id / stride, xx = id - yy * stride;
            pb[id] = (int32_t)tl[yy * lg.pitch + xx];
        }
        /* calc_hessian (:468-581) */
        const int sh = 31 - __clz(ps), rstep = 32 >> sh, ppt = (ps * ps) >> 5;
        const uint8_t* c = tl + ((t >> sh) + 1) * lg.pitch + (t & (ps - 1)) + 1;
        float H[NH];
#pragma unroll
        for (int k = 0; k < NH; k++) H[k] = 0.0f;
        for (int i = 0; i < ppt; i++, c += rstep * lg.pitch) {
            const float J0 = __fmul_rn(0.5f, (float)((int)c[1] - (int)c[-1]));
            const float J1 = __fmul_rn(0.5f, (float)((int)c[lg.pitch] - (int)c[-lg.pitch]));
            const float v = (float)c[0];
            if (OFF && GAIN) {
                H[0] = ft_mac(H[0], J0, J0);
                H[1] = ft_mac(H[1], J0, J1);
                H[2] = ft_mac(H[2], J0, 1.0f);
                H[3] = ft_mac(H[3], J0, v);
                H[4] = ft_mac(H[4], J1, J1);
                H[5] = ft_mac(H[5], J1, 1.0f);
                H[6] = ft_mac(H[6], J1, v);
                H[7] = ft_mac(H[7], 1.0f, 1.0f);
                H[8] = ft_mac(H[8], 1.0f, v);
                H[9] = ft_mac(H[9], v, v);
            } else if (OFF || GAIN) {
                const float J2 = OFF ? 1.0f : v;
                H[0] = ft_mac(H[0], J0, J0);
                H[1] = ft_mac(H[1], J0, J1);
                H[2] = ft_mac(H[2], J0, J2);
                H[3] = ft_mac(H[3], J1, J1);
                H[4] = ft_mac(H[4], J1, J2);
                H[5] = ft_mac(H[5], J2, J2);
            } else {
                H[0] = ft_mac(H[0], J0, J0);
                H[1] = ft_mac(H[1], J0, J1);
                H[2] = ft_mac(H[2], J1, J1);
            }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) /* down to lane 0 of the half; a lane whose partner is outside it adds itself, as in CUDA */
#pragma unroll
            for (int k = 0; k < NH; k++) H[k] = __fadd_rn(H[k], __shfl_down(H[k], o, 32));
        if (t == 0) {
            float o[NH];
            ft_invert<OFF, GAIN>(H, o);
#pragma unroll
            for (int k = 0; k < NH; k++) hb[k] = o[k];
        }
    }
}

/* K11.  result[cx] = (cur_px, disparity) of candidate cx, or the NaN word twice where it did not converge. */
template <bool OFF, bool GAIN, bool BUNDLE>
__global__ void __launch_bounds__(64)
k_ft_track(int n, const uint32_t* __restrict__ cand, const uint8_t* __restrict__ pyr, FtGeom G, float* __restrict__ meta,
           const int32_t* __restrict__ patches, const float* __restrict__ invh, float4* __restrict__ result) {
    constexpr int NP = FtDim<OFF, GAIN>::NP, NH = FtDim<OFF, GAIN>::NH;
    const int t = threadIdx.x & 31, cx = blockIdx.x * 2 + (threadIdx.x >> 5);
    if (cx >= n) return; /* an idle half */
    const uint32_t cw = cand[cx];
    const int slot = BUNDLE ? (int)((cw >> FT_CAND_SLOT_SHIFT) & FT_CAND_SLOT) : 0;
    const int bx = BUNDLE ? slot * G.max_ftr + (int)(cw & FT_CAND_ID) : (int)cw; /* one camera: the word is the buffer id */
    float* m = meta + (size_t)bx * FT_META;
    const int32_t* pb = patches + (size_t)bx * G.nlev * G.max_area;
    const float* hb = invh + (size_t)bx * G.nlev * 10;
    bool converged = false, go_to_next_level = true;
    float x = m[FT_CUR], y = m[FT_CUR + 1], alpha = m[FT_AB], beta = m[FT_AB + 1];
    float scale = 1.0f;
    for (int level = G.max_level; (converged || go_to_next_level) && level >= G.min_level;
         x = __fmul_rn(x, scale), y = __fmul_rn(y, scale), --level, pb += G.max_area, hb += 10) {
        scale = (float)(1 << level);
        const float inv_scale = __fdiv_rn(1.0f, scale);
        x = __fmul_rn(x, inv_scale);
        y = __fmul_rn(y, inv_scale);
        if (isnan(hb[0])) continue; /* no template on this level (:256-258) */
        /* perform_lk (:57-187) */
        converged = false;
        go_to_next_level = false;
        const FgLevel lg = G.lv[level];
        const int ps = G.ps[level], half = ps >> 1, stride = ps + 2;
        const int sh = 31 - __clz(ps), rstep = 32 >> sh, ppt = (ps * ps) >> 5;
        const int px = t & (ps - 1), py = t >> sh;
        const int32_t* ref0 = pb + (py + 1) * stride + px + 1;
        /* image `slot` of the level starts slot * bytes = slot * h rows behind the level's base (fg_pyramid_layout): the
         * lane's row within the patch, counted from the base */
        const uint8_t* img = pyr + lg.base;
        const int row0 = slot * lg.h + py;
        float iH[NH];
#pragma unroll
        for (int k = 0; k < NH; k++) iH[k] = hb[k];
        for (int iter = 0; iter < VSLAM_FT_MAX_ITER; ++iter) {
            if (isnan(x) || isnan(y)) break;
            const int u = ft_floor_int(x), v = ft_floor_int(y);
            if (u < half || v < half || u >= lg.w - half || v >= lg.h - half) {
                go_to_next_level = true;
                break;
            }
            /* rows v - half .. v + half and columns u - half .. u + half are inside the level from here on */
            const float sx = __fsub_rn(x, (float)u), sy = __fsub_rn(y, (float)v);
            const float wTL = __fmul_rn(__fsub_rn(1.0f, sx), __fsub_rn(1.0f, sy)), wTR = __fmul_rn(sx, __fsub_rn(1.0f, sy));
            const float wBL = __fmul_rn(__fsub_rn(1.0f, sx), sy), wBR = __fmul_rn(sx, sy);
            const float gain1 = __fadd_rn(1.0f, alpha);
            const uint8_t* it = img + (size_t)(v - half + row0) * lg.pitch + (u - half + px);
            const int32_t* r = ref0;
            float J[NP];
#pragma unroll
            for (int k = 0; k < NP; k++) J[k] = 0.0f;
            for (int i = 0; i < ppt; i++, it += rstep * lg.pitch, r += rstep * stride) {
                const float s = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(wTL, (float)it[0]), __fmul_rn(wTR, (float)it[1])),
                                                    __fmul_rn(wBL, (float)it[lg.pitch])), __fmul_rn(wBR, (float)it[lg.pitch + 1]));
                const float rv = (float)r[0];
                const float res = __fsub_rn(__fsub_rn(s, __fmul_rn(gain1, rv)), beta);
                const float hres = __fmul_rn(res, 0.5f);
                J[0] = ft_mac(J[0], hres, (float)(r[1] - r[-1]));
                J[1] = ft_mac(J[1], hres, (float)(r[stride] - r[-stride]));
                if (OFF && GAIN) {
                    J[2] = __fadd_rn(J[2], res);
                    J[3] = ft_mac(J[3], res, rv);
                } else if (OFF) {
                    J[2] = __fadd_rn(J[2], res);
                } else if (GAIN) {
                    J[2] = ft_mac(J[2], res, rv);
                }
            }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) /* the xor butterfly: afterwards every lane of the half holds the same words */
#pragma unroll
                for (int k = 0; k < NP; k++) J[k] = __fadd_rn(J[k], __shfl_xor(J[k], o, 32));
            float up[NP];
            if (OFF && GAIN) {
                up[0] = ft_mac(ft_mac(ft_mac(__fmul_rn(iH[0], J[0]), iH[1], J[1]), iH[2], J[2]), iH[3], J[3]);
                up[1] = ft_mac(ft_mac(ft_mac(__fmul_rn(iH[1], J[0]), iH[4], J[1]), iH[5], J[2]), iH[6], J[3]);
                up[2] = ft_mac(ft_mac(ft_mac(__fmul_rn(iH[2], J[0]), iH[5], J[1]), iH[7], J[2]), iH[8], J[3]);
                up[3] = ft_mac(ft_mac(ft_mac(__fmul_rn(iH[3], J[0]), iH[6], J[1]), iH[8], J[2]), iH[9], J[3]);
            } else if (OFF || GAIN) {
                up[0] = ft_mac(ft_mac(__fmul_rn(iH[0], J[0]), iH[1], J[1]), iH[2], J[2]);
                up[1] = ft_mac(ft_mac(__fmul_rn(iH[1], J[0]), iH[3], J[1]), iH[4], J[2]);
                up[2] = ft_mac(ft_mac(__fmul_rn(iH[2], J[0]), iH[4], J[1]), iH[5], J[2]);
            } else {
                up[0] = ft_mac(__fmul_rn(iH[0], J[0]), iH[1], J[1]);
                up[1] = ft_mac(__fmul_rn(iH[1], J[0]), iH[2], J[1]);
            }
            x = __fsub_rn(x, up[0]);
            y = __fsub_rn(y, up[1]);
            if (OFF && GAIN) {
                alpha = __fadd_rn(alpha, up[3]);
                beta = __fadd_rn(beta, up[2]);
            } else if (OFF) {
                beta = __fadd_rn(beta, up[2]);
            } else if (GAIN) {
                alpha = __fadd_rn(alpha, up[2]);
            }
            if (__fadd_rn(__fmul_rn(up[0], up[0]), __fmul_rn(up[1], up[1])) < G.min_update_squared) {
                converged = true;
                break;
            }
        }
    }
    if (t == 0) {
        if (converged) {
            const float dx = __fsub_rn(x, m[FT_FIRST]), dy = __fsub_rn(y, m[FT_FIRST + 1]);
            const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            m[FT_CUR] = x;
            m[FT_CUR + 1] = y;
            if (GAIN) m[FT_AB] = alpha;
            if (OFF) m[FT_AB + 1] = beta;
            m[FT_DISP] = d;
            result[cx] = make_float4(x, y, d, 0.0f);
        } else {
            m[FT_CUR] = m[FT_CUR + 1] = __uint_as_float(FT_NAN);
            result[cx] = make_float4(__uint_as_float(FT_NAN), __uint_as_float(FT_NAN), 0.0f, 0.0f);
        }
    }
}

/* ---------------------------------------------------------------------------------------------- host */
struct vslam_ft {
    vslam_ft_params p;
    GdHost* det = nullptr;
    int n_cam = 0;
    std::vector<vslam_ftbook*> book; /* one per camera; the track-id counter is threaded through them (next_id) */
    int next_id = 0;
    FtGeom G;
    int max_ftr = 0; /* per camera */
    size_t cap = 0;  /* n_cam * max_ftr: candidates, buffers */
    size_t pyr_bytes = 0;
    /* stage, packed anew in every call so that it goes up as one range: float2 newpx[n_upd] (per entry of ucand) |
     * uint32 cand[n] (the next call's k_ft_track; cand_off bytes in) | uint32 ucand[n_upd] (k_ft_update); n, n_upd <= cap */
    vslam_dbuf<uint8_t> d_pyr, d_stage;
    vslam_hbuf<uint8_t> h_stage;
    size_t cand_off = 0;
    vslam_dbuf<float> d_meta, d_invh;
    vslam_hbuf<float> h_res;
    vslam_dbuf<float4> d_res;
    vslam_dbuf<int32_t> d_patch;
    std::vector<float> pos, score; /* the detector's grids of slots 0 .. n_cam - 1 */
    std::vector<int32_t> level;
    std::vector<vslam_ft_track_info> info;
    std::vector<int32_t> n_live, tracked, detected; /* per camera, within a call */
    vslam_event ev[4]; /* vslam_ft_profile: around k_ft_track, around k_ft_update */
    bool profile = false, ran_track = false, ran_update = false;
};

template <class K>
static K* ft_pick(const vslam_ft* ft, K* k00, K* k10, K* k01, K* k11) {
    return ft->p.affine_est_offset ? (ft->p.affine_est_gain ? k11 : k10) : (ft->p.affine_est_gain ? k01 : k00);
}
#define FT_KERNEL(ft, k) \
    ((ft)->n_cam > 1 ? ft_pick(ft, k<false, false, true>, k<true, false, true>, k<false, true, true>, k<true, true, true>) \
                     : ft_pick(ft, k<false, false, false>, k<true, false, false>, k<false, true, false>, k<true, true, false>))

extern "C" void vslam_ft_destroy(vslam_ft* ft) {
    if (!ft) return;
    if (ft->det) {
        (void)hipSetDevice(ft->det->device);
        if (ft->det->stream) (void)hipStreamSynchronize(ft->det->stream);
    }
    for (vslam_ftbook* b : ft->book) vslam_ftbook_destroy(b);
    delete ft;
}

static int ft_alloc(vslam_ft* ft) {
    const size_t n = ft->cap;
    HIPCHK(hipSetDevice(ft->det->device));
    if (int rc = ft->d_pyr.alloc(ft->pyr_bytes)) return rc;
    HIPCHK(hipMemset(ft->d_pyr, 0, ft->pyr_bytes));
    if (int rc = ft->d_stage.alloc(n * 16)) return rc;
    if (int rc = ft->h_stage.alloc(n * 16)) return rc;
    memset(ft->h_stage, 0, n * 16);
    if (int rc = ft->d_meta.alloc(n * FT_META)) return rc;
    HIPCHK(hipMemset(ft->d_meta, 0, n * FT_META * 4));
    if (int rc = ft->d_patch.alloc(n * ft->G.nlev * ft->G.max_area)) return rc;
    HIPCHK(hipMemset(ft->d_patch, 0, n * ft->G.nlev * ft->G.max_area * 4));
    if (int rc = ft->d_invh.alloc(n * ft->G.nlev * 10)) return rc;
    HIPCHK(hipMemset(ft->d_invh, 0, n * ft->G.nlev * 40));
    if (int rc = ft->d_res.alloc(n)) return rc;
    if (int rc = ft->h_res.alloc(n * 4)) return rc;
    HIPCHK(hipDeviceSynchronize());
    return VSLAM_OK;
}

extern "C" int vslam_ft_create_bundle(const vslam_ft_params* p, int detector_kind, void* detector, int n_cameras, vslam_ft** out) {
    if (!p || !out || !detector || (detector_kind != VSLAM_FT_DETECTOR_FAST && detector_kind != VSLAM_FT_DETECTOR_HARRIS)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *out = nullptr;
    /* vslam_fg and vslam_hg derive from GdHost and from nothing else (vslam_fastgrid.hip, vslam_harrisgrid.hip), so either
     * handle is the address of its GdHost: the tracker needs no more of a detector than DetectorBaseGPU offers */
    GdHost* det = reinterpret_cast<GdHost*>(detector);
    if (n_cameras < 1 || n_cameras > det->max_batch) {
        g_err = "vslam_ft_create_bundle: 1 <= n_cameras <= the detector's max_batch";
        return VSLAM_ERR_INVALID;
    }
    const FgLevel& L0 = det->G.lv[0];
    bool ok = det->launch && p->klt_min_level >= 0 && p->klt_max_level > p->klt_min_level && p->klt_max_level < VSLAM_FT_MAX_LEVELS &&
              p->pyramid_levels >= p->klt_max_level + 1 && p->pyramid_levels >= det->G.max_level && p->pyramid_levels <= FG_MAX_LEVELS &&
              p->klt_min_update_squared == p->klt_min_update_squared && p->min_tracks_to_detect_new_features >= 0 &&
              p->use_best_n_features >= -1;
    int max_ps = 0;
    for (int l = p->klt_min_level; ok && l <= p->klt_max_level; l++) {
        const int s = p->klt_patch_sizes[l];
        ok = s == 8 || s == 16 || s == 32; /* 32 % size == 0 with at least one pixel per lane */
        max_ps = std::max(max_ps, s);
    }
    if (!ok) {
        g_err = "vslam_ft_create: unsupported parameters";
        return VSLAM_ERR_INVALID;
    }
    if ((L0.w % (1 << (p->pyramid_levels - 1))) || (L0.h % (1 << (p->pyramid_levels - 1)))) { /* pyramid_pool.cpp:58-59 */
        g_err = "vslam_ft_create: the image size must be divisible by 2^(pyramid_levels-1)";
        return VSLAM_ERR_INVALID;
    }
    vslam_ft* ft = new vslam_ft();
    ft->p = *p;
    ft->det = det;
    ft->n_cam = n_cameras;
    for (int c = 0; c < n_cameras; c++) {
        vslam_ftbook* b = nullptr;
        if (vslam_ftbook_create(p, det->G.n_cols, det->G.n_rows, det->G.cw, det->G.ch, &b) != 0) {
            vslam_ft_destroy(ft);
            g_err = "vslam_ft_create: min_tracks_to_detect_new_features and use_best_n_features leave no room for a track";
            return VSLAM_ERR_INVALID;
        }
        ft->book.push_back(b);
    }
    ft->max_ftr = vslam_ftbook_capacity(ft->book[0]); /* at most 2^20 (vslam_ftbook_create): FT_CAND_ID holds a buffer id */
    ft->cap = (size_t)ft->max_ftr * n_cameras;
    FtGeom& G = ft->G;
    memset(&G, 0, sizeof(G));
    /* the detector's level-major layout, continued: a level's base does not depend on how many levels follow, so the
     * detector's kernel finds its levels, and every image slot of them, in this pyramid where it finds them in its own */
    ft->pyr_bytes = fg_pyramid_layout(G.lv, L0.w, L0.h, p->pyramid_levels, det->max_batch);
    for (int l = 0; l < VSLAM_FT_MAX_LEVELS; l++) G.ps[l] = p->klt_patch_sizes[l];
    G.min_level = p->klt_min_level;
    G.max_level = p->klt_max_level;
    G.nlev = p->klt_max_level - p->klt_min_level + 1;
    G.max_area = (max_ps + 2) * (max_ps + 2); /* feature_tracker_gpu.cpp:68-76, over the levels in use */
    G.min_update_squared = p->klt_min_update_squared;
    G.max_ftr = ft->max_ftr;
    ft->pos.resize((size_t)det->cells * 2 * n_cameras);
    ft->score.resize((size_t)det->cells * n_cameras);
    ft->level.resize((size_t)det->cells * n_cameras);
    ft->info.resize((size_t)ft->max_ftr);
    ft->n_live.resize((size_t)n_cameras);
    ft->tracked.resize((size_t)n_cameras);
    ft->detected.resize((size_t)n_cameras);
    if (ft_alloc(ft) != VSLAM_OK) {
        vslam_ft_destroy(ft);
        return VSLAM_ERR_HIP;
    }
    *out = ft;
    return VSLAM_OK;
}

extern "C" int vslam_ft_create(const vslam_ft_params* p, int detector_kind, void* detector, vslam_ft** out) {
    return vslam_ft_create_bundle(p, detector_kind, detector, 1, out);
}

extern "C" int vslam_ft_capacity(const vslam_ft* ft) { return ft ? ft->max_ftr : -1; }
extern "C" int vslam_ft_cameras(const vslam_ft* ft) { return ft ? ft->n_cam : -1; }

extern "C" int vslam_ft_track_bundle(vslam_ft* ft, const uint8_t* const* imgs, size_t pitch, int on_device, int32_t* n_tracked,
                                     int32_t* n_detected) {
    if (!ft || !imgs || pitch < (size_t)ft->G.lv[0].w) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const int C = ft->n_cam;
    for (int c = 0; c < C; c++)
        if (!imgs[c]) {
            g_err = "null image";
            return VSLAM_ERR_INVALID;
        }
    GdHost* det = ft->det;
    HIPCHK(hipSetDevice(det->device));
    hipStream_t st = det->stream;
    /* 00) the bundle's pyramids, once for the tracker and the detector: camera c is image slot c of every level */
    gd_stage_images(det, C, imgs, pitch, on_device, ft->d_pyr);
    fg_pyramid_halfsample(st, ft->d_pyr, ft->G.lv, ft->p.pyramid_levels, C);
    /* 01) + 02) track what there is, one camera's tracks after the other's; the candidate words went up at the end of the
     * previous call */
    int n = 0;
    for (int c = 0; c < C; c++) {
        vslam_ftbook_tracks(ft->book[c], nullptr, 0, &ft->n_live[c]);
        n += ft->n_live[c];
    }
    ft->ran_track = n > 0;
    if (n > 0) {
        if (ft->profile) HIPCHK(hipEventRecord(ft->ev[0], st));
        hipLaunchKernelGGL(FT_KERNEL(ft, k_ft_track),
                           dim3((n + 1) / 2), dim3(64), 0, st, n, (const uint32_t*)(ft->d_stage + ft->cand_off), ft->d_pyr, ft->G, ft->d_meta, ft->d_patch,
                           ft->d_invh, ft->d_res);
        if (ft->profile) HIPCHK(hipEventRecord(ft->ev[1], st));
        vslam_copy_range(st, ft->h_res, ft->d_res, (size_t)n * 16);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    int hi = 0; /* one more than the highest camera that wants new features */
    for (int c = 0, at = 0; c < C; at += ft->n_live[c], c++) {
        vslam_ftbook_results(ft->book[c], ft->h_res + (size_t)at * 4, ft->n_live[c]);
        vslam_ftbook_tracks(ft->book[c], nullptr, 0, &ft->tracked[c]);
        ft->detected[c] = 0;
        if (vslam_ftbook_need_detect(ft->book[c])) hi = c + 1;
    }
    /* 03) detect on the same pyramids where too few tracks are left: one launch over the slots [0, hi).  Detection keeps
     * no state, so the grid of a camera below hi that did not ask is computed and not read.  Ids go camera by camera. */
    if (hi > 0) {
        const int rc = gd_detect_pyramid(det, hi, ft->d_pyr, ft->pos.data(), ft->score.data(), ft->level.data());
        if (rc != VSLAM_OK) return rc;
        const size_t cells = (size_t)det->cells;
        for (int c = 0; c < hi; c++) {
            vslam_ftbook* b = ft->book[c];
            if (!vslam_ftbook_need_detect(b)) continue;
            vslam_ftbook_set_next_id(b, ft->next_id);
            int d = 0;
            vslam_ftbook_detect(b, ft->pos.data() + cells * 2 * c, ft->score.data() + cells * c, ft->level.data() + cells * c, &d);
            ft->next_id = vslam_ftbook_next_id(b);
            ft->detected[c] = d;
            if (ft->p.reset_before_detection) ft->tracked[c] = 0;
        }
    }
    /* 04) one upload, one range: the positions of the update candidates that are new tracks, every track's candidate word
     * for the next call's k_ft_track, and the candidate words of every camera's last `last_n` tracks, which get templates */
    int n_upd = 0;
    n = 0;
    for (int c = 0; c < C; c++) {
        vslam_ftbook_tracks(ft->book[c], nullptr, 0, &ft->n_live[c]);
        n += ft->n_live[c];
        n_upd += std::min(ft->n_live[c], vslam_ftbook_update_count(ft->book[c]));
    }
    float* newpx = (float*)ft->h_stage;
    uint32_t *cand = (uint32_t*)ft->h_stage + 2 * (size_t)n_upd, *ucand = cand + n;
    ft->cand_off = 8 * (size_t)n_upd;
    for (int c = 0, at = 0, u = 0; c < C; at += ft->n_live[c], c++) {
        const int nc = ft->n_live[c], first_upd = nc - std::min(nc, vslam_ftbook_update_count(ft->book[c]));
        vslam_ftbook_tracks(ft->book[c], ft->info.data(), ft->max_ftr, nullptr);
        for (int i = 0; i < nc; i++) {
            const uint32_t w = ((uint32_t)c << FT_CAND_SLOT_SHIFT) | (uint32_t)ft->info[i].buffer_id;
            cand[at + i] = w;
            if (i < first_upd) continue;
            if (i >= nc - ft->detected[c]) { /* the new tracks are the last `detected` of the camera's list */
                ucand[u] = w | FT_CAND_NEW;
                newpx[2 * u] = ft->info[i].first_pos[0];
                newpx[2 * u + 1] = ft->info[i].first_pos[1];
            } else {
                ucand[u] = w;
            }
            u++;
        }
    }
    if (n > 0) vslam_copy_range(st, ft->d_stage, ft->h_stage, ((size_t)n + 3 * (size_t)n_upd) * 4);
    ft->ran_update = n_upd > 0;
    if (n_upd > 0) {
        if (ft->profile) HIPCHK(hipEventRecord(ft->ev[2], st));
        hipLaunchKernelGGL(FT_KERNEL(ft, k_ft_update),
                           dim3((n_upd + 1) / 2), dim3(64), 0, st, n_upd, (const uint32_t*)(ft->d_stage + ft->cand_off) + n,
                           (const float2*)ft->d_stage, ft->d_pyr, ft->G, ft->d_meta, ft->d_patch, ft->d_invh);
        if (ft->profile) HIPCHK(hipEventRecord(ft->ev[3], st));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st)); /* the staging blocks and the caller's images are free again */
    for (int c = 0; c < C; c++) {
        if (n_tracked) n_tracked[c] = ft->tracked[c];
        if (n_detected) n_detected[c] = ft->detected[c];
    }
    return VSLAM_OK;
}

extern "C" int vslam_ft_track(vslam_ft* ft, const uint8_t* img, size_t pitch, int on_device, int32_t* n_tracked, int32_t* n_detected) {
    if (!ft || !img || ft->n_cam != 1) {
        g_err = ft && ft->n_cam != 1 ? "vslam_ft_track: a bundle of several cameras takes vslam_ft_track_bundle" : "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const uint8_t* one[1] = {img};
    return vslam_ft_track_bundle(ft, one, pitch, on_device, n_tracked, n_detected);
}

extern "C" int vslam_ft_profile(vslam_ft* ft, int enable) {
    if (!ft) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(ft->det->device));
    for (vslam_event& e : ft->ev)
        if (enable)
            if (int rc = e.ensure()) return rc;
    ft->profile = enable != 0;
    ft->ran_track = ft->ran_update = false;
    return VSLAM_OK;
}

extern "C" int vslam_ft_kernel_ms(vslam_ft* ft, float* track_ms, float* update_ms) {
    if (!ft || !ft->profile || !track_ms || !update_ms) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    *track_ms = *update_ms = 0.0f;
    HIPCHK(hipSetDevice(ft->det->device));
    HIPCHK(hipStreamSynchronize(ft->det->stream));
    if (ft->ran_track) HIPCHK(hipEventElapsedTime(track_ms, ft->ev[0], ft->ev[1]));
    if (ft->ran_update) HIPCHK(hipEventElapsedTime(update_ms, ft->ev[2], ft->ev[3]));
    return VSLAM_OK;
}

static int ft_book_rc(int rc) {
    if (rc == 0) return VSLAM_OK;
    g_err = "invalid arguments";
    return VSLAM_ERR_INVALID;
}
static const vslam_ftbook* ft_book(const vslam_ft* ft, int camera) { /* nullptr, which every vslam_ftbook_* rejects */
    return ft && camera >= 0 && camera < ft->n_cam ? ft->book[camera] : nullptr;
}

extern "C" int vslam_ft_features_cam(const vslam_ft* ft, int camera, vslam_ft_feature* out, int cap, int* n) {
    return ft_book_rc(vslam_ftbook_features(ft_book(ft, camera), out, cap, n));
}
extern "C" int vslam_ft_tracks_cam(const vslam_ft* ft, int camera, vslam_ft_track_info* out, int cap, int* n) {
    return ft_book_rc(vslam_ftbook_tracks(ft_book(ft, camera), out, cap, n));
}
extern "C" int vslam_ft_disparity_cam(const vslam_ft* ft, int camera, double pivot_ratio, double* out) {
    return ft_book_rc(vslam_ftbook_disparity(ft_book(ft, camera), pivot_ratio, out));
}
extern "C" int vslam_ft_features(const vslam_ft* ft, vslam_ft_feature* out, int cap, int* n) { return vslam_ft_features_cam(ft, 0, out, cap, n); }
extern "C" int vslam_ft_tracks(const vslam_ft* ft, vslam_ft_track_info* out, int cap, int* n) { return vslam_ft_tracks_cam(ft, 0, out, cap, n); }
extern "C" int vslam_ft_disparity(const vslam_ft* ft, double pivot_ratio, double* out) { return vslam_ft_disparity_cam(ft, 0, pivot_ratio, out); }

/* the options are the bundle's: every camera's book gets the call; the first refusal is returned */
template <class F>
static int ft_all_books(vslam_ft* ft, F f) {
    int rc = ft ? 0 : -1;
    for (int c = 0; ft && c < ft->n_cam; c++)
        if (f(ft->book[c]) != 0) rc = -1;
    return ft_book_rc(rc);
}
extern "C" int vslam_ft_reset(vslam_ft* ft) { return ft_all_books(ft, [](vslam_ftbook* b) { return vslam_ftbook_reset(b); }); }
extern "C" int vslam_ft_set_best_n(vslam_ft* ft, int n) { return ft_all_books(ft, [n](vslam_ftbook* b) { return vslam_ftbook_set_best_n(b, n); }); }
extern "C" int vslam_ft_set_min_tracks(vslam_ft* ft, int n) { return ft_all_books(ft, [n](vslam_ftbook* b) { return vslam_ftbook_set_min_tracks(b, n); }); }

extern "C" int vslam_ft_template_copy_cam(vslam_ft* ft, int camera, int track, int level, int32_t* patch, float* invH) {
    int n = 0;
    const vslam_ftbook* b = ft_book(ft, camera);
    if (b) vslam_ftbook_tracks(b, ft->info.data(), ft->max_ftr, &n);
    if (!b || track < 0 || track >= n || level < ft->G.min_level || level > ft->G.max_level || (!patch && !invH)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const size_t buf = (size_t)camera * ft->max_ftr + (size_t)ft->info[track].buffer_id;
    const size_t slot = buf * ft->G.nlev + (size_t)(ft->G.max_level - level); /* max_level first */
    const int side = ft->G.ps[level] + 2;
    HIPCHK(hipSetDevice(ft->det->device));
    if (patch) HIPCHK(hipMemcpyAsync(patch, ft->d_patch + slot * ft->G.max_area, (size_t)side * side * 4, hipMemcpyDeviceToHost, ft->det->stream));
    if (invH) HIPCHK(hipMemcpyAsync(invH, ft->d_invh + slot * 10, 40, hipMemcpyDeviceToHost, ft->det->stream));
    HIPCHK(hipStreamSynchronize(ft->det->stream));
    return VSLAM_OK;
}
extern "C" int vslam_ft_template_copy(vslam_ft* ft, int track, int level, int32_t* patch, float* invH) {
    return vslam_ft_template_copy_cam(ft, 0, track, level, patch, invH);
}
