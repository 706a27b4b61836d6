/* vslam_harrisgrid.h -- C ABI of the grid Harris / Shi-Tomasi detector, vilib::HarrisGPU.
 *
 * Replaces, on MI355X (gfx950), vilib::HarrisGPU
 *   thirdparty/vilib/visual_lib/include/vilib/feature_detection/harris/harris_gpu.h
 *   thirdparty/vilib/visual_lib/src/feature_detection/harris/harris_gpu.cpp, harris_gpu_cuda_tools.cu
 *   thirdparty/vilib/visual_lib/src/preprocess/conv_filter.cpp, conv_filter_row.cu, conv_filter_col.cu
 * over vilib::DetectorBaseGPU (.../feature_detection/detector_base_gpu.cpp) on a vilib::Frame's half-sampled pyramid.
 * It is the sibling of the grid FAST detector (vslam_fastgrid.h): same pyramid, same suppression and cell arg-max
 * with the same tie rules, same feature-grid buffers; the corner response is the Harris or the Shi-Tomasi score of
 * the 3x3-averaged structure tensor of Sobel derivatives.  Every float operation is rounded on its own, in the
 * order in which the reference's source text reads (DESIGN.md section 8 lists what the reference leaves undefined).
 * Error codes and vslam_last_error() are those of vslam_fe.h.
 */
#ifndef VSLAM_HARRISGRID_H
#define VSLAM_HARRISGRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vilib::conv_filter_border_type (preprocess/conv_filter.h:59-72), in its order */
#define VSLAM_HG_BORDER_SKIP 0        /* filter with zeros outside, skip the outermost ring */
#define VSLAM_HG_BORDER_ZERO 1        /* 000000|abcdefgh|0000000 */
#define VSLAM_HG_BORDER_REPLICATE 2   /* aaaaaa|abcdefgh|hhhhhhh */
#define VSLAM_HG_BORDER_REFLECT 3     /* fedcba|abcdefgh|hgfedcb */
#define VSLAM_HG_BORDER_WRAP 4        /* cdefgh|abcdefgh|abcdefg */
#define VSLAM_HG_BORDER_REFLECT_101 5 /* gfedcb|abcdefgh|gfedcba */

/* The constructor arguments of vilib::HarrisGPU (harris_gpu.cpp:63-74) in their order, then ours. */
typedef struct vslam_hg_params {
    int32_t image_width, image_height;
    int32_t cell_size_width, cell_size_height;  /* 32 or 64 */
    int32_t min_level, max_level;               /* levels min_level <= l < max_level are searched; max_level <= 8 */
    int32_t horizontal_border, vertical_border; /* raised to 2 (3 for BORDER_SKIP) as the reference does, :58-59,:81-82 */
    int32_t filter_border_type;                 /* VSLAM_HG_BORDER_* */
    int32_t use_harris;                         /* != 0: Harris score, 0: Shi-Tomasi score */
    float harris_k;
    float quality_level;                        /* >= 0; a cell is kept iff score > max score * quality_level */
    int32_t tie_rule;                           /* 0: CUDA launch order, 1: raster (as in vslam_fastgrid.h) */
    int32_t device;
    int32_t max_batch;                          /* images per vslam_hg_detect_batch call, 1..64 */
} vslam_hg_params;

typedef struct vslam_hg vslam_hg;

int vslam_hg_create(const vslam_hg_params* p, vslam_hg** out);
void vslam_hg_destroy(vslam_hg* hg);
int vslam_hg_grid(const vslam_hg* hg, int* n_cols, int* n_rows);

/* vilib::Frame(image, 0, levels) + HarrisGPU::detect(frame->pyramid_) (harris_gpu.cpp:195-198).  pos / score / level
 * are the h_pos_ / h_score_ / h_level_ arrays of the feature grid as in vslam_fg_detect: n_cols*n_rows cells,
 * row-major, pos = (x, y) on level 0; cells without a corner carry pos (0, 0), score 0, level -1.
 * keep[cell] = (score > max over the grid's scores * quality_level), n_keep their count: what
 * processGridAndThreshold (detector_base_gpu.cpp:228-248) turns into feature points.  Both may be NULL, which is
 * the callback overload's raw grid (harris_gpu.cpp:200-207). */
int vslam_hg_detect(vslam_hg* hg, const uint8_t* img_host, size_t pitch, float* pos, float* score, int32_t* level,
                    uint8_t* keep, int32_t* n_keep);

/* n images of the same size in one pass; imgs[i] are host pointers, or device pointers when on_device != 0.
 * Outputs hold n consecutive grids; the maximum, keep (n * cells bytes) and n_keep (n counts) are per image. */
int vslam_hg_detect_batch(vslam_hg* hg, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos,
                          float* score, int32_t* level, uint8_t* keep, int32_t* n_keep);

/* A pyramid level of image `slot` of the last call (vilib::Subframe: width >> l, height >> l). */
int vslam_hg_level_copy(vslam_hg* hg, int slot, int level, uint8_t* dst, size_t dst_pitch, int* w, int* h);
/* DetectorBaseGPU::copyResponseTo: the corner response of a searched level, (width >> l) * (height >> l) floats,
 * recomputed for image `slot` of the last call.  Outside [m, w-1-m] x [m, h-1-m] (m = 2 for BORDER_SKIP, else 1),
 * where the reference never writes, it is 0. */
int vslam_hg_response_copy(vslam_hg* hg, int slot, int level, float* dst);

#ifdef __cplusplus
}
#endif
#endif
