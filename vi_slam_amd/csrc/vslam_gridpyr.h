/* vslam_gridpyr.h -- the half-sampled pyramid under the grid detectors (vilib::Frame over a PyramidPool:
 * thirdparty/vilib/visual_lib/src/common/frame.cpp:49-57, preprocess/pyramid_gpu.cu:76-96), shared by
 * vslam_fastgrid.hip (which defines the kernels and the functions below) and vslam_harrisgrid.hip.
 */
#ifndef VSLAM_GRIDPYR_H
#define VSLAM_GRIDPYR_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define FG_MAX_LEVELS 8
#define FG_MAX_BATCH 64

struct FgLevel {
    int32_t w, h, pitch;
    uint32_t pad;
    size_t base, bytes; /* level-major layout: image s of level l starts at base + s * bytes */
};
struct FgPtrs {
    const uint8_t* p[FG_MAX_BATCH];
};

/* Fills lv[0 .. levels) for max_batch images of w x h (level sizes are original >> l, pyramid_pool.cpp:61-62; pitches
 * are multiples of 64 with at least 8 bytes behind a row) and returns the bytes to allocate. */
size_t fg_pyramid_layout(FgLevel* lv, int w, int h, int levels, int max_batch);
/* n device images of pitch src_pitch -> level 0 (k_fg_gather) */
void fg_pyramid_gather(hipStream_t st, const uint8_t* const* imgs, int n, size_t src_pitch, uint8_t* pyr, const FgLevel& L0);
/* level l - 1 -> level l for l = 1 .. levels - 1 of n images (k_fg_halfsample, one launch per level) */
void fg_pyramid_halfsample(hipStream_t st, uint8_t* pyr, const FgLevel* lv, int levels, int n);

#endif
