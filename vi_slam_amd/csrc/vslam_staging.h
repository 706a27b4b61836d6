/* vslam_staging.h -- private: the staging block of a matcher entry point.  A block in HBM and a pinned mirror of the
 * same layout, carved by vslam::layout (vslam_host.h): the host fills the mirror's input parts, one range goes up, the
 * kernels run, one range of results comes down.  Included by vslam_ctx.h. */
#ifndef VSLAM_STAGING_H
#define VSLAM_STAGING_H
#include <hip/hip_runtime.h>

#include <cstring>

#include "vslam_host.h"
#include "vslam_kernels.h"
#include "vslam_mem.h"

/* `bytes` from src to dst on st by vk_copy_ranges (a copy kernel, or the runtime for large ranges); returns the number
 * of copy operations, which the sites that keep delivery statistics hand to vslam_count_delivery */
static inline int vslam_copy_range(hipStream_t st, void* dst, const void* src, size_t bytes,
                                   const vslam_tuning& T = vslam_process_tuning()) {
    CopyRanges R;
    memset(&R, 0, sizeof(R));
    R.dst[0] = dst;
    R.src[0] = src;
    R.bytes[0] = bytes;
    R.n = 1;
    return vk_copy_ranges(st, R, T);
}

struct vslam_staging {
    vslam_dbuf<uint8_t> d; /* HBM */
    vslam_hbuf<uint8_t> h; /* pinned mirror */
    /* grow-only: a smaller block reuses the buffers of a larger one before it */
    int ensure(size_t total) {
        const int rc = d.ensure(total);
        return rc ? rc : h.ensure(total);
    }
    void release() {
        d.release();
        h.release();
    }
    /* [off, off + bytes) of the block: mirror -> HBM, HBM -> mirror */
    int up(hipStream_t st, size_t off, size_t bytes) const { return vslam_copy_range(st, d + off, h + off, bytes); }
    int down(hipStream_t st, size_t off, size_t bytes) const { return vslam_copy_range(st, h + off, d + off, bytes); }
};

#endif
