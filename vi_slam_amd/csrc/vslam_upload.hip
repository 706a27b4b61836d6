/* vslam_upload.hip -- host images on their way into level 0: the pinned staging of pageable images, the two upload
 * transports (DMA engines into a device staging buffer, or a kernel that pulls over PCIe), the pixel format of the
 * image entries, and the NUMA-aware pinned allocator behind every pinned buffer of the library. */
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include "vslam_ctx.h"

#include <mutex>
#include <cstdio>
#include <cstdlib>

/* host images: rows into pinned staging (a copy kernel pulls them into HBM afterwards).  hipMemcpy2DAsync from
 * pageable memory took 2.8 ms per KITTI frame on this stack -- 90 % of a single-frame call. */
/* memcpy with streaming stores (dst 16-byte aligned): the staged image is read next by the GPU over PCIe, not by this
 * core -- lines left dirty in the core's cache have to be snooped out for every read the device makes */
static void copy_streaming(uint8_t* dst, const uint8_t* src, size_t n) {
#if defined(__SSE2__)
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(src + i)), b = _mm_loadu_si128((const __m128i*)(src + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(src + i + 32)), d = _mm_loadu_si128((const __m128i*)(src + i + 48));
        _mm_stream_si128((__m128i*)(dst + i), a);
        _mm_stream_si128((__m128i*)(dst + i + 16), b);
        _mm_stream_si128((__m128i*)(dst + i + 32), c);
        _mm_stream_si128((__m128i*)(dst + i + 48), d);
    }
    if (i < n) memcpy(dst + i, src + i, n - i);
    _mm_sfence();
#else
    memcpy(dst, src, n);
#endif
}

/* bytes of one image in the pinned staging h_img: level-0 pitch x height for gray, dense colour rows (256-byte aligned) else */
static size_t host_stage_stride(const vslam_fe* fe) {
    if (fe->pix_fmt == VSLAM_PIX_GRAY8) return (size_t)fe->geom.lv[0].pitch * (size_t)fe->p.height;
    return (vslam_row_bytes(fe) * (size_t)fe->p.height + 255) & ~(size_t)255;
}

int vslam_stage_host_images(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch) {
    const vslam_fe_params& p = fe->p;
    const size_t lp = fe->geom.lv[0].pitch, img_bytes = host_stage_stride(fe);
    if (int rc = fe->h_img.ensure(img_bytes * fe->B)) return rc; /* gray: first use; colour formats: vslam_fe_set_pixel_format allocated it */
    for (int s = 0; s < nimg; s++)
        if (!imgs[s]) {
            g_err = "null image";
            return VSLAM_ERR_INVALID;
        }
    if (fe->pix_fmt != VSLAM_PIX_GRAY8) { /* colour rows are staged dense, whatever the caller's pitch */
        const size_t rowb = vslam_row_bytes(fe);
        fe->h_img_pitch = rowb;
        fe->pool->parallel_for(nimg, [&](int s) {
            uint8_t* hs = fe->h_img + img_bytes * s;
            if (pitch == rowb) copy_streaming(hs, imgs[s], rowb * p.height);
            else
                for (int y = 0; y < p.height; y++) memcpy(hs + (size_t)y * rowb, imgs[s] + (size_t)y * pitch, rowb);
        });
        return VSLAM_OK;
    }
    /* one task per image on the context's worker pool: a single thread copies ~18 GB/s, which bounded the
     * host-image batch path at 0.85 ms per 32 KITTI frames */
    /* dense rows (pitch == width, what cv::Mat::isContinuous() images are) stay dense in the staging: ONE memcpy per
     * image instead of one per row (a 1241 x 376 frame: 12 instead of 27 us) and 3 % fewer bytes over the link; the
     * pull kernel and the DMA route take any source pitch */
    fe->h_img_pitch = pitch == (size_t)p.width ? (size_t)p.width : lp;
    fe->pool->parallel_for(nimg, [&](int s) {
        uint8_t* hs = fe->h_img + img_bytes * s;
        if (pitch == (size_t)p.width) copy_streaming(hs, imgs[s], (size_t)p.width * p.height);
        else if (pitch == lp) memcpy(hs, imgs[s], img_bytes - (lp - p.width));
        else
            for (int y = 0; y < p.height; y++) memcpy(hs + (size_t)y * lp, imgs[s] + (size_t)y * pitch, p.width);
    });
    return VSLAM_OK;
}

/* the widest row pitch vslam_stage_host_images leaves in h_img */
size_t vslam_host_stage_pitch(const vslam_fe* fe) {
    return fe->pix_fmt == VSLAM_PIX_GRAY8 ? (size_t)fe->geom.lv[0].pitch : vslam_row_bytes(fe);
}

/* VSLAM_H2D = sdma | pull forces one transport; default: the DMA engines for batches (they run beside the other
 * contexts' kernels without disturbing them), the pull kernel for one or two images (a synchronous single-frame call
 * has nothing to overlap with, and the hand-over between the DMA engine and the compute queue costs ~30 us) */
static bool h2d_uses_sdma(const vslam_fe* fe, int nimg) {
    const int mode = fe->tune.h2d_route; /* 1 pull, 2 sdma, else by batch size */
    return mode == 2 || (mode != 1 && nimg > 2);
}

/* the device staging buffer of the sdma transport, allocated OUTSIDE stream capture (hipMalloc is not capturable) */
int vslam_stage_ensure(vslam_fe* fe, size_t spitch, int nimg) {
    if (!h2d_uses_sdma(fe, nimg)) return VSLAM_OK;
    const size_t one = (size_t)(fe->p.height - 1) * spitch + vslam_row_bytes(fe);
    const size_t stride = (one + 255) & ~(size_t)255;
    if (fe->d_stage.bytes() >= stride * fe->B + 256) return VSLAM_OK;
    HIPCHK(vslam_stream_wait(fe->stream)); /* an earlier pass may still read the old buffer */
    return fe->d_stage.ensure(stride * fe->B + 256);
}

/* Host rows -> level 0 of slots 0..nimg-1, enqueued on fe's stream.  `where` = VSLAM_IMGS_PINNED (the caller's pinned
 * images) or VSLAM_IMGS_HOST (rows already copied into the context's pinned staging by vslam_stage_host_images).
 * Two transports (VSLAM_H2D = sdma | pull, default sdma):
 *   sdma: hipMemcpyAsync (the DMA engines: no CU, no L2 miss-queue entries held for microseconds) copies every image
 *         as one linear block into a device staging buffer -- ONE call when the images are equally spaced in memory, as
 *         the buffers of a capture ring are -- and a kernel re-pitches from HBM into the 128-byte-pitched level 0.
 *         Measured beside the other contexts' kernels: 102 k frames/s against 64-72 k with the pull kernel, whose host
 *         reads (2-3 us each) sit in the L2's queues in front of everybody's HBM requests (describe 122 -> 274 us).
 *   pull: one kernel reads the host rows over PCIe itself (55 GB/s alone on the GPU; kept for A/B runs). */
static bool hip_stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int vslam_upload_host_rows(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int where) {
    const vslam_fe_params& p = fe->p;
    hipStream_t st = fe->stream;
    const size_t lp = fe->geom.lv[0].pitch, img_bytes = host_stage_stride(fe);
    const size_t rowb = vslam_row_bytes(fe); /* bytes of a source row: the width, or width x 3 | 4 of a colour format */
    const bool use_sdma = h2d_uses_sdma(fe, nimg);
    BatchSrc hs;
    for (int s = 0; s < nimg; s++) {
        if (where == VSLAM_IMGS_PINNED && !imgs[s]) {
            g_err = "null image";
            return VSLAM_ERR_INVALID;
        }
        hs.l0[s] = where == VSLAM_IMGS_PINNED ? imgs[s] : fe->h_img + img_bytes * s;
        hs.pitch0[s] = where == VSLAM_IMGS_PINNED ? (uint32_t)pitch : (uint32_t)fe->h_img_pitch;
    }
    int from_host = 1;
    if (use_sdma) {
        const size_t spitch = hs.pitch0[0];
        const size_t one = (size_t)(p.height - 1) * spitch + rowb; /* bytes of one image, first to last pixel */
        const size_t stride = (one + 255) & ~(size_t)255;
        if (fe->d_stage.bytes() < stride * fe->B + 256) { /* vslam_stage_ensure() runs before any capture; cannot happen */
            g_err = "internal: device staging buffer not allocated";
            return VSLAM_ERR_HIP;
        }
        hipStream_t cs = st;
        bool even = nimg > 1; /* equally spaced sources: one copy */
        const ptrdiff_t d = nimg > 1 ? hs.l0[1] - hs.l0[0] : 0;
        for (int s = 2; s < nimg && even; s++) even = hs.l0[s] - hs.l0[s - 1] == d;
        if (even && d > 0 && (size_t)d >= one && (size_t)d * (nimg - 1) + one <= fe->d_stage.bytes()) {
            /* vslam_tuning.stage_split_event = k (0..3): the upload goes as TWO transfers and the context's user event k
             * (vslam_fe_event_wait) is recorded between them -- a pipelined caller that chains the uploads of its contexts
             * on that event keeps a second transfer queued behind the running one, so the link does not idle for the
             * hand-over between two chained uploads */
            const int ek = fe->tune.stage_split_event;
            const int h1 = nimg / 2;
            if (ek >= 0 && ek < 4 && h1 >= 1 && !hip_stream_capturing(cs)) {
                HIPCHK(hipMemcpyAsync(fe->d_stage, hs.l0[0], (size_t)d * h1, hipMemcpyHostToDevice, cs));
                if (int rc = fe->ev_user[ek].ensure(hipEventDisableTiming)) return rc;
                HIPCHK(hipEventRecord(fe->ev_user[ek], cs));
                HIPCHK(hipMemcpyAsync(fe->d_stage + (size_t)d * h1, hs.l0[0] + (size_t)d * h1, (size_t)d * (nimg - 1 - h1) + one,
                                      hipMemcpyHostToDevice, cs));
            } else
                HIPCHK(hipMemcpyAsync(fe->d_stage, hs.l0[0], (size_t)d * (nimg - 1) + one, hipMemcpyHostToDevice, cs));
            for (int s = 0; s < nimg; s++) hs.l0[s] = fe->d_stage + (size_t)d * s;
        } else {
            for (int s = 0; s < nimg; s++) {
                HIPCHK(hipMemcpyAsync(fe->d_stage + stride * s, hs.l0[s], one, hipMemcpyHostToDevice, cs));
                hs.l0[s] = fe->d_stage + stride * s;
            }
        }
        from_host = 0;
    }
    if (fe->pix_fmt != VSLAM_PIX_GRAY8) /* cv::cvtColor on the way into level 0 */
        vk_gray_images(st, hs, fe->d_pyr, fe->slot_stride, fe->geom.lv[0].off, (int)lp, p.width, p.height, nimg, from_host,
                       fe->pix_fmt, fe->gray_shift, fe->tune);
    else
        vk_pull_images(st, hs, fe->d_pyr, fe->slot_stride, fe->geom.lv[0].off, (int)lp, p.width, p.height, nimg, from_host, fe->tune);
    return VSLAM_OK;
}

extern "C" int vslam_fe_stage_images_async(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch,
                                           int where) {
    if (!fe || !imgs || nimg < 1 || nimg > fe->B || pitch < vslam_row_bytes(fe) ||
        (where != VSLAM_IMGS_PINNED && where != VSLAM_IMGS_HOST)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    if (where == VSLAM_IMGS_HOST) {
        HIPCHK(vslam_stream_wait(fe->stream)); /* the pinned staging may still be read by the previous pull */
        int rc = vslam_stage_host_images(fe, nimg, imgs, pitch);
        if (rc) return rc;
    }
    int rc2 = vslam_stage_ensure(fe, where == VSLAM_IMGS_PINNED ? pitch : vslam_host_stage_pitch(fe), nimg);
    if (rc2) return rc2;
    /* (Tried in round 2 and removed: the DMA copy on an upload stream of its own, issued passes ahead of its use.  One
     * upload stream serialises copies that otherwise overlap on several DMA engines -- 77-86 k against 85-103 k mono
     * frames/s -- and the host-input rate is bound by the link either way.) */
    rc2 = vslam_upload_host_rows(fe, nimg, imgs, pitch, where);
    if (rc2) return rc2;
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

/* The pixel format of every image entry (cv::cvtColor in front of the three GrabImage* callers).  The captured graph holds
 * the upload kernel of the format it was captured with: dropped.  Staging for the wider rows is allocated here, outside
 * any capture: the pinned rows of pageable images, and the DMA route's device buffer for dense rows (vslam_stage_ensure grows it
 * for a wider pitch before a pass is captured, as it does for gray). */
extern "C" int vslam_fe_set_pixel_format(vslam_fe* fe, int fmt, int gray_shift) {
    if (!fe || fmt < VSLAM_PIX_GRAY8 || fmt > VSLAM_PIX_BGRA8 || (gray_shift != 0 && gray_shift != 14 && gray_shift != 15)) {
        g_err = "invalid pixel format or gray shift (0, 14 or 15)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    if (fe->stream) HIPCHK(hipStreamSynchronize(fe->stream)); /* a pass in flight may still read the staging */
    if (fe->graph_exec) {
        (void)hipGraphExecDestroy(fe->graph_exec);
        fe->graph_exec = nullptr;
        fe->graph_key = 0;
    }
    fe->pix_fmt = fmt;
    fe->gray_shift = gray_shift ? gray_shift : 15;
    if (fmt == VSLAM_PIX_GRAY8) { /* gray allocates its own on first use, as ever */
        fe->h_img.release();
        return VSLAM_OK;
    }
    if (int rc = fe->h_img.ensure(host_stage_stride(fe) * fe->B)) return rc;
    return vslam_stage_ensure(fe, vslam_row_bytes(fe), fe->B);
}

extern "C" int vslam_fe_get_pixel_format(const vslam_fe* fe, int* fmt, int* gray_shift) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (fmt) *fmt = fe->pix_fmt;
    if (gray_shift) *gray_shift = fe->gray_shift;
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ pinned host memory on the GPU's NUMA node
 * hipHostMalloc takes its pages from the node the calling thread happens to run on; across the socket boundary the
 * link delivered noticeably less (host-input rate of the mono workload: 79-84 k frames/s on some runs, 96 k on others).
 * The allocating thread is moved onto the CPUs next to the device for the duration of the allocation and its first
 * touch (sysfs: /sys/bus/pci/devices/<bus id>/local_cpulist), then back.  VSLAM_NUMA=0 disables. */
#include <sched.h>
static bool device_cpuset(cpu_set_t* out) {
    static std::mutex mu; /* contexts may be created from several threads */
    std::lock_guard<std::mutex> lk(mu);
    /* one entry per device (the current one): a process with contexts on several GPUs gets each device's own CPUs */
    struct PerDevice {
        int state = 0; /* 0 unknown, 1 unavailable, 2 cached */
        cpu_set_t set;
    };
    static PerDevice per_device[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    int& state = per_device[dev].state;
    cpu_set_t& cached = per_device[dev].set;
    if (state == 0) {
        state = 1;
        const bool off = vslam_process_tuning().numa == 0; /* process-wide */
        char bus[64] = {0};
        if (!off && hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev) == hipSuccess) {
            for (char* c = bus; *c; c++) *c = (char)tolower(*c);
            char path[160];
            snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bus);
            if (FILE* fp = fopen(path, "r")) {
                char line[1024] = {0};
                if (fgets(line, sizeof(line), fp)) {
                    CPU_ZERO(&cached);
                    int n = 0;
                    char* save = nullptr;
                    for (char* tok = strtok_r(line, ",\n", &save); tok; tok = strtok_r(nullptr, ",\n", &save)) {
                        int a = 0, b = 0;
                        const int k = sscanf(tok, "%d-%d", &a, &b);
                        if (k == 1) b = a;
                        if (k >= 1)
                            for (int c = a; c <= b && c < CPU_SETSIZE; c++) {
                                CPU_SET(c, &cached);
                                n++;
                            }
                    }
                    if (n > 0) state = 2;
                }
                fclose(fp);
            }
        }
    }
    if (state == 2) *out = cached;
    return state == 2;
}
int vslam_pinned_alloc(void** p, size_t bytes) {
    cpu_set_t near, saved;
    const bool move = device_cpuset(&near) && sched_getaffinity(0, sizeof(saved), &saved) == 0;
    bool moved = false;
    if (move) {
        cpu_set_t both;
        CPU_AND(&both, &near, &saved); /* never leave the set the process is allowed on */
        if (CPU_COUNT(&both) > 0) moved = sched_setaffinity(0, sizeof(both), &both) == 0;
    }
    const hipError_t rc = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (rc == hipSuccess && moved) memset(*p, 0, bytes); /* first touch while we are on the right node */
    if (moved) sched_setaffinity(0, sizeof(saved), &saved);
    return (int)rc;
}

extern "C" int vslam_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return VSLAM_ERR_INVALID;
    *out = nullptr;
    HIPCHK((hipError_t)vslam_pinned_alloc(out, bytes));
    return VSLAM_OK;
}
extern "C" void vslam_host_free(void* p) {
    if (p) hipHostFree(p);
}
