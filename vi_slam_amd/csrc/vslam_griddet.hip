/* vslam_griddet.hip -- the pyramid kernels and the host object of the grid detectors (vslam_griddet.h). */
#include "vslam_griddet.h"

/* ---------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256)
k_fg_gather(FgPtrs src, size_t src_pitch, uint8_t* pyr, FgLevel d) { /* device images -> level 0 */
    const int x16 = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), s = blockIdx.z;
    if (y >= d.h || x16 * 16 >= d.w) return;
    const uint8_t* sp = src.p[s] + (size_t)y * src_pitch + (size_t)x16 * 16;
    uint8_t* dp = pyr + d.base + (size_t)s * d.bytes + (size_t)y * d.pitch + (size_t)x16 * 16;
    const int n = min(16, d.w - x16 * 16);
    if (n == 16 && (((uintptr_t)sp) & 15) == 0) {
        *(uint4*)dp = *(const uint4*)sp;
    } else if (n == 16 && (((uintptr_t)sp) & 3) == 0) {
        const uint32_t* s4 = (const uint32_t*)sp;
        *(uint4*)dp = make_uint4(s4[0], s4[1], s4[2], s4[3]);
    } else {
        for (int i = 0; i < n; i++) dp[i] = sp[i];
    }
}

/* K5: (a + b + c + d) >> 2 */
__global__ void __launch_bounds__(256)
k_fg_halfsample(uint8_t* pyr, FgLevel s, FgLevel d) {
    const int q = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), img = blockIdx.z;
    if (y >= d.h || 4 * q >= d.w) return;
    const uint8_t* sp = pyr + s.base + (size_t)img * s.bytes + (size_t)(2 * y) * s.pitch + (size_t)q * 8;
    const uint2 t = *(const uint2*)sp, b = *(const uint2*)(sp + s.pitch); /* pitches are multiples of 64 */
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t tw = i < 2 ? t.x : t.y, bw = i < 2 ? b.x : b.y;
        const int sh = (i & 1) * 16;
        const uint32_t v = ((tw >> sh) & 0xFF) + ((tw >> (sh + 8)) & 0xFF) + ((bw >> sh) & 0xFF) + ((bw >> (sh + 8)) & 0xFF);
        out |= (v >> 2) << (8 * i);
    }
    *(uint32_t*)(pyr + d.base + (size_t)img * d.bytes + (size_t)y * d.pitch + (size_t)q * 4) = out;
}

/* ---------------------------------------------------------------------------------------------- host */
size_t fg_pyramid_layout(FgLevel* lv, int w, int h, int levels, int max_batch) {
    size_t off = 0;
    for (int l = 0; l < levels; l++) {
        FgLevel& L = lv[l];
        L.w = w >> l; /* pyramid_pool.cpp:61-62 */
        L.h = h >> l;
        L.pitch = (L.w + 8 + 63) & ~63;
        L.bytes = (size_t)L.pitch * L.h;
        L.base = off;
        off += L.bytes * max_batch;
    }
    return off + 256;
}

void fg_pyramid_gather(hipStream_t st, const uint8_t* const* imgs, int n, size_t src_pitch, uint8_t* pyr, const FgLevel& L0) {
    FgPtrs P;
    memset(&P, 0, sizeof(P));
    for (int s = 0; s < n; s++) P.p[s] = imgs[s];
    hipLaunchKernelGGL(k_fg_gather, dim3(((L0.w + 15) / 16 + 63) / 64, (L0.h + 3) / 4, n), dim3(256), 0, st, P, src_pitch, pyr, L0);
}

void fg_pyramid_halfsample(hipStream_t st, uint8_t* pyr, const FgLevel* lv, int levels, int n) {
    for (int l = 1; l < levels; l++) {
        const FgLevel& D = lv[l];
        hipLaunchKernelGGL(k_fg_halfsample, dim3(((D.w + 3) / 4 + 63) / 64, (D.h + 3) / 4, n), dim3(256), 0, st, pyr, lv[l - 1], D);
    }
}

int gd_alloc(GdHost& h) {
    const FgLevel& L0 = h.G.lv[0];
    HIPCHK(hipSetDevice(h.device));
    HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    if (int rc = h.d_pyr.alloc(h.pyr_bytes)) return rc;
    h.search_pyr = h.d_pyr;
    HIPCHK(hipMemset(h.d_pyr, 0, h.pyr_bytes));
    if (int rc = h.h_img.alloc(L0.bytes * h.max_batch)) return rc;
    memset(h.h_img, 0, L0.bytes * h.max_batch);
    if (int rc = h.d_grid.alloc((size_t)h.cells * 16 * h.max_batch)) return rc;
    if (int rc = h.h_grid.alloc((size_t)h.cells * 16 * h.max_batch)) return rc;
    if (int rc = h.d_resp.alloc((size_t)L0.w * L0.h)) return rc;
    HIPCHK(hipDeviceSynchronize());
    return VSLAM_OK;
}

void gd_free(GdHost& h) {
    (void)hipSetDevice(h.device);
    if (h.stream) (void)hipStreamSynchronize(h.stream);
    if (h.stream) (void)hipStreamDestroy(h.stream);
}

int gd_grid(const GdHost* h, int* n_cols, int* n_rows) {
    if (!h) return VSLAM_ERR_INVALID;
    if (n_cols) *n_cols = h->G.n_cols;
    if (n_rows) *n_rows = h->G.n_rows;
    return VSLAM_OK;
}

int gd_nt() {
    const int v = vslam_process_tuning().fg_threads; /* process-wide */
    return (v == 64 || v == 128 || v == 256) ? v : 128;
}

void gd_stage_images(GdHost* h, int n, const uint8_t* const* imgs, size_t pitch, int on_device, uint8_t* pyr) {
    const FgLevel& L0 = h->G.lv[0];
    if (on_device) {
        fg_pyramid_gather(h->stream, imgs, n, pitch, pyr, L0);
    } else { /* pageable rows -> pinned staging in the device layout -> one copy kernel (see vslam_fe.hip) */
        for (int s = 0; s < n; s++)
            for (int y = 0; y < L0.h; y++) memcpy(h->h_img + (size_t)s * L0.bytes + (size_t)y * L0.pitch, imgs[s] + (size_t)y * pitch, L0.w);
        vslam_copy_range(h->stream, pyr + L0.base, h->h_img, L0.bytes * n);
    }
}

int gd_detect_pyramid(GdHost* h, int n, uint8_t* pyr, float* pos, float* score, int32_t* level) {
    h->search_pyr = pyr; /* the launch reads it */
    h->launch(h, n, nullptr, -1, -1);
    h->search_pyr = h->d_pyr;
    vslam_copy_range(h->stream, h->h_grid, h->d_grid, (size_t)h->cells * 16 * n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    const int C = h->cells;
    for (int s = 0; s < n; s++) {
        const uint8_t* g = h->h_grid + (size_t)s * C * 16;
        memcpy(pos + (size_t)s * C * 2, g, (size_t)C * 8);
        memcpy(score + (size_t)s * C, g + (size_t)C * 8, (size_t)C * 4);
        memcpy(level + (size_t)s * C, g + (size_t)C * 12, (size_t)C * 4);
    }
    return VSLAM_OK;
}

int gd_detect_batch(GdHost* h, int n, const uint8_t* const* imgs, size_t pitch, int on_device, float* pos, float* score,
                    int32_t* level) {
    if (!h || n < 1 || n > h->max_batch || !imgs || !pos || !score || !level || pitch < (size_t)h->G.lv[0].w) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int s = 0; s < n; s++)
        if (!imgs[s]) {
            g_err = "null image";
            return VSLAM_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(h->device));
    gd_stage_images(h, n, imgs, pitch, on_device, h->d_pyr);
    fg_pyramid_halfsample(h->stream, h->d_pyr, h->G.lv, h->G.max_level, n);
    const int rc = gd_detect_pyramid(h, n, h->d_pyr, pos, score, level);
    if (rc == VSLAM_OK) h->last_n = n;
    return rc;
}

int gd_level_copy(GdHost* h, int slot, int level, uint8_t* dst, size_t dst_pitch, int* w, int* h_out) {
    if (!h || slot < 0 || slot >= h->last_n || level < 0 || level >= h->G.max_level) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const FgLevel& L = h->G.lv[level];
    if (w) *w = L.w;
    if (h_out) *h_out = L.h;
    if (!dst) return VSLAM_OK;
    if (dst_pitch < (size_t)L.w) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, h->d_pyr + L.base + (size_t)slot * L.bytes, L.pitch, L.w, L.h, hipMemcpyDeviceToHost,
                            h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VSLAM_OK;
}

int gd_response_copy(GdHost* h, int slot, int level, float* dst) {
    if (!h || !dst || slot < 0 || slot >= h->last_n || level < h->G.min_level || level >= h->G.max_level) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const FgLevel& L = h->G.lv[level];
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemsetAsync(h->d_resp, 0, (size_t)L.w * L.h * 4, h->stream));
    h->launch(h, h->last_n, h->d_resp, level, slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, h->d_resp, (size_t)L.w * L.h * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VSLAM_OK;
}
