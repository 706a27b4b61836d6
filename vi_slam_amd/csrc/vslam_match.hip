/* vslam_match.hip -- FMatcher::SearchForInitialization: the whole matcher on the device (k_si_*), or the distances from
 * the device and the order-dependent part replayed on the host; the grid-bounds setters of the projection matchers;
 * the dbg_* entry points of the tests; the brute-force descriptor matchers (vslam_hamming_*, the fisheye stereo
 * candidates). */
#include "vslam_ctx.h"

/* ------------------------------------------------------------------ SearchForInitialization on the device */
static int init_scratch(vslam_fe* fe, int npairs) {
    const size_t per = (size_t)fe->cap * 4 + (size_t)fe->cap * 8 + 16;
    const bool stereo_owns = fe->init_in_block && fe->block_region_owner == VSLAM_REGION_STEREO;
    if (per * npairs <= fe->init_bytes && !stereo_owns) { /* the result block's own region: up to max_batch pairs */
        if (fe->init_in_block) fe->block_region_owner = VSLAM_REGION_INIT;
        return VSLAM_OK;
    }
    /* more pairs than image slots, or the stereo matcher's outputs live there: the context's own pair from now on */
    fe->init_in_block = false;
    fe->d_init = fe->h_init = nullptr;
    fe->init_bytes = 0;
    int rc = fe->d_init_own.ensure(per * npairs);
    if (!rc) rc = fe->h_init_own.ensure(per * npairs);
    if (rc) return rc;
    fe->d_init = fe->d_init_own;
    fe->h_init = fe->h_init_own;
    fe->init_bytes = fe->d_init_own.bytes();
    return VSLAM_OK;
}

extern "C" int vslam_fe_set_grid_bounds(vslam_fe* fe, const vslam_bounds* b) {
    if (!fe) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (!b) {
        fe->has_grid_bounds = false;
        return VSLAM_OK;
    }
    if (!bounds_ok(b)) {
        g_err = "invalid image bounds";
        return VSLAM_ERR_INVALID;
    }
    fe->grid_bounds = SiBounds{b->min_x, b->max_x, b->min_y, b->max_y};
    fe->has_grid_bounds = true;
    return VSLAM_OK;
}

extern "C" int vslam_fe_get_grid_bounds(const vslam_fe* fe, vslam_bounds* b, int* is_set) {
    if (!fe || !b || !is_set) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const SiBounds s = matcher_bounds(fe, fe->p.width, fe->p.height);
    *b = vslam_bounds{s.minX, s.maxX, s.minY, s.maxY};
    *is_set = fe->has_grid_bounds ? 1 : 0;
    return VSLAM_OK;
}

static int search_init_dev_async_b(vslam_fe* fe, int npairs, const vslam_init_job* jobs, const SiBounds& bnd, int window,
                                   float nnratio, int check_orientation) {
    if (!fe || npairs < 1 || npairs > VSLAM_MAX_MAT_JOBS || !jobs) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (!(nnratio >= 0.2f)) { /* see the distance clamp in vslam_init_kernel.hip */
        g_err = "SearchForInitialization on the device needs nnratio >= 0.2";
        return VSLAM_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    InitJobs J;
    memset(&J, 0, sizeof(J));
    for (int j = 0; j < npairs; j++) {
        if (!jobs[j].dev_kps1 || !jobs[j].dev_desc1 || !jobs[j].dev_n1 || !jobs[j].dev_kps2 || !jobs[j].dev_desc2 ||
            !jobs[j].dev_n2) {
            g_err = "null device pointer in job";
            return VSLAM_ERR_INVALID;
        }
        J.job[j].k1 = jobs[j].dev_kps1;
        J.job[j].d1 = jobs[j].dev_desc1;
        J.job[j].cnt1 = jobs[j].dev_n1;
        J.job[j].k2 = jobs[j].dev_kps2;
        J.job[j].d2 = jobs[j].dev_desc2;
        J.job[j].cnt2 = jobs[j].dev_n2;
        J.job[j].prev = jobs[j].dev_prev_matched;
    }
    int rc = init_scratch(fe, npairs);
    if (rc) return rc;
    /* octave-0 keypoints of frame 2 kept in LDS: the level-0 quota (+ the quadtree's overshoot) bounds them
     * for extractor output; foreign inputs are clipped to the context's capacity */
    const int max_c2 = std::min(fe->cap, std::max(fe->tab.quota[0] + 8, 64));
    if (max_c2 > 4096) { /* candidate slot is a 12-bit field of the ordering key */
        g_err = "SearchForInitialization on the device supports at most 4096 octave-0 keypoints per frame";
        return VSLAM_ERR_UNSUPPORTED;
    }
    const size_t lds = vk_search_init_lds(fe->cap, max_c2);
    if (lds > 150 * 1024) {
        g_err = "SearchForInitialization: keypoint capacity too large for the LDS-resident matcher";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (!fe->init_lds_set) {
        if (vk_search_init_set_max_lds(150 * 1024) != 0) {
            g_err = "hipFuncSetAttribute(k_si_*) failed";
            return VSLAM_ERR_HIP;
        }
        fe->init_lds_set = true;
    }
    /* sorted candidate prefix per query; VSLAM_INIT_TOPM=<1..16> (tests force the re-scan path with 2) */
    const int M = std::min(16, std::max(1, tune_or(fe->tune.init_topm, 8)));
    rc = fe->d_init_scratch.ensure(vk_search_init_scratch_bytes(npairs, max_c2, M) + 16);
    if (!rc) rc = vslam_init_fb_ensure(fe);
    if (rc) return rc;
    const size_t nm = (size_t)npairs * fe->cap;
    int32_t* d_m = (int32_t*)fe->d_init;
    float* d_p = (float*)(d_m + nm);
    int32_t* d_n = (int32_t*)(d_p + 2 * nm);
    vk_search_init(fe->stream, J, npairs, fe->cap, bnd, window, nnratio, check_orientation, d_m, d_p, d_n,
                   max_c2, M, fe->d_init_scratch, fe->d_init_fb, fe->tune);
    HIPCHK(hipGetLastError());
    if (fe->deliver_deferred && fe->init_in_block) {
        /* the extraction of this step asked for its delivery to be deferred (want_host = 2): counts, keypoints, descriptors
         * and the matcher's outputs are contiguous in the result block -> ONE transfer for the whole step */
        fe->deliver_deferred = false;
        const int rc = vslam_deliver_block(fe, (nm * 12 + (size_t)npairs * 4 + 15) & ~(size_t)15);
        if (rc) return rc;
    } else {
        const size_t bytes = nm * 12 + (size_t)npairs * 4;
        vslam_count_delivery(fe, vslam_copy_range(fe->stream, fe->h_init, fe->d_init, bytes, fe->tune), bytes);
        HIPCHK(hipGetLastError());
    }
    fe->init_pairs = npairs;
    return VSLAM_OK;
}

extern "C" int vslam_search_init_dev_async(vslam_fe* fe, int npairs, const vslam_init_job* jobs, int img_w,
                                           int img_h, int window, float nnratio, int check_orientation) {
    return search_init_dev_async_b(fe, npairs, jobs, int_bounds(img_w, img_h), window, nnratio, check_orientation);
}

extern "C" int vslam_search_init_dev_async_ex(vslam_fe* fe, int npairs, const vslam_init_job* jobs, const vslam_bounds* b,
                                              int window, float nnratio, int check_orientation) {
    if (!bounds_ok(b)) {
        g_err = "invalid image bounds";
        return VSLAM_ERR_INVALID;
    }
    return search_init_dev_async_b(fe, npairs, jobs, SiBounds{b->min_x, b->max_x, b->min_y, b->max_y}, window, nnratio,
                                   check_orientation);
}

extern "C" int vslam_search_init_dev_wait(vslam_fe* fe, const int* n1, int32_t* const* matches12,
                                          float* const* prev_matched, int* nmatches) {
    if (!fe || fe->init_pairs < 1) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    const int npairs = fe->init_pairs;
    const size_t nm = (size_t)npairs * fe->cap;
    const int32_t* h_m = (const int32_t*)fe->h_init;
    const float* h_p = (const float*)(h_m + nm);
    const int32_t* h_n = (const int32_t*)(h_p + 2 * nm);
    for (int j = 0; j < npairs; j++) {
        const int n = n1 ? std::min(n1[j], fe->cap) : 0;
        if (matches12 && matches12[j] && n) memcpy(matches12[j], h_m + (size_t)j * fe->cap, (size_t)n * 4);
        if (prev_matched && prev_matched[j] && n) memcpy(prev_matched[j], h_p + (size_t)j * fe->cap * 2, (size_t)n * 8);
        if (nmatches) nmatches[j] = h_n[j];
    }
    for (int j = 0; j < npairs; j++)
        if (h_n[j] < 0) { /* k_si_topm found more octave-0 keypoints than its lists hold: nothing was truncated silently */
            g_err = "SearchForInitialization on the device: more octave-0 keypoints in a frame than the context's "
                    "level-0 quota allows (use the host-keypoint entry point, which falls back to the host replay)";
            return VSLAM_ERR_CAPACITY;
        }
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ SearchForInitialization */
static int search_init_batch_b(vslam_fe* fe, int npairs, const vslam_kp* const* kps1, const uint8_t* const* dev_desc1,
                               const int* n1, const vslam_kp* const* kps2, const uint8_t* const* dev_desc2, const int* n2,
                               const SiBounds& bnd, float* const* prev_matched, int32_t* const* matches12, int window,
                               float nnratio, int check_orientation, int* nmatches) {
    if (!fe || npairs < 1 || npairs > VSLAM_MAX_MAT_JOBS || !kps1 || !dev_desc1 || !n1 || !kps2 || !dev_desc2 ||
        !n2 || !prev_matched || !matches12 || !nmatches) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int j = 0; j < npairs; j++)
        if (n1[j] < 0 || n2[j] < 0 || (n1[j] && (!kps1[j] || !dev_desc1[j] || !prev_matched[j] || !matches12[j])) ||
            (n2[j] && (!kps2[j] || !dev_desc2[j]))) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(fe->p.device));
    {
        /* default: the whole matcher on the GPU (k_si_topm + k_si_replay).  VSLAM_INIT_MATCH=host keeps the distance
         * matrices on the GPU and replays the order-dependent part on the host (cross-check path). */
        const bool host_mode = fe->tune.init_match_host == 1;
        bool fits = true;
        for (int j = 0; j < npairs; j++) fits = fits && n1[j] <= fe->cap && n2[j] <= fe->cap;
        fits = fits && fe->tab.quota[0] + 8 <= 4096 && nnratio >= 0.2f;
        /* the device matcher keeps at most max_c2 octave-0 keypoints per frame (sized for THIS context's level-0
         * quota); keypoints from another extractor configuration can exceed that while n <= cap: host replay then */
        const int max_c2 = std::min(fe->cap, std::max(fe->tab.quota[0] + 8, 64));
        for (int j = 0; j < npairs && fits; j++) {
            int o1 = 0, o2 = 0;
            for (int i = 0; i < n1[j]; i++) o1 += kps1[j][i].octave == 0;
            for (int i = 0; i < n2[j]; i++) o2 += kps2[j][i].octave == 0;
            fits = o1 <= max_c2 && o2 <= max_c2;
        }
        if (!host_mode && fits) {
            /* upload keypoints, counts and vbPrevMatched of every pair, run, download */
            size_t bytes = 0;
            for (int j = 0; j < npairs; j++) bytes += ((size_t)(n1[j] + n2[j]) * sizeof(vslam_kp) + (size_t)n1[j] * 8 + 16 + 63) & ~(size_t)63;
            int rc = fe->d_tmp_desc[1].ensure(bytes + 64);
            if (rc) return rc;
            std::vector<uint8_t> stage(bytes + 64);
            std::vector<vslam_init_job> jobs(npairs);
            size_t off = 0;
            for (int j = 0; j < npairs; j++) {
                uint8_t* base = fe->d_tmp_desc[1] + off;
                uint8_t* hb = stage.data() + off;
                int32_t cnt[4] = {n1[j], n2[j], 0, 0};
                memcpy(hb, cnt, 16);
                memcpy(hb + 16, kps1[j], (size_t)n1[j] * sizeof(vslam_kp));
                memcpy(hb + 16 + (size_t)n1[j] * sizeof(vslam_kp), kps2[j], (size_t)n2[j] * sizeof(vslam_kp));
                const size_t poff = 16 + (size_t)(n1[j] + n2[j]) * sizeof(vslam_kp);
                memcpy(hb + poff, prev_matched[j], (size_t)n1[j] * 8);
                jobs[j].dev_n1 = (const int32_t*)base;
                jobs[j].dev_n2 = (const int32_t*)base + 1;
                jobs[j].dev_kps1 = (const vslam_kp*)(base + 16);
                jobs[j].dev_kps2 = (const vslam_kp*)(base + 16 + (size_t)n1[j] * sizeof(vslam_kp));
                jobs[j].dev_prev_matched = (const float*)(base + poff);
                jobs[j].dev_desc1 = dev_desc1[j];
                jobs[j].dev_desc2 = dev_desc2[j];
                off += (poff + (size_t)n1[j] * 8 + 63) & ~(size_t)63;
            }
            HIPCHK(hipMemcpyAsync(fe->d_tmp_desc[1], stage.data(), off, hipMemcpyHostToDevice, fe->stream));
            HIPCHK(vslam_stream_wait(fe->stream)); /* stage is pageable and goes out of scope */
            rc = search_init_dev_async_b(fe, npairs, jobs.data(), bnd, window, nnratio, check_orientation);
            if (rc) return rc;
            return vslam_search_init_dev_wait(fe, n1, matches12, prev_matched, nmatches);
        }
    }
    /* only octave-0 keypoints take part (fmatcher.cpp:999-1003: level1 > 0 -> continue; window query
     * restricted to [level1, level1]) */
    std::vector<std::vector<int>> row_of(npairs), col_of(npairs);
    std::vector<int32_t> idx;
    MatJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    size_t rows_total = 0, out_total = 0;
    int maxr = 0, maxc = 0;
    for (int j = 0; j < npairs; j++) {
        MatJob& jb = jobs.job[j];
        row_of[j].assign(n1[j], -1);
        col_of[j].assign(n2[j], -1);
        jb.idx_off1 = (uint32_t)idx.size();
        int nr = 0, nc = 0;
        for (int i = 0; i < n1[j]; i++)
            if (kps1[j][i].octave == 0) { row_of[j][i] = nr++; idx.push_back(i); }
        jb.idx_off2 = (uint32_t)idx.size();
        for (int i = 0; i < n2[j]; i++)
            if (kps2[j][i].octave == 0) { col_of[j][i] = nc++; idx.push_back(i); }
        jb.desc1 = dev_desc1[j];
        jb.desc2 = dev_desc2[j];
        jb.nr = nr;
        jb.nc = nc;
        jb.q_off = (uint32_t)rows_total;
        jb.t_off = (uint32_t)(rows_total + nr);
        jb.out_off = out_total;
        rows_total += (size_t)nr + nc;
        out_total += ((size_t)nr * nc + 15) & ~(size_t)15;
        maxr = std::max(maxr, nr);
        maxc = std::max(maxc, nc);
    }
    std::vector<uint8_t> dmat(std::max<size_t>(out_total, 16));
    if (maxr && maxc) {
        int rc;
        const size_t ib = (idx.size() * 4 + 255) & ~(size_t)255;
        if ((rc = fe->d_tmp_desc[0].ensure(ib + rows_total * 32))) return rc;
        if ((rc = fe->d_dmat.ensure(out_total))) return rc;
        int32_t* d_idx = (int32_t*)fe->d_tmp_desc[0];
        uint8_t* d_rows = fe->d_tmp_desc[0] + ib;
        hipStream_t st = fe->stream;
        HIPCHK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
        vk_hamming_matrix_batch(st, jobs, npairs, maxr, maxc, d_idx, d_rows, fe->d_dmat);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dmat.data(), fe->d_dmat, out_total, hipMemcpyDeviceToHost, st));
        HIPCHK(vslam_stream_wait(st));
    }
    /* the stealing / ratio / rotation-histogram logic is order dependent: replayed on the host, one
     * pair per worker */
    const float hb[4] = {bnd.minX, bnd.maxX, bnd.minY, bnd.maxY};
    fe->pool->parallel_for(npairs, [&](int j) {
        const MatJob& jb = jobs.job[j];
        nmatches[j] = vslam::search_for_initialization_replay(
            kps1[j], n1[j], kps2[j], n2[j], dmat.data() + jb.out_off, row_of[j].data(), col_of[j].data(),
            std::max(jb.nc, 1), hb, prev_matched[j], matches12[j], window, nnratio, check_orientation != 0);
    });
    return VSLAM_OK;
}

extern "C" int vslam_search_for_initialization_batch(vslam_fe* fe, int npairs, const vslam_kp* const* kps1,
                                                     const uint8_t* const* dev_desc1, const int* n1,
                                                     const vslam_kp* const* kps2, const uint8_t* const* dev_desc2,
                                                     const int* n2, int img_w, int img_h,
                                                     float* const* prev_matched, int32_t* const* matches12,
                                                     int window, float nnratio, int check_orientation,
                                                     int* nmatches) {
    return search_init_batch_b(fe, npairs, kps1, dev_desc1, n1, kps2, dev_desc2, n2, int_bounds(img_w, img_h), prev_matched,
                               matches12, window, nnratio, check_orientation, nmatches);
}

extern "C" int vslam_search_for_initialization_batch_ex(vslam_fe* fe, int npairs, const vslam_kp* const* kps1,
                                                        const uint8_t* const* dev_desc1, const int* n1,
                                                        const vslam_kp* const* kps2, const uint8_t* const* dev_desc2,
                                                        const int* n2, const vslam_bounds* b, float* const* prev_matched,
                                                        int32_t* const* matches12, int window, float nnratio,
                                                        int check_orientation, int* nmatches) {
    if (!bounds_ok(b)) {
        g_err = "invalid image bounds";
        return VSLAM_ERR_INVALID;
    }
    return search_init_batch_b(fe, npairs, kps1, dev_desc1, n1, kps2, dev_desc2, n2,
                               SiBounds{b->min_x, b->max_x, b->min_y, b->max_y}, prev_matched, matches12, window, nnratio,
                               check_orientation, nmatches);
}

static int search_init_single_b(vslam_fe* fe, const vslam_kp* kps1, const uint8_t* dev_desc1, int n1, const vslam_kp* kps2,
                                const uint8_t* dev_desc2, int n2, const SiBounds& bnd, float* prev_matched,
                                int32_t* matches12, int window, float nnratio, int check_orientation, int* nmatches) {
    /* the reference tolerates empty frames: nothing to match */
    static const vslam_kp no_kp = {0, 0, 0, 0, 0, 0, 0};
    static const uint8_t* no_desc = (const uint8_t*)&no_kp;
    static float no_prev[2];
    static int32_t no_match[1];
    const vslam_kp* k1 = n1 ? kps1 : &no_kp;
    const vslam_kp* k2 = n2 ? kps2 : &no_kp;
    const uint8_t* d1 = n1 ? dev_desc1 : no_desc;
    const uint8_t* d2 = n2 ? dev_desc2 : no_desc;
    float* pm = n1 ? prev_matched : no_prev;
    int32_t* m = n1 ? matches12 : no_match;
    return search_init_batch_b(fe, 1, &k1, &d1, &n1, &k2, &d2, &n2, bnd, &pm, &m, window, nnratio, check_orientation,
                               nmatches);
}

extern "C" int vslam_search_for_initialization(vslam_fe* fe, const vslam_kp* kps1, const uint8_t* dev_desc1,
                                               int n1, const vslam_kp* kps2, const uint8_t* dev_desc2, int n2,
                                               int img_w, int img_h, float* prev_matched, int32_t* matches12,
                                               int window, float nnratio, int check_orientation,
                                               int* nmatches) {
    return search_init_single_b(fe, kps1, dev_desc1, n1, kps2, dev_desc2, n2, int_bounds(img_w, img_h), prev_matched,
                                matches12, window, nnratio, check_orientation, nmatches);
}

extern "C" int vslam_search_for_initialization_ex(vslam_fe* fe, const vslam_kp* kps1, const uint8_t* dev_desc1, int n1,
                                                  const vslam_kp* kps2, const uint8_t* dev_desc2, int n2,
                                                  const vslam_bounds* b, float* prev_matched, int32_t* matches12,
                                                  int window, float nnratio, int check_orientation, int* nmatches) {
    if (!bounds_ok(b)) {
        g_err = "invalid image bounds";
        return VSLAM_ERR_INVALID;
    }
    return search_init_single_b(fe, kps1, dev_desc1, n1, kps2, dev_desc2, n2, SiBounds{b->min_x, b->max_x, b->min_y, b->max_y},
                                prev_matched, matches12, window, nnratio, check_orientation, nmatches);
}

/* ------------------------------------------------------------------ diagnostics */
static int dbg_buffers(vslam_fe* fe, int n, float** a, float** b, float** c) {
    int rc = fe->d_tmp_desc[1].ensure((size_t)n * 12);
    if (rc) return rc;
    *a = (float*)fe->d_tmp_desc[1];
    *b = *a + n;
    *c = *b + n;
    return VSLAM_OK;
}

extern "C" int vslam_dbg_sincos(vslam_fe* fe, const float* x, int n, float* sin_out, float* cos_out) {
    if (!fe || n < 0 || (n && (!x || !sin_out || !cos_out))) return VSLAM_ERR_INVALID;
    if (!n) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    float *dx, *ds, *dc;
    int rc = dbg_buffers(fe, n, &dx, &ds, &dc);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, fe->stream));
    vk_dbg_sincos(fe->stream, dx, n, ds, dc);
    HIPCHK(hipMemcpyAsync(sin_out, ds, (size_t)n * 4, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(hipMemcpyAsync(cos_out, dc, (size_t)n * 4, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_dbg_logf(vslam_fe* fe, const float* x, int n, float* y) {
    if (!fe || n < 0 || (n && (!x || !y))) return VSLAM_ERR_INVALID;
    if (!n) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    float *dx, *dy, *dz;
    int rc = dbg_buffers(fe, n, &dx, &dy, &dz);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, fe->stream));
    vk_dbg_logf(fe->stream, dx, n, dy);
    HIPCHK(hipMemcpyAsync(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_dbg_fast_atan2(vslam_fe* fe, const float* y, const float* x, int n, int fma, float* deg) {
    if (!fe || n < 0 || (n && (!x || !y || !deg))) return VSLAM_ERR_INVALID;
    if (!n) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    float *dy, *dx, *da;
    int rc = dbg_buffers(fe, n, &dy, &dx, &da);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dy, y, (size_t)n * 4, hipMemcpyHostToDevice, fe->stream));
    HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, fe->stream));
    vk_dbg_atan2(fe->stream, dy, dx, n, fma, da);
    HIPCHK(hipMemcpyAsync(deg, da, (size_t)n * 4, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_dbg_search_init_fallbacks(vslam_fe* fe, int* count) {
    if (!fe || !count) return VSLAM_ERR_INVALID;
    *count = 0;
    if (!fe->d_init_fb) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    HIPCHK(vslam_stream_wait(fe->stream));
    HIPCHK(hipMemcpy(count, fe->d_init_fb, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(fe->d_init_fb, 0, 4));
    return VSLAM_OK;
}

/* rounds / queries / pairs of the replay wave since the last call (k_si_replay's own counters; read-and-reset) */
extern "C" int vslam_dbg_search_init_replay_stats(vslam_fe* fe, int* rounds, int* queries, int* pairs) {
    if (!fe) return VSLAM_ERR_INVALID;
    int v[4] = {0, 0, 0, 0};
    if (fe->d_init_fb) {
        HIPCHK(hipSetDevice(fe->p.device));
        HIPCHK(vslam_stream_wait(fe->stream));
        HIPCHK(hipMemcpy(v, fe->d_init_fb, 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(fe->d_init_fb + 1, 0, 12));
    }
    if (rounds) *rounds = v[1];
    if (queries) *queries = v[2];
    if (pairs) *pairs = v[3];
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ brute-force descriptor matching (k_hamming_*) */
extern "C" int vslam_hamming_top2_batch(vslam_fe* fe, int nprob, const uint8_t* const* dev_q, const int32_t* nq,
                                        const uint8_t* const* dev_t, const int32_t* nt, int32_t* const* idx2,
                                        int32_t* const* dist2) {
    if (!fe || nprob < 0 || nprob > VSLAM_MAX_TOP2_JOBS || (nprob && (!dev_q || !nq || !dev_t || !nt || !idx2 || !dist2))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    Top2Jobs J;
    memset(&J, 0, sizeof(J));
    size_t rows = 0;
    int max_nq = 0, max_nt = 0;
    for (int p = 0; p < nprob; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nt[p] > 65535 || (nq[p] && (!dev_q[p] || !idx2[p] || !dist2[p])) || (nt[p] && !dev_t[p])) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
        J.job[p].q = (const uint32_t*)dev_q[p];
        J.job[p].t = (const uint32_t*)dev_t[p];
        J.job[p].nq = nq[p];
        J.job[p].nt = nt[p];
        J.job[p].row0 = (uint32_t)rows;
        rows += (size_t)nq[p];
        max_nq = std::max(max_nq, nq[p]);
        max_nt = std::max(max_nt, nt[p]);
    }
    if (rows == 0) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    const int nsplit = vk_hamming_top2_batch_split(nprob, max_nq, max_nt);
    int rc;
    if ((rc = fe->d_part.ensure(rows * nsplit * 2))) return rc;
    if ((rc = fe->d_idx2.ensure(rows * 2))) return rc;
    if ((rc = fe->d_dist2.ensure(rows * 2))) return rc;
    if ((rc = fe->h_top2.ensure(rows * 16))) return rc;
    /* a split that lies past a problem's last tile, or a problem without train descriptors, writes nothing: "missing" */
    HIPCHK(hipMemsetAsync(fe->d_part, 0xFF, rows * nsplit * 8, fe->stream));
    vk_hamming_top2_batch(fe->stream, J, nprob, max_nq, (int)rows, nsplit, fe->d_part, fe->d_idx2, fe->d_dist2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fe->h_top2, fe->d_idx2, rows * 8, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(hipMemcpyAsync(fe->h_top2 + rows * 8, fe->d_dist2, rows * 8, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    for (int p = 0; p < nprob; p++) {
        if (!nq[p]) continue;
        memcpy(idx2[p], fe->h_top2 + (size_t)J.job[p].row0 * 8, (size_t)nq[p] * 8);
        memcpy(dist2[p], fe->h_top2 + rows * 8 + (size_t)J.job[p].row0 * 8, (size_t)nq[p] * 8);
    }
    return VSLAM_OK;
}

/* one problem = a batch of one (k_hamming_top2_batch splits the train set over as many workgroups as fill the GPU) */
extern "C" int vslam_hamming_top2(vslam_fe* fe, const uint8_t* dev_q, int nq, const uint8_t* dev_t, int nt,
                                  int32_t* idx2, int32_t* dist2) {
    if (!fe || nq < 0 || nt < 0 || nt > 65535 || (nq && (!dev_q || !idx2 || !dist2)) || (nt && !dev_t)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (nq == 0) return VSLAM_OK;
    const int32_t nq1 = nq, nt1 = nt;
    return vslam_hamming_top2_batch(fe, 1, &dev_q, &nq1, &dev_t, &nt1, &idx2, &dist2);
}

/* enqueue-only form for profilers and pipelines: results stay in the context's device arrays (rows back to back) */
extern "C" int vslam_hamming_top2_batch_dev_async(vslam_fe* fe, int nprob, const uint8_t* const* dev_q, const int32_t* nq,
                                                  const uint8_t* const* dev_t, const int32_t* nt) {
    if (!fe || nprob <= 0 || nprob > VSLAM_MAX_TOP2_JOBS || !dev_q || !nq || !dev_t || !nt) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    Top2Jobs J;
    memset(&J, 0, sizeof(J));
    size_t rows = 0;
    int max_nq = 0, max_nt = 0;
    for (int p = 0; p < nprob; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nt[p] > 65535 || (nq[p] && !dev_q[p]) || (nt[p] && !dev_t[p])) {
            g_err = "invalid arguments";
            return VSLAM_ERR_INVALID;
        }
        J.job[p].q = (const uint32_t*)dev_q[p];
        J.job[p].t = (const uint32_t*)dev_t[p];
        J.job[p].nq = nq[p];
        J.job[p].nt = nt[p];
        J.job[p].row0 = (uint32_t)rows;
        rows += (size_t)nq[p];
        max_nq = std::max(max_nq, nq[p]);
        max_nt = std::max(max_nt, nt[p]);
    }
    if (rows == 0) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    const int nsplit = vk_hamming_top2_batch_split(nprob, max_nq, max_nt);
    if (fe->d_part.count() < rows * nsplit * 2 || fe->d_idx2.count() < rows * 2 || fe->d_dist2.count() < rows * 2) { /* sized by a previous vslam_hamming_top2_batch */
        g_err = "vslam_hamming_top2_batch_dev_async: call vslam_hamming_top2_batch with these sizes first (it allocates)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipMemsetAsync(fe->d_part, 0xFF, rows * nsplit * 8, fe->stream));
    vk_hamming_top2_batch(fe->stream, J, nprob, max_nq, (int)rows, nsplit, fe->d_part, fe->d_idx2, fe->d_dist2);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

/* Frame::ComputeStereoFishEyeMatches (frame.cpp:1149-1174), the descriptor half: BFmatcher.knnMatch(left rows
 * [mono_left, n_left), right rows [mono_right, n_right), k = 2) + Lowe's ratio test.  What follows in the reference --
 * KannalaBrandt8::TriangulateMatches per surviving pair (:1176-1188) -- is the camera model's and stays with the caller. */
extern "C" int vslam_stereo_fisheye_candidates(vslam_fe* fe, const uint8_t* dev_desc_left, int n_left, int mono_left,
                                               const uint8_t* dev_desc_right, int n_right, int mono_right,
                                               int32_t* left_to_right, int32_t* best_dist, int32_t* second_dist,
                                               int* n_candidates) {
    if (!fe || !left_to_right || n_left < 0 || n_right < 0 || mono_left < 0 || mono_right < 0 || mono_left > n_left ||
        mono_right > n_right || (n_left && !dev_desc_left) || (n_right && !dev_desc_right)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    for (int i = 0; i < n_left; i++) {
        left_to_right[i] = -1;
        if (best_dist) best_dist[i] = -1;
        if (second_dist) second_dist[i] = -1;
    }
    if (n_candidates) *n_candidates = 0;
    const int nq = n_left - mono_left, nt = n_right - mono_right;
    if (nq == 0) return VSLAM_OK;
    std::vector<int32_t> idx2((size_t)nq * 2), dist2((size_t)nq * 2);
    int rc = vslam_hamming_top2(fe, dev_desc_left + (size_t)mono_left * 32, nq, dev_desc_right + (size_t)mono_right * 32, nt,
                                idx2.data(), dist2.data());
    if (rc != VSLAM_OK) return rc;
    int nc = 0;
    for (int q = 0; q < nq; q++) {
        if (idx2[2 * q] < 0 || idx2[2 * q + 1] < 0) continue; /* (*it).size() >= 2 */
        /* DMatch::distance is a float; `distance * 0.7` is float x double: the comparison happens in double */
        const float d0 = (float)dist2[2 * q], d1 = (float)dist2[2 * q + 1];
        if (!((double)d0 < (double)d1 * 0.7)) continue;
        left_to_right[q + mono_left] = idx2[2 * q] + mono_right;
        if (best_dist) best_dist[q + mono_left] = dist2[2 * q];
        if (second_dist) second_dist[q + mono_left] = dist2[2 * q + 1];
        nc++;
    }
    if (n_candidates) *n_candidates = nc; /* the reference's descMatches */
    return VSLAM_OK;
}

extern "C" int vslam_hamming_matrix(vslam_fe* fe, const uint8_t* dev_q, int nq, const uint8_t* dev_t, int nt,
                                    uint8_t* out) {
    if (!fe || nq < 0 || nt < 0 || (nq && nt && (!dev_q || !dev_t || !out))) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    if (nq == 0 || nt == 0) return VSLAM_OK;
    HIPCHK(hipSetDevice(fe->p.device));
    int rc;
    if ((rc = fe->d_dmat.ensure((size_t)nq * nt))) return rc;
    vk_hamming_matrix(fe->stream, dev_q, nq, dev_t, nt, fe->d_dmat);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, fe->d_dmat, (size_t)nq * nt, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}
