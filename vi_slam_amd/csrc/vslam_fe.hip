/* vslam_fe.hip -- the extraction pipeline behind include/vslam_fe.h: the launch sequence of a pass, its capture into a
 * graph, waiting and delivery.  (The context's life: vslam_context.hip; host images into level 0: vslam_upload.hip.)
 *
 * Per batch of image slots the extractor issues, on ONE stream:
 *     front (upload, pyramid, FAST)  ->  blur, select  ->  describe + undistort  ->  deliver
 * Only the selection stage (FExtractor::DistributeOctTree) knows where the quadtree runs: k_octree_v4 + k_assign_out on the
 * device, or -- VSLAM_FLAG_HOST_OCTREE, or a node list too long for LDS -- candidates fetched to the host, one task per
 * (slot, level) on a small worker pool while the blur runs, and the same per-slot lists and counts block uploaded.
 */
#include "vslam_ctx.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

/* ------------------------------------------------------------------ extraction */
static void decode_candidates(vslam_fe* fe, int s, int l) {
    const int ncells = (int)fe->cells.size();
    const size_t hdr_bytes = 8 + (size_t)ncells * sizeof(CellOut);
    const uint8_t* base = fe->h_cand + (size_t)s * fe->cand_stride;
    const CellOut* co = (const CellOut*)(base + 8);
    const uint32_t* cand = (const uint32_t*)(base + hdr_bytes);
    std::vector<vslam::Cand>& cl = fe->cand_level[(size_t)s * fe->p.nlevels + l];
    cl.clear();
    for (int c = fe->level_cell_first[l]; c < fe->level_cell_first[l + 1]; c++) {
        const uint32_t* q = cand + co[c].base;
        for (uint32_t k = 0; k < co[c].count; k++) {
            vslam::Cand cd;
            cd.x = (int16_t)(q[k] & 0xFFF);
            cd.y = (int16_t)((q[k] >> 12) & 0xFFF);
            cd.response = (uint8_t)(q[k] >> 24);
            cl.push_back(cd);
        }
    }
}

/* level 0 of slots 0..nimg-1 is read from the context's own pyramid */
static void src_at_slots(vslam_fe* fe, int nimg) {
    for (int s = 0; s < nimg; s++) {
        fe->src.l0[s] = fe->d_pyr + (size_t)s * fe->slot_stride + fe->geom.lv[0].off;
        fe->src.pitch0[s] = (uint32_t)fe->geom.lv[0].pitch;
    }
}

/* steps shared by both quadtree placements: level 0, pyramid, FAST */
static int enqueue_front(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int on_device) {
    const vslam_fe_params& p = fe->p;
    const int L = p.nlevels;
    hipStream_t st = fe->stream;
    if (on_device == VSLAM_IMGS_DEVICE) {
        BatchSrc ds;
        for (int s = 0; s < nimg; s++) {
            if (!imgs[s]) {
                g_err = "null image";
                return VSLAM_ERR_INVALID;
            }
            ds.l0[s] = fe->src.l0[s] = imgs[s];
            ds.pitch0[s] = fe->src.pitch0[s] = (uint32_t)pitch;
        }
        if (fe->pix_fmt != VSLAM_PIX_GRAY8) { /* colour: not zero copy, the gray image lives in the context's level 0 */
            vk_gray_images(st, ds, fe->d_pyr, fe->slot_stride, fe->geom.lv[0].off, fe->geom.lv[0].pitch, p.width, p.height, nimg,
                           0, fe->pix_fmt, fe->gray_shift, fe->tune);
            src_at_slots(fe, nimg);
        }
    } else {
        if (on_device != VSLAM_IMGS_STAGED) { /* staged: vslam_fe_stage_images_async put them there */
            int rc = vslam_upload_host_rows(fe, nimg, imgs, pitch, on_device);
            if (rc) return rc;
        }
        src_at_slots(fe, nimg);
    }
    fe->last_nimg = nimg;
    fe->cand_on_host = false;
    /* per-slot candidate header (total, overflow) and the device-quadtree error word: one tiny kernel instead
     * of two runtime memsets */
    int32_t* d_errw = fe->dev_octree ? fe->d_counts + (size_t)fe->B * 4 : nullptr;
    if (fe->pyr_groups.empty()) vk_reset_headers(st, fe->d_cand, fe->cand_stride, nimg, d_errw); /* else: the first pyramid launch does it */
    const bool prof = fe->profiling;
    if (prof) HIPCHK(hipEventRecord(fe->ev_prof[0], st));
    bool first_group = true;
    for (const auto& g : (fe->pyr_resident_hint && !fe->pyr_groups_resident.empty()) ? fe->pyr_groups_resident : fe->pyr_groups) {
        vk_pyramid_group(st, fe->d_pyr, fe->slot_stride, fe->src, g.dev, g.lds_bytes, g.fit, nimg,
                         first_group ? fe->d_cand : nullptr, fe->cand_stride, first_group ? d_errw : nullptr);
        first_group = false;
    }
    for (int l = 1; l < L && fe->pyr_groups.empty(); l++) {
        if (fe->d_quads[l])
            vk_resize_level_v2(st, fe->d_pyr, fe->slot_stride, fe->src, fe->geom.lv[l - 1], fe->geom.lv[l], l - 1,
                               fe->d_qbase[l], fe->d_quads[l], fe->d_ytab[l], fe->d_yb[l], nimg);
        else
            vk_resize_level(st, fe->d_pyr, fe->slot_stride, fe->src, fe->geom.lv[l - 1], fe->geom.lv[l], l - 1,
                            fe->d_xtab[l], fe->d_xa[l], fe->d_ytab[l], fe->d_yb[l], nimg);
    }
    if (prof) HIPCHK(hipEventRecord(fe->ev_prof[1], st));
    if (fe->fast_gate && fe->fast_gate->ev_fast) HIPCHK(hipStreamWaitEvent(st, fe->fast_gate->ev_fast, 0));
    /* vslam_tuning.fast_kernel: 4 = one workgroup per band of cells (default for batches: 17 % fewer instructions, every
     * image byte fetched once), 3 = one per cell (default for contexts of one or two images, where the launch is a frame's
     * latency: 15 instead of 21 us, four times as many and shorter workgroups) */
    if (fe->nbands > 0 && tune_or(fe->tune.fast_kernel, fe->B <= 2 ? 3 : 4) != 3)
        vk_fast_bands(st, fe->d_pyr, fe->slot_stride, fe->src, fe->geom, fe->d_bands, fe->nbands, fe->d_band_classes, fe->d_cells,
                      (int)fe->cells.size(), fe->d_cand, fe->cand_stride, p.ini_th_fast, p.min_th_fast, fe->band_max_wh, fe->band_max_iw, nimg);
    else
        vk_fast_cells_v3(st, fe->d_pyr, fe->slot_stride, fe->src, fe->geom, fe->d_cells, (int)fe->cells.size(), fe->d_cand,
                         fe->cand_stride, p.ini_th_fast, p.min_th_fast, fe->tile_rows, fe->tile_pitch, fe->max_px, nimg);
    if (fe->fast_gated_by_someone && fe->ev_fast) HIPCHK(hipEventRecord(fe->ev_fast, st));
    if (prof) HIPCHK(hipEventRecord(fe->ev_prof[2], st));
    return VSLAM_OK;
}

static int fetch_candidates(vslam_fe* fe, int nimg) {
    /* header + cell table + candidates of every slot: the cells own fixed segments, so the used entries are scattered and
     * the whole region travels */
    const size_t hdr_bytes = 8 + fe->cells.size() * sizeof(CellOut);
    HIPCHK(hipMemcpy2DAsync(fe->h_cand, fe->cand_stride, fe->d_cand, fe->cand_stride, hdr_bytes + (size_t)fe->cand_cap * 4,
                            nimg, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(hipEventRecord(fe->ev_cand, fe->stream));
    return VSLAM_OK;
}

static int wait_candidates(vslam_fe* fe, int nimg) {
    HIPCHK(hipEventSynchronize(fe->ev_cand));
    for (int s = 0; s < nimg; s++) {
        const uint32_t* hdr = (const uint32_t*)(fe->h_cand + (size_t)s * fe->cand_stride);
        if (hdr[1]) {
            g_err = "FAST candidate buffer overflow";
            return VSLAM_ERR_CAPACITY;
        }
    }
    fe->cand_on_host = true;
    return VSLAM_OK;
}

static int enqueue_blur(vslam_fe* fe, int nimg) {
    if (fe->profiling) HIPCHK(hipEventRecord(fe->ev_prof[3], fe->stream));
    vk_blur7_v2(fe->stream, fe->d_pyr, fe->slot_stride, fe->src, fe->geom, fe->d_blur, fe->d_blur_tasks,
                fe->n_blur_tasks, fe->taps, fe->blur_rows, nimg);
    if (fe->profiling) HIPCHK(hipEventRecord(fe->ev_prof[4], fe->stream));
    return VSLAM_OK;
}

/* Selection on the host (VSLAM_FLAG_HOST_OCTREE, or a node list that does not fit LDS): fetch the candidates, distribute
 * them on the worker pool while the blur runs, and upload exactly what k_assign_out leaves behind -- the SelKp list of
 * slot s at d_sel + s * cap and the counts block.  What it finds wrong is returned here, at enqueue time. */
static int select_host(vslam_fe* fe, int nimg, int lap0, int lap1) {
    const int L = fe->p.nlevels;
    hipStream_t st = fe->stream;
    int rc = fetch_candidates(fe, nimg);
    if (rc == VSLAM_OK) rc = enqueue_blur(fe, nimg); /* runs while the host distributes */
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = wait_candidates(fe, nimg))) return rc;
    std::atomic<int> bad(0);
    fe->pool->parallel_for(nimg * L, [&](int task) {
        const int s = task / L, l = task % L;
        decode_candidates(fe, s, l);
        const std::vector<vslam::Cand>& cl = fe->cand_level[(size_t)s * L + l];
        const LevelGeom& g = fe->geom.lv[l];
        if (!vslam::distribute_octree(cl.data(), (int)cl.size(), g.w - 2 * VSLAM_FAST_BORDER,
                                      g.h - 2 * VSLAM_FAST_BORDER, fe->tab.quota[l],
                                      fe->sel_level[(size_t)s * L + l]))
            bad++;
    });
    if (bad.load()) {
        g_err = "DistributeOctTree: nIni == 0";
        return VSLAM_ERR_UNSUPPORTED;
    }
    /* output order (fextractor.cpp:1071-1129): level-major, lapping-area keypoints from the tail */
    for (int s = 0; s < nimg; s++) {
        int nk = 0;
        for (int l = 0; l < L; l++) nk += (int)fe->sel_level[(size_t)s * L + l].size();
        if (nk > fe->cap) {
            g_err = "internal keypoint capacity exceeded";
            return VSLAM_ERR_CAPACITY;
        }
        SelKp* sel = fe->h_sel + (size_t)s * fe->cap;
        int monoIndex = 0, stereoIndex = nk - 1;
        for (int l = 0; l < L; l++) {
            const float scale = fe->tab.scale[l];
            for (const vslam::Cand& c : fe->sel_level[(size_t)s * L + l]) {
                const int lx = c.x + VSLAM_FAST_BORDER, ly = c.y + VSLAM_FAST_BORDER;
                float px = (float)lx;
                if (l != 0) px = px * scale;
                SelKp k;
                k.x = (uint16_t)lx;
                k.y = (uint16_t)ly;
                k.level = (uint8_t)l;
                k.slot = (uint8_t)s;
                k.response = c.response;
                k.pad = 0;
                k.out = (px >= (float)lap0 && px <= (float)lap1) ? (uint32_t)stereoIndex-- : (uint32_t)monoIndex++;
                *sel++ = k;
            }
        }
        fe->h_counts[s * 4] = nk;
        fe->h_counts[s * 4 + 1] = monoIndex;
        fe->h_counts[s * 4 + 2] = 0; /* the device quadtree's deep-level mask */
    }
    fe->h_counts[fe->B * 4] = 0; /* error word */
    HIPCHK(hipMemcpyAsync(fe->d_counts, fe->h_counts, (size_t)(fe->B * 4 + 4) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(fe->d_sel, fe->h_sel, (size_t)nimg * fe->cap * sizeof(SelKp), hipMemcpyHostToDevice, st));
    if (fe->profiling) { /* nothing of this stage runs on the device: a zero-length span */
        HIPCHK(hipEventRecord(fe->ev_prof[7], st));
        HIPCHK(hipEventRecord(fe->ev_prof[8], st));
    }
    return VSLAM_OK;
}

/* selection on the device: nothing returns to the host until the results do */
static int select_dev(vslam_fe* fe, int nimg, int lap0, int lap1) {
    hipStream_t st = fe->stream;
    int32_t* d_err = fe->d_counts + (size_t)fe->B * 4;
    const int rc = enqueue_blur(fe, nimg);
    if (rc) return rc;
    if (fe->profiling) HIPCHK(hipEventRecord(fe->ev_prof[7], st));
    vk_octree(st, fe->d_cand, fe->cand_stride, (int)fe->cells.size(), fe->oct, fe->d_pts,
              fe->d_oct_sorted, (size_t)fe->cand_cap, fe->d_sel_xyr, fe->d_sel_cnt, d_err, fe->p.nlevels, nimg,
              fe->d_oct_redo, fe->tune.oct_regkeys, fe->oct_threads);
    vk_assign_out(st, fe->oct, fe->geom, fe->d_sel_xyr, fe->d_sel_cnt, lap0, lap1, fe->d_sel, fe->d_counts, fe->cap,
                  d_err, nimg, fe->d_oct_redo);
    if (fe->profiling) HIPCHK(hipEventRecord(fe->ev_prof[8], st));
    return VSLAM_OK;
}

/* blur and selection, then what both placements share: orientation + descriptors of the per-slot lists, undistortion */
static int enqueue_back(vslam_fe* fe, int nimg, int lap0, int lap1) {
    hipStream_t st = fe->stream;
    const bool prof = fe->profiling;
    int rc = fe->dev_octree ? select_dev(fe, nimg, lap0, lap1) : select_host(fe, nimg, lap0, lap1);
    if (rc) return rc;
    if (prof) HIPCHK(hipEventRecord(fe->ev_prof[5], st));
    vk_orient_describe_dev(st, fe->d_pyr, fe->d_blur, fe->slot_stride, fe->src, fe->geom, fe->d_sel, fe->d_counts,
                           fe->d_pattern, fe->d_kps, fe->d_desc, fe->cap, (fe->p.flags & VSLAM_FLAG_ATAN_FMA) ? 1 : 0,
                           nimg, fe->tune.desc_kpw >= 0 ? fe->tune.desc_kpw : fe->desc_kpw_hint);
    rc = vslam_enqueue_undistort(fe, nimg); /* Frame::UndistortKeyPoints, if a camera asks for it */
    if (rc) return rc;
    if (prof) HIPCHK(hipEventRecord(fe->ev_prof[6], st));
    HIPCHK(hipGetLastError());
    return VSLAM_OK; /* counts travel to the host with the results (deliver) */
}

/* VSLAM_HOST_PROF=1: host-side wall time per API phase, printed by vslam_fe_destroy (diagnostics only) */
static double g_hp[6];
static long g_hp_n;
static const bool g_hp_on = vslam_process_tuning().host_prof == 1; /* process-wide */
static inline double hp_now() {
    return g_hp_on ? std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch())
                         .count()
                   : 0.0;
}
void vslam_host_prof_report() {
    if (!g_hp_on || !g_hp_n) return;
    fprintf(stderr, "[vslam host prof] per call (us): front %.1f back %.1f d2h-enqueue %.1f sync %.1f deliver %.1f (n=%ld)\n",
            g_hp[0] / g_hp_n, g_hp[1] / g_hp_n, g_hp[2] / g_hp_n, g_hp[3] / g_hp_n, g_hp[4] / g_hp_n, g_hp_n);
    g_hp_n = 0;
    for (double& v : g_hp) v = 0;
}

static int enqueue_extract_plain(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int on_device,
                                 int lap0, int lap1, int want_host) {
    const double t0 = hp_now();
    int rc = enqueue_front(fe, nimg, imgs, pitch, on_device);
    if (rc) return rc;
    const double t1 = hp_now();
    rc = enqueue_back(fe, nimg, lap0, lap1);
    if (rc) return rc;
    const double t2 = hp_now();
    g_hp[0] += t1 - t0;
    g_hp[1] += t2 - t1;
    g_hp_n++;
    struct D2hTimer {
        double t;
        ~D2hTimer() { g_hp[2] += hp_now() - t; }
    } d2h_timer{t2};
    /* results go to pinned host memory by a kernel (whole blocks: the host does not know the counts yet) */
    if (nimg == fe->B && want_host == 2 && fe->res_init_bytes != 0)
        return VSLAM_OK; /* deferred: vslam_search_init_dev_async (or the wait) sends the block; vslam_enqueue_extract sets the flag */
    if (nimg == fe->B && want_host) /* a full batch: counts, keypoints and descriptors are one contiguous block -> ONE transfer */
        return vslam_deliver_block(fe, 0);
    CopyRanges R;
    memset(&R, 0, sizeof(R));
    R.dst[R.n] = fe->h_counts;
    R.src[R.n] = fe->d_counts;
    R.bytes[R.n++] = (size_t)(fe->B * 4 + 4) * 4;
    if (want_host) {
        R.dst[R.n] = fe->h_kps;
        R.src[R.n] = fe->d_kps;
        R.bytes[R.n++] = (size_t)nimg * fe->cap * sizeof(vslam_kp);
        R.dst[R.n] = fe->h_desc;
        R.src[R.n] = fe->d_desc;
        R.bytes[R.n++] = (size_t)nimg * fe->cap * 32;
    }
    vslam_count_delivery(fe, vk_copy_ranges(fe->stream, R, fe->tune), R);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

/* want_host: 0 results stay in HBM (counts still reach the host), 1 delivered by this pass, 2 delivery DEFERRED to the
 * device SearchForInitialization that follows on this context (one transfer for both); if none follows, the wait delivers */
static int enqueue_extract_impl(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int on_device, int lap0,
                                int lap1, int want_host) {
    HIPCHK(hipSetDevice(fe->p.device));
    if (on_device == VSLAM_IMGS_HOST) {
        int rc = vslam_stage_host_images(fe, nimg, imgs, pitch);
        if (rc) return rc;
    }
    if (on_device == VSLAM_IMGS_HOST || on_device == VSLAM_IMGS_PINNED) {
        int rc = vslam_stage_ensure(fe, on_device == VSLAM_IMGS_PINNED ? pitch : vslam_host_stage_pitch(fe), nimg);
        if (rc) return rc;
    }
    /* Host-image passes of one shape replay a captured HIP graph: every kernel argument of such a pass is fixed
     * (staging, pyramid and result buffers belong to the context), so the ~20 launches become one hipGraphLaunch. */
    const bool graphable = fe->use_graph && on_device != VSLAM_IMGS_DEVICE && fe->dev_octree && !fe->profiling;
    if (!graphable) return enqueue_extract_plain(fe, nimg, imgs, pitch, on_device, lap0, lap1, want_host);
    long long key = ((long long)nimg << 48) ^ ((long long)(uint16_t)lap0 << 32) ^ ((long long)(uint16_t)lap1 << 16) ^
                    (long long)(want_host & 3) ^ ((long long)(lap0 >> 16) << 40) ^ ((long long)(lap1 >> 16) << 24) ^
                    ((long long)on_device << 56); /* host / pinned / staged passes capture different launches */
    if (on_device == VSLAM_IMGS_HOST && fe->h_img_pitch != (size_t)fe->geom.lv[0].pitch) key ^= 1ll << 59; /* dense staging rows */
    if (fe->pyr_resident_hint && !fe->pyr_groups_resident.empty()) key ^= 1ll << 58; /* the entry's pyramid plan is part of the capture */
    if (on_device == VSLAM_IMGS_PINNED) {
        /* the caller's pointers are kernel arguments of the captured pull: a different set of images is a different
         * graph (a capture-card ring of a few buffers per context hits the cache every time) */
        unsigned long long hsh = 0x9E3779B97F4A7C15ull ^ (unsigned long long)pitch;
        for (int s = 0; s < nimg; s++) hsh = (hsh ^ (unsigned long long)(uintptr_t)imgs[s]) * 0x100000001B3ull;
        key ^= (long long)(hsh | 2ull);
    }
    const bool same_imgs = on_device != VSLAM_IMGS_PINNED ||
                           (fe->graph_pitch == pitch && !memcmp(fe->graph_imgs, imgs, (size_t)nimg * sizeof(imgs[0])));
    if (fe->graph_exec && fe->graph_key == key && fe->graph_lap0 == lap0 && fe->graph_lap1 == lap1 && same_imgs) {
        fe->last_nimg = nimg;
        fe->cand_on_host = false;
        /* what enqueue_front records on a plain pass: later NON-captured consumers (stereo refinement,
         * vslam_fe_level_copy level 0) read fe->src, which a device-image pass in between may have pointed at the
         * caller's (by now possibly freed) images */
        src_at_slots(fe, nimg);
        HIPCHK(hipGraphLaunch(fe->graph_exec, fe->stream));
        fe->n_deliveries += fe->graph_deliveries;
        fe->n_delivery_bytes += fe->graph_delivery_bytes;
        return VSLAM_OK;
    }
    if (fe->graph_exec) {
        hipGraphExecDestroy(fe->graph_exec);
        fe->graph_exec = nullptr;
    }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(fe->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        fe->use_graph = false; /* capture unavailable: plain launches from now on */
        return enqueue_extract_plain(fe, nimg, imgs, pitch, on_device, lap0, lap1, want_host);
    }
    const unsigned long long del0 = fe->n_deliveries, delb0 = fe->n_delivery_bytes;
    int rc = enqueue_extract_plain(fe, nimg, imgs, pitch, on_device, lap0, lap1, want_host);
    const hipError_t ce = hipStreamEndCapture(fe->stream, &graph);
    fe->graph_deliveries = fe->n_deliveries - del0; /* what one replay of this graph sends to the host */
    fe->graph_delivery_bytes = fe->n_delivery_bytes - delb0;
    fe->n_deliveries = del0; /* the capture itself ran nothing */
    fe->n_delivery_bytes = delb0;
    if (rc != VSLAM_OK || ce != hipSuccess || !graph ||
        hipGraphInstantiate(&fe->graph_exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) hipGraphDestroy(graph);
        fe->graph_exec = nullptr;
        fe->use_graph = false;
        if (rc != VSLAM_OK) return rc;
        return enqueue_extract_plain(fe, nimg, imgs, pitch, on_device, lap0, lap1, want_host);
    }
    hipGraphDestroy(graph);
    fe->graph_key = key;
    fe->graph_pitch = pitch;
    /* only a pinned pass bakes the caller's pointers into the graph; STAGED passes may come with imgs == NULL */
    if (on_device == VSLAM_IMGS_PINNED) memcpy(fe->graph_imgs, imgs, (size_t)nimg * sizeof(imgs[0]));
    else memset(fe->graph_imgs, 0, sizeof(fe->graph_imgs));
    fe->graph_lap0 = lap0;
    fe->graph_lap1 = lap1;
    HIPCHK(hipGraphLaunch(fe->graph_exec, fe->stream));
    fe->n_deliveries += fe->graph_deliveries;
    fe->n_delivery_bytes += fe->graph_delivery_bytes;
    return VSLAM_OK;
}

int vslam_enqueue_extract(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int on_device,
                          int lap0, int lap1, int want_host) {
    fe->last_rgbd = false; /* vslam_frame_rgbd_batch_async sets it behind its depth gather */
    const int rc = enqueue_extract_impl(fe, nimg, imgs, pitch, on_device, lap0, lap1, want_host);
    /* set on every path, a replayed graph included (the captured pass of want_host = 2 holds no copy) */
    fe->deliver_deferred = rc == VSLAM_OK && want_host == 2 && nimg == fe->B && fe->res_init_bytes != 0;
    return rc;
}

int vslam_finish_extract(vslam_fe* fe, int nimg) {
    hipStream_t st = fe->stream;
    if (fe->deliver_deferred) { /* a deferred delivery that no matcher call picked up */
        fe->deliver_deferred = false;
        const int rc = vslam_deliver_block(fe, 0);
        if (rc) return rc;
    }
    const double t_sync = hp_now();
    HIPCHK(vslam_stream_wait(st));
    g_hp[3] += hp_now() - t_sync;
    const int32_t err = fe->h_counts[(size_t)fe->B * 4];
    if (err & 1) {
        g_err = "FAST candidate buffer overflow (or > 65535 candidates on one level)";
        return VSLAM_ERR_CAPACITY;
    }
    if (err & 2) {
        g_err = "internal keypoint capacity exceeded";
        return VSLAM_ERR_CAPACITY;
    }
    for (int s = 0; s < nimg; s++) {
        fe->n_out[s] = fe->h_counts[s * 4];
        fe->mono_out[s] = fe->h_counts[s * 4 + 1];
        fe->oct_last_mask[s] = (uint32_t)fe->h_counts[s * 4 + 2];
        fe->oct_deep += (unsigned)__builtin_popcount(fe->oct_last_mask[s]);
    }
    if (fe->dev_octree) fe->oct_problems += (unsigned long long)nimg * fe->p.nlevels; /* problems distributed on the device */
    if (fe->profiling) {
        float ms;
        static const int span[5][2] = {{0, 1}, {1, 2}, {3, 4}, {5, 6}, {7, 8}};
        for (int i = 0; i < 5; i++) {
            HIPCHK(hipEventElapsedTime(&ms, fe->ev_prof[span[i][0]], fe->ev_prof[span[i][1]]));
            fe->prof_ms[i] += ms;
        }
        fe->prof_batches++;
        fe->prof_images += nimg;
    }
    return VSLAM_OK;
}

int vslam_deliver(vslam_fe* fe, int nimg, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                  int* mono_index) {
    struct DeliverTimer {
        double t;
        ~DeliverTimer() { g_hp[4] += hp_now() - t; }
    } deliver_timer{hp_now()};
    for (int s = 0; s < nimg; s++) {
        if (kps && desc) {
            if (fe->n_out[s] > cap) {
                g_err = "caller keypoint capacity too small";
                return VSLAM_ERR_CAPACITY;
            }
            if (fe->n_out[s]) {
                memcpy(kps[s], fe->h_kps + (size_t)s * fe->cap, (size_t)fe->n_out[s] * sizeof(vslam_kp));
                memcpy(desc[s], fe->h_desc + (size_t)s * fe->cap * 32, (size_t)fe->n_out[s] * 32);
            }
        }
        if (n) n[s] = fe->n_out[s];
        if (mono_index) mono_index[s] = fe->mono_out[s];
    }
    return VSLAM_OK;
}

extern "C" int vslam_fe_extract_batch(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch,
                                      int imgs_on_device, int lap0, int lap1, vslam_kp* const* kps,
                                      uint8_t* const* desc, int cap, int* n, int* mono_index) {
    if (!fe || (!imgs && imgs_on_device != VSLAM_IMGS_STAGED) || nimg < 1 || nimg > fe->B ||
        (pitch < vslam_row_bytes(fe) && imgs_on_device != VSLAM_IMGS_STAGED) || imgs_on_device < 0 ||
        imgs_on_device > VSLAM_IMGS_STAGED) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_enqueue_extract(fe, nimg, imgs, pitch, imgs_on_device, lap0, lap1, kps && desc);
    if (rc == VSLAM_OK) rc = vslam_finish_extract(fe, nimg);
    if (rc != VSLAM_OK) {
        hipStreamSynchronize(fe->stream);
        return rc;
    }
    return vslam_deliver(fe, nimg, kps, desc, cap, n, mono_index);
}

/* split form: enqueue everything (no host synchronisation in the device-quadtree path), collect later */
extern "C" int vslam_fe_extract_batch_async(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch,
                                            int imgs_on_device, int lap0, int lap1, int want_host) {
    if (!fe || (!imgs && imgs_on_device != VSLAM_IMGS_STAGED) || nimg < 1 || nimg > fe->B ||
        (pitch < vslam_row_bytes(fe) && imgs_on_device != VSLAM_IMGS_STAGED) || imgs_on_device < 0 ||
        imgs_on_device > VSLAM_IMGS_STAGED) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_enqueue_extract(fe, nimg, imgs, pitch, imgs_on_device, lap0, lap1, want_host < 0 ? 0 : want_host > 2 ? 1 : want_host);
    if (rc != VSLAM_OK) hipStreamSynchronize(fe->stream);
    return rc;
}

extern "C" int vslam_fe_extract_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                                     int* mono_index) {
    if (!fe || fe->last_nimg < 1) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_finish_extract(fe, fe->last_nimg);
    if (rc != VSLAM_OK) return rc;
    return vslam_deliver(fe, fe->last_nimg, kps, desc, cap, n, mono_index);
}

extern "C" int vslam_fe_extract(vslam_fe* fe, const uint8_t* img, size_t pitch, int lap0, int lap1,
                                vslam_kp* kps, uint8_t* desc, int cap, int* n, int* mono_index) {
    if (!fe || !img || !kps || !desc || !n) {
        g_err = "invalid arguments";
        if (mono_index) *mono_index = -1; /* FExtractor::compute returns -1 on an empty image */
        return VSLAM_ERR_INVALID;
    }
    const uint8_t* imgs[1] = {img};
    vslam_kp* k[1] = {kps};
    uint8_t* d[1] = {desc};
    return vslam_fe_extract_batch(fe, 1, imgs, pitch, 0, lap0, lap1, k, d, cap, n, mono_index);
}

extern "C" int vslam_fe_candidates(vslam_fe* fe, int slot, int level, vslam_kp* out, int cap) {
    if (!fe || slot < 0 || slot >= fe->B || level < 0 || level >= fe->p.nlevels || slot >= fe->last_nimg)
        return VSLAM_ERR_INVALID;
    if (!fe->cand_on_host) { /* device quadtree: the candidates never left HBM; fetch them now */
        HIPCHK(hipSetDevice(fe->p.device));
        int rc = fetch_candidates(fe, fe->last_nimg);
        if (rc == VSLAM_OK) rc = wait_candidates(fe, fe->last_nimg);
        if (rc) return rc;
    }
    decode_candidates(fe, slot, level);
    const std::vector<vslam::Cand>& cl = fe->cand_level[(size_t)slot * fe->p.nlevels + level];
    for (int i = 0; i < (int)cl.size() && i < cap && out; i++) {
        out[i].x = (float)cl[i].x;
        out[i].y = (float)cl[i].y;
        out[i].size = 7.f;
        out[i].angle = -1.f;
        out[i].response = (float)cl[i].response;
        out[i].octave = 0;
        out[i].class_id = -1;
    }
    return (int)cl.size();
}
