/* vslam_context.hip -- the life of a vslam_fe context: the error string, vslam_fe_create in steps and vslam_fe_destroy,
 * tuning, tables and statistics, the stream / event / gate entry points, profiling, and the accessors of the slots'
 * buffers.  What a context owns is written down in its members (vslam_ctx.h, vslam_mem.h). */
#include "vslam_ctx.h"

#include <algorithm>
#include <mutex>
#include <cstdio>
#include <cstdlib>

void vslam_host_prof_report();

std::string& vslam_err() {
    static thread_local std::string e;
    return e;
}
extern "C" const char* vslam_last_error(void) { return vslam_err().c_str(); }

static std::mutex g_gate_mu; /* the gate links between contexts (set / destroy may come from different threads) */

static void gate_unlink(vslam_fe* fe) { /* g_gate_mu held */
    if (fe->fast_gate) {
        auto& w = fe->fast_gate->gate_waiters;
        w.erase(std::remove(w.begin(), w.end(), fe), w.end());
        fe->fast_gate = nullptr;
    }
}

/* what has an order or a lock; every allocation is a member that frees itself */
static void free_ctx(vslam_fe* fe) {
    if (!fe) return;
    if (fe->stream) hipStreamSynchronize(fe->stream);
    delete fe->pool;
    if (fe->graph_exec) hipGraphExecDestroy(fe->graph_exec);
    {   /* a destroyed context gates nobody: its waiters run un-gated from now on */
        std::lock_guard<std::mutex> lk(g_gate_mu);
        gate_unlink(fe);
        for (vslam_fe* w : fe->gate_waiters) w->fast_gate = nullptr;
        fe->gate_waiters.clear();
    }
    if (fe->stream) hipStreamDestroy(fe->stream);
    delete fe; /* buffers and events go with their members (vslam_mem.h) */
}

extern "C" void vslam_fe_destroy(vslam_fe* fe) {
    if (fe) hipSetDevice(fe->p.device);
    vslam_host_prof_report();
    free_ctx(fe);
}

/* ---- vslam_fe_create in steps, called in this order by create_impl; what a failed step leaves behind goes with the context */

/* constructor tables, level sizes / pitches / offsets (level 0 staging included at offset 0), keypoint capacity, pyramids */
static int create_geometry(vslam_fe* fe) {
    const vslam_fe_params& p = fe->p;
    vslam::build_tables(p.nfeatures, p.scale_factor, p.nlevels, fe->tab);
    fe->B = p.max_batch;
    static const int32_t def_taps[7] = {18, 34, 48, 56, 48, 34, 18};
    bool zero = true;
    for (int i = 0; i < 7; i++) zero = zero && p.gauss_taps[i] == 0;
    for (int i = 0; i < 7; i++) fe->taps[i] = zero ? def_taps[i] : p.gauss_taps[i];

    memset(&fe->geom, 0, sizeof(fe->geom));
    fe->geom.nlevels = p.nlevels;
    int lws[VSLAM_MAX_LEVELS], lhs[VSLAM_MAX_LEVELS];
    size_t off = 0;
    for (int l = 0; l < p.nlevels; l++) {
        int lw, lh;
        vslam::level_size(fe->tab, p.width, p.height, l, &lw, &lh);
        LevelGeom& g = fe->geom.lv[l];
        g.w = lws[l] = lw;
        g.h = lhs[l] = lh;
        g.pitch = (lw + 127) & ~127;
        g.off = (uint32_t)off;
        g.scale = fe->tab.scale[l];
        off += (size_t)g.pitch * lh;
        off = (off + 255) & ~(size_t)255;
        if (lw < 40 || lh < 40 || lw > 4095 + 32 || lh > 4095 + 32) {
            g_err = "image too small/large for this level count";
            return VSLAM_ERR_UNSUPPORTED;
        }
        /* DistributeOctTree needs nIni = round(W/H) >= 1 (fextractor.cpp:534) */
        if ((int)std::round((float)(lw - 32) / (float)(lh - 32)) < 1) {
            g_err = "portrait aspect ratio: the reference's DistributeOctTree has nIni == 0 (undefined)";
            return VSLAM_ERR_UNSUPPORTED;
        }
    }
    fe->slot_stride = off;
    fe->cap = vslam::keypoint_capacity(fe->tab.quota.data(), lws, lhs, p.nlevels, p.nfeatures);
    if (int rc = fe->d_pyr.alloc(fe->slot_stride * fe->B)) return rc;
    if (int rc = fe->d_blur.alloc(fe->slot_stride * fe->B)) return rc;
    HIPCHK(hipMemset(fe->d_pyr, 0, fe->slot_stride * fe->B));
    HIPCHK(hipMemset(fe->d_blur, 0, fe->slot_stride * fe->B));
    return VSLAM_OK;
}

/* resize tables of every level, and the fused pyramid plan: levels 1-3 from level 0, then groups of four (8 levels = 2
 * launches instead of 7).  Needs the quad table on every level; VSLAM_PYRAMID=levels keeps one launch per level (A/B runs). */
static int create_pyramid(vslam_fe* fe) {
    const vslam_fe_params& p = fe->p;
    std::vector<vslam::PyrLevelTables> pyr_tabs(p.nlevels);
    for (int l = 1; l < p.nlevels; l++) {
        vslam::ResizeTables& r = pyr_tabs[l].r;
        const LevelGeom &s = fe->geom.lv[l - 1], &d = fe->geom.lv[l];
        pyr_tabs[l].sw = s.w; pyr_tabs[l].sh = s.h; pyr_tabs[l].dw = d.w; pyr_tabs[l].dh = d.h;
        vslam::build_resize_tables(s.w, s.h, d.w, d.h, r);
        if (int rc = vslam_upload(fe->d_xtab[l], r.xtab.data(), r.xtab.size() * 2)) return rc;
        if (int rc = vslam_upload(fe->d_xa[l], r.xa.data(), r.xa.size() * 2)) return rc;
        if (int rc = vslam_upload(fe->d_ytab[l], r.ytab.data(), r.ytab.size() * 2)) return rc;
        if (int rc = vslam_upload(fe->d_yb[l], r.yb.data(), r.yb.size() * 2)) return rc;
        std::vector<uint16_t>& qbase = pyr_tabs[l].qbase;
        std::vector<uint32_t>& quads = pyr_tabs[l].quads;
        /* four outputs whose eight taps do not fit one 8-byte source window (scale factors >~ 1.6): that level uses
         * the generic one-pixel-per-thread kernel */
        if (vslam::build_resize_quads(r, s.w, d.w, qbase, quads)) {
            if (int rc = vslam_upload(fe->d_qbase[l], qbase.data(), qbase.size() * 2)) return rc;
            if (int rc = vslam_upload(fe->d_quads[l], quads.data(), quads.size() * 4)) return rc;
        } else {
            qbase.clear(); /* marks "no quad table" for the fused-pyramid planner */
            quads.clear();
        }
    }
    bool fused = fe->tune.pyramid_per_level != 1 && p.nlevels > 1;
    for (int l = 1; l < p.nlevels && fused; l++) fused = fe->d_quads[l] != nullptr;
    static_assert(sizeof(PyrTileDev) == sizeof(vslam::PyrTileLevel), "planner and kernel share the tile record");
    /* tile height: 16 rows for contexts of one or two images, where a frame's latency counts and more workgroups per image
     * finish sooner (batch-1 latency through the C ABI: 0.135 ms with 12-16 rows, 0.137 with 20-28, 0.142 with 36, 0.146 with
     * 48); for batches see vslam::pyramid_tile_shape */
    /* one plan set (a vector of groups) per tile shape; false: some group has no plan at that shape */
    auto plan_groups = [&](int tune_pingpong, std::vector<vslam_fe::PyrGroupCtx>& out, bool* is_pingpong) -> int {
        int pyr_rows;
        bool pyr_pingpong;
        size_t pyr_lds;
        vslam::pyramid_tile_shape(p.width, p.height, fe->B, fe->tune.pyr_rows, tune_pingpong, &pyr_rows, &pyr_pingpong, &pyr_lds);
        if (is_pingpong) *is_pingpong = pyr_pingpong;
        bool ok = true;
        for (int l0 = 0; ok && l0 + 1 < p.nlevels;) {
            const int nl = std::min(l0 == 0 ? 3 : VSLAM_PYR_GROUP_LEVELS, p.nlevels - 1 - l0);
            std::vector<const vslam::PyrLevelTables*> gt;
            for (int j = 1; j <= nl; j++) gt.push_back(&pyr_tabs[l0 + j]);
            vslam::PyrGroupPlan plan;
            if (!vslam::build_pyramid_group(gt, l0, pyr_lds, plan, pyr_rows, pyr_pingpong)) {
                ok = false;
                break;
            }
            vslam_fe::PyrGroupCtx g;
            memset(&g.dev, 0, sizeof(g.dev));
            g.dev.l0 = l0;
            g.dev.nl = nl;
            g.dev.ntiles = plan.ntx * plan.nty;
            g.dev.readable_w0 = p.width;
            g.lds_bytes = plan.lds_bytes;
            g.fit = pyr_pingpong;
            if (int rc = vslam_upload(g.d_tiles, plan.tiles.data(), plan.tiles.size() * sizeof(PyrTileDev))) return rc;
            g.dev.tiles = g.d_tiles;
            for (int j = 0; j <= nl; j++) g.dev.lg[j] = fe->geom.lv[l0 + j];
            for (int j = 1; j <= nl; j++) {
                g.dev.qbase[j - 1] = fe->d_qbase[l0 + j];
                g.dev.quads[j - 1] = fe->d_quads[l0 + j];
                g.dev.ytab[j - 1] = fe->d_ytab[l0 + j];
                g.dev.yb[j - 1] = fe->d_yb[l0 + j];
            }
            out.push_back(std::move(g));
            l0 += nl;
        }
        if (!ok) out.clear();
        return VSLAM_OK;
    };
    if (fused) {
        bool is_pingpong = false;
        const int rc = plan_groups(fe->tune.pyr_pingpong, fe->pyr_groups, &is_pingpong);
        if (rc != VSLAM_OK) return rc;
        /* The default ping-pong shape is the mono entries': beside the init matcher's coupled contexts it gains 3.7 % at KITTI
         * size.  Stereo frames lose 2.7 % with it (their step is the sum of the wide kernels' single-context times; FAST beside
         * a co-resident pyramid is longer), so the stereo-frame entry keeps the resident plan -- chosen per pass, like desc_kpw
         * (profiles/pyramid_beside_fast_ab.txt).  A shape set through vslam_tuning.pyr_pingpong holds for every entry. */
        if (is_pingpong && fe->tune.pyr_pingpong < 0 && !fe->pyr_groups.empty()) {
            const int rc2 = plan_groups(0, fe->pyr_groups_resident, nullptr);
            if (rc2 != VSLAM_OK) return rc2;
        }
    }
    return VSLAM_OK;
}

/* FAST cells, the bands of k_fast_bands and the candidate regions */
static int create_fast(vslam_fe* fe) {
    const vslam_fe_params& p = fe->p;
    for (int l = 0; l < p.nlevels; l++) {
        fe->level_cell_first[l] = (int)fe->cells.size();
        vslam::build_cells(l, fe->geom.lv[l].w, fe->geom.lv[l].h, fe->cells);
    }
    fe->level_cell_first[p.nlevels] = (int)fe->cells.size();
    if (fe->cells.empty()) { /* (w-32)/30 or (h-32)/30 is 0 on every level: the reference divides by it (fextractor.cpp:772-778) */
        g_err = "image too small: no 30-px FAST cell fits on any pyramid level";
        return VSLAM_ERR_UNSUPPORTED;
    }
    int maxw = 8, maxh = 8;
    size_t cand_total = 0;
    std::vector<CellDesc> dc(fe->cells.size());
    for (size_t i = 0; i < fe->cells.size(); i++) {
        const vslam::HostCell& c = fe->cells[i];
        dc[i].level = c.level; dc[i].x0 = c.x0; dc[i].y0 = c.y0; dc[i].x1 = c.x1; dc[i].y1 = c.y1; dc[i].pad = 0;
        dc[i].base = (uint32_t)cand_total;
        cand_total += (size_t)((c.x1 - c.x0 - 6 + 1) / 2) * (size_t)((c.y1 - c.y0 - 6 + 1) / 2);
        maxw = std::max(maxw, c.x1 - c.x0);
        maxh = std::max(maxh, c.y1 - c.y0);
    }
    fe->tile_pitch = (maxw + 3) & ~3;
    fe->tile_rows = maxh;
    fe->max_px = (maxw - 6) * (maxh - 6);
    if (fe->max_px > 8192) {
        g_err = "FAST cell larger than 8192 px";
        return VSLAM_ERR_UNSUPPORTED;
    }
    /* limits of k_fast_cells_v3 (LDS pitch 72, 2 keep words per interior row) and k_blur7_v2 (8-byte row windows); cell
     * windows are at most 59 + 6 px on a side and levels at least 40 px wide, so these never trigger */
    if (maxw > 66 || maxh > 134 || fe->geom.lv[p.nlevels - 1].w < 8) {
        g_err = "FAST cell window larger than 66 x 134 px";
        return VSLAM_ERR_UNSUPPORTED;
    }
    if (int rc = vslam_upload(fe->d_cells, dc.data(), dc.size() * sizeof(CellDesc))) return rc;
    /* bands of k_fast_bands: up to four cells of a cell row whose interiors are together at most 128 px wide */
    std::vector<vslam::HostBand> hb;
    vslam::build_bands(fe->cells, std::min(4, std::max(1, tune_or(fe->tune.fast_band_cells, 4))), 128, hb);
    vslam::BandTables bt;
    vslam::pack_bands(hb, p.nlevels, bt);
    static_assert(sizeof(BandDesc) == sizeof(vslam::BandWords), "packer and kernel share the band record");
    if (bt.ok && vk_fast_bands_check(bt.max_wh, bt.max_iw, bt.max_cells) == 0) {
        if (int rc = vslam_upload(fe->d_band_classes, bt.classes.data(), bt.classes.size())) return rc;
        if (int rc = vslam_upload(fe->d_bands, bt.bands.data(), bt.bands.size() * sizeof(BandDesc))) return rc;
        fe->nbands = (int)bt.bands.size();
        fe->band_max_wh = bt.max_wh;
        fe->band_max_iw = bt.max_iw;
    }
    /* every cell owns a fixed segment sized by the exact upper bound of its NMS survivors */
    fe->cand_cap = (int)std::max<size_t>(cand_total, 16);
    fe->cand_stride = (8 + fe->cells.size() * sizeof(CellOut) + (size_t)fe->cand_cap * 4 + 255) & ~(size_t)255;
    if (int rc = fe->d_cand.alloc(fe->cand_stride * fe->B)) return rc;
    return fe->h_cand.alloc(fe->cand_stride * fe->B);
}

/* descriptor pattern and disc, and the marching-rows blur's task list: one wave task per (level, row chunk, 248-column strip) */
static int create_blur(vslam_fe* fe) {
    if (int rc = vslam_upload(fe->d_pattern, VSLAM_ORB_PATTERN, 1024)) return rc;
    vk_upload_disc(fe->tab.umax);
    if (fe->tune.blur_rows >= 0) fe->blur_rows = std::min(512, std::max(8, (int)fe->tune.blur_rows));
    else if (fe->B <= 2) fe->blur_rows = 8; /* one or two images: more, shorter tasks finish sooner (batch-1 latency -5 us) */
    std::vector<uint32_t> tasks;
    for (int l = 0; l < fe->p.nlevels; l++) {
        const int br = fe->blur_rows;
        const int ns = std::max(1, (fe->geom.lv[l].w + 247) / 248), nc = (fe->geom.lv[l].h + br - 1) / br;
        for (int c = 0; c < nc; c++)
            for (int s = 0; s < ns; s++) tasks.push_back(((uint32_t)l << 24) | ((uint32_t)c << 12) | (uint32_t)s);
    }
    fe->n_blur_tasks = (int)tasks.size();
    if (int rc = vslam_upload(fe->d_blur_tasks, tasks.data(), tasks.size() * 4)) return rc;
    return VSLAM_OK;
}

/* the selected-keypoint lists, and ONE result block per context -- counts | keypoints | descriptors, back to back -- with
 * one pinned mirror of it: a full batch leaves the device in a single transfer (vslam_deliver_block) */
static int create_result_block(vslam_fe* fe) {
    const size_t nk = (size_t)fe->B * fe->cap;
    if (int rc = fe->d_sel.alloc(nk)) return rc;
    if (int rc = fe->h_sel.alloc(nk)) return rc;
    fe->res_counts_bytes = (((size_t)(fe->B * 4 + 4) * 4) + 255) & ~(size_t)255;
    fe->res_feat_bytes = fe->res_counts_bytes + nk * sizeof(vslam_kp) + nk * 32; /* multiple of 16: cap % 4 == 0 */
    /* ... followed by the outputs of the device SearchForInitialization for up to B pairs (vnMatches12 | vbPrevMatched |
     * nmatches), so that extraction and matcher results of a step can leave in ONE transfer (want_host = 2) */
    fe->res_init_bytes = (nk * 12 + (size_t)fe->B * 16 + 255) & ~(size_t)255; /* = init_scratch's need for B pairs */
    fe->res_bytes = fe->res_feat_bytes + fe->res_init_bytes;
    if (int rc = fe->d_res.alloc(fe->res_bytes)) return rc;
    if (int rc = fe->h_res.alloc(fe->res_bytes)) return rc;
    HIPCHK(hipMemset(fe->d_res, 0, fe->res_bytes));
    memset(fe->h_res, 0, fe->res_bytes);
    fe->d_counts = (int32_t*)fe->d_res;
    fe->h_counts = (int32_t*)fe->h_res;
    fe->d_kps = (vslam_kp*)(fe->d_res + fe->res_counts_bytes);
    fe->h_kps = (vslam_kp*)(fe->h_res + fe->res_counts_bytes);
    fe->d_desc = fe->d_res + fe->res_counts_bytes + nk * sizeof(vslam_kp);
    fe->h_desc = fe->h_res + fe->res_counts_bytes + nk * sizeof(vslam_kp);
    fe->d_init = fe->d_res + fe->res_feat_bytes; /* moves to d_init_own / h_init_own for more than B pairs (vslam_match.hip) */
    fe->h_init = fe->h_res + fe->res_feat_bytes;
    fe->init_bytes = fe->res_init_bytes;
    fe->init_in_block = true;
    return VSLAM_OK;
}

/* quadtree distribution on the device (k_octree_v4): the plan (vslam::plan_octree) into OctParams, key arrays,
 * result lists; decides the placement */
static int create_quadtree(vslam_fe* fe) {
    const vslam_fe_params& p = fe->p;
    int lws[VSLAM_MAX_LEVELS], lhs[VSLAM_MAX_LEVELS];
    for (int l = 0; l < p.nlevels; l++) {
        lws[l] = fe->geom.lv[l].w;
        lhs[l] = fe->geom.lv[l].h;
    }
    /* LDS a quadtree workgroup may take in all (default 128 KB of the CU's 160) */
    const size_t budget = (size_t)std::min(150, std::max(16, tune_or(fe->tune.oct_lds_budget_kb, 128))) * 1024;
    vslam::OctPlan plan;
    vslam::plan_octree(fe->tab.quota.data(), lws, lhs, fe->level_cell_first, p.nlevels, fe->tune.oct_fine_depth, budget,
                       vk_octree_lds_bytes, plan);
    OctParams& O = fe->oct;
    memset(&O, 0, sizeof(O));
    for (int l = 0; l < p.nlevels; l++) {
        O.N[l] = plan.N[l]; O.H[l] = plan.H[l]; O.nIni[l] = plan.nIni[l]; O.hX[l] = plan.hX[l];
        O.selOff[l] = plan.selOff[l]; O.fineD[l] = plan.fineD[l]; O.lutOff[l] = plan.lutOff[l]; O.lutW[l] = plan.lutW[l];
    }
    for (int l = 0; l <= p.nlevels; l++) O.cellFirst[l] = fe->level_cell_first[l];
    O.selStride = plan.selStride;
    O.maxNodes = plan.maxNodes;
    O.fineLdsOff = plan.fineLdsOff;
    O.fineLdsBytes = plan.fineLdsBytes;
    O.ptsCap = fe->cand_cap;
    if (fe->tune.oct_debug == 1) {
        if (int rc = fe->d_oct_dbg.alloc(64)) return rc;
        O.dbg = fe->d_oct_dbg;
        HIPCHK(hipMemset(O.dbg, 0, 64 * 8));
    }
    O.maxIter = tune_or(fe->tune.oct_max_iter, 64);
    const bool on_device = fe->dev_octree = plan.fits && !(p.flags & VSLAM_FLAG_HOST_OCTREE);
    /* threads per quadtree problem (vk_octree): 1024 for one or two images, else 256 at every frame size */
    fe->oct_threads = fe->tune.oct_threads == 256 || fe->tune.oct_threads == 512 || fe->tune.oct_threads == 1024
                          ? fe->tune.oct_threads
                          : fe->B <= 2 ? 1024 : 256;
    if (!on_device) return VSLAM_OK; /* none of the buffers below is needed */
    if (vk_octree_set_max_lds((size_t)O.fineLdsOff + (size_t)O.fineLdsBytes + 16) != 0) {
        g_err = "hipFuncSetAttribute(k_octree, max dynamic LDS) failed";
        return VSLAM_ERR_HIP;
    }
    const size_t np = (size_t)fe->B * fe->cand_cap;
    if (int rc = fe->d_pts.alloc(np)) return rc;
    if (int rc = fe->d_sel_xyr.alloc((size_t)fe->B * O.selStride)) return rc;
    if (int rc = fe->d_sel_cnt.alloc((size_t)fe->B * VSLAM_MAX_LEVELS)) return rc;
    if (int rc = fe->d_oct_sorted.alloc(np * 8)) return rc;
    if (int rc = fe->d_oct_redo.alloc((size_t)fe->B * VSLAM_MAX_LEVELS)) return rc;
    HIPCHK(hipMemset(fe->d_oct_redo, 0, (size_t)fe->B * VSLAM_MAX_LEVELS * 4));
    if (int rc = vslam_upload(fe->d_oct_lut, plan.lut.data(), plan.lut.size() * 4)) return rc;
    O.lut = fe->d_oct_lut;
    return VSLAM_OK;
}

static int create_stream_and_pool(vslam_fe* fe) {
    /* The runtime multiplexes HIP streams onto a fixed number of hardware queues (GPU_MAX_HW_QUEUES), one pool per
     * stream priority, least-used queue first.  In a process that already holds dozens of streams (torch, four RCCL
     * communicators) two contexts ended up on ONE hardware queue and their passes ran one behind the other (mono
     * 157 k -> 97 k frames/s, the kernel trace shows the shared queue id).  Streams of a priority of their own draw
     * from a pool nobody else uses: with stream_priority 2 (1 = low) the context's stream is created with a priority of
     * its own.  The library default is 0 -- the default pool -- because a high-priority stream also pre-empts the
     * host application's own default-priority work; a pipelined caller opts in (bench.py does).  Measured: collective path at world size 1 97 k -> 143 k (high) / 141 k (low),
     * the plain path unchanged at 157 k. */
    const int pr = tune_or(fe->tune.stream_priority, 0);
    int lo = 0, hi = 0;
    if (pr != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
        HIPCHK(hipStreamCreateWithPriority(&fe->stream, hipStreamNonBlocking, pr == 1 ? lo : hi));
    else
        HIPCHK(hipStreamCreateWithFlags(&fe->stream, hipStreamNonBlocking));
    if (int rc = fe->ev_cand.ensure(hipEventDisableTiming)) return rc;
    fe->use_graph = fe->tune.graphs != 0; /* 0: never replay captured graphs */
    fe->sel_level.resize((size_t)fe->B * fe->p.nlevels);
    fe->cand_level.resize((size_t)fe->B * fe->p.nlevels);
    unsigned hw = std::thread::hardware_concurrency();
    int nthreads = (int)std::min<unsigned>(hw ? hw : 4, 16) - 1;
    nthreads = std::min(nthreads, fe->B * fe->p.nlevels - 1);
    fe->pool = new WorkerPool(std::max(nthreads, 0));
    return VSLAM_OK;
}

static int create_impl(vslam_fe* fe) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || fe->p.device >= ndev) {
        g_err = "no usable HIP device (this library has no CPU fallback)";
        return VSLAM_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int (*const steps[])(vslam_fe*) = {create_geometry, create_pyramid, create_fast, create_blur, create_result_block,
                                       create_quadtree, create_stream_and_pool};
    for (auto step : steps) {
        const int rc = step(fe);
        if (rc != VSLAM_OK) return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    return VSLAM_OK;
}

extern "C" int vslam_fe_create(const vslam_fe_params* p, vslam_fe** out) {
    if (!p || !out) return VSLAM_ERR_INVALID;
    *out = nullptr;
    if (p->width <= 0 || p->height <= 0 || p->nfeatures <= 0 || p->nlevels < 1 ||
        p->nlevels > VSLAM_MAX_LEVELS || p->scale_factor <= 1.0f || p->max_batch < 1 ||
        p->max_batch > VSLAM_MAX_BATCH || p->min_th_fast < 1 || p->ini_th_fast < p->min_th_fast ||
        p->ini_th_fast > 254 || p->nfeatures > 60000) {
        g_err = "invalid parameters";
        return VSLAM_ERR_INVALID;
    }
    vslam_fe* fe = new vslam_fe();
    fe->p = *p;
    fe->tune = vslam_resolve_tuning(p->tuning);
    fe->p.tuning = nullptr; /* the caller's struct need not outlive the call */
    int rc = create_impl(fe);
    if (rc != VSLAM_OK) {
        std::string keep = g_err;
        free_ctx(fe);
        g_err = keep;
        return rc;
    }
    *out = fe;
    return VSLAM_OK;
}

extern "C" int vslam_fe_set_tuning(vslam_fe* fe, const vslam_tuning* t) {
    if (!fe || !t) return VSLAM_ERR_INVALID;
    vslam_apply_tuning(fe->tune, t);
    fe->use_graph = fe->use_graph && fe->tune.graphs != 0;
    /* a captured graph froze the launch shapes and transport routes it was captured with, and its key does not cover the
     * tuning fields: drop it, so that the next host-image pass captures again under the new switches (otherwise an A/B
     * run through this call would compare a configuration with itself) */
    if (fe->graph_exec) {
        if (fe->stream) hipStreamSynchronize(fe->stream);
        hipGraphExecDestroy(fe->graph_exec);
        fe->graph_exec = nullptr;
        fe->graph_key = 0;
    }
    return VSLAM_OK;
}

extern "C" int vslam_fe_tables(const vslam_fe* fe, float* scale, float* inv_scale, float* sigma2,
                               float* inv_sigma2, int32_t* quota) {
    if (!fe) return VSLAM_ERR_INVALID;
    for (int i = 0; i < fe->p.nlevels; i++) {
        if (scale) scale[i] = fe->tab.scale[i];
        if (inv_scale) inv_scale[i] = fe->tab.inv_scale[i];
        if (sigma2) sigma2[i] = fe->tab.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = fe->tab.inv_sigma2[i];
        if (quota) quota[i] = fe->tab.quota[i];
    }
    return fe->p.nlevels;
}

extern "C" int vslam_fe_octree_stats(const vslam_fe* fe, unsigned long long* problems, unsigned long long* split_below_grid,
                                     uint32_t* last_level_masks) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (problems) *problems = fe->oct_problems;
    if (split_below_grid) *split_below_grid = fe->oct_deep;
    if (last_level_masks)
        for (int s = 0; s < fe->B; s++) last_level_masks[s] = s < fe->last_nimg ? fe->oct_last_mask[s] : 0u;
    return VSLAM_OK;
}

extern "C" int vslam_fe_delivery_stats(const vslam_fe* fe, unsigned long long* transfers, unsigned long long* bytes) {
    if (!fe) return VSLAM_ERR_INVALID;
    if (transfers) *transfers = fe->n_deliveries;
    if (bytes) *bytes = fe->n_delivery_bytes;
    return VSLAM_OK;
}

extern "C" int vslam_dbg_octree_stamps(vslam_fe* fe, unsigned long long* out64) {
    if (!fe || !fe->oct.dbg) return VSLAM_ERR_INVALID;
    HIPCHK(hipMemcpy(out64, fe->oct.dbg, 64 * 8, hipMemcpyDeviceToHost));
    return VSLAM_OK;
}

extern "C" int vslam_dbg_live_memory(unsigned long long* device_bytes, unsigned long long* device_blocks,
                                     unsigned long long* pinned_bytes, unsigned long long* pinned_blocks) {
    if (device_bytes) *device_bytes = g_vslam_device_mem.bytes.load();
    if (device_blocks) *device_blocks = g_vslam_device_mem.blocks.load();
    if (pinned_bytes) *pinned_bytes = g_vslam_pinned_mem.bytes.load();
    if (pinned_blocks) *pinned_blocks = g_vslam_pinned_mem.blocks.load();
    return VSLAM_OK;
}

extern "C" void* vslam_fe_stream(vslam_fe* fe) { return fe ? (void*)fe->stream : nullptr; }

/* GPU-side ordering between two contexts: everything enqueued on `waiter` after this call runs after
 * everything enqueued on `signal` so far (hipEventRecord + hipStreamWaitEvent; no host synchronisation). */
extern "C" int vslam_fe_wait_for(vslam_fe* waiter, vslam_fe* signal) {
    if (!waiter || !signal || waiter->p.device != signal->p.device) return VSLAM_ERR_INVALID;
    if (waiter == signal) return VSLAM_OK;
    HIPCHK(hipSetDevice(waiter->p.device));
    if (int rc = signal->ev_x.ensure(hipEventDisableTiming)) return rc;
    HIPCHK(hipEventRecord(signal->ev_x, signal->stream));
    HIPCHK(hipStreamWaitEvent(waiter->stream, signal->ev_x, 0));
    return VSLAM_OK;
}

/* Finer-grained form: four user events per context.  _record marks a point of fe's stream, _wait makes
 * waiter's stream wait for the last recorded instance of signal's event idx (a never-recorded event does
 * not block). */
extern "C" int vslam_fe_event_record(vslam_fe* fe, int idx) {
    if (!fe || idx < 0 || idx >= 4) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(fe->p.device));
    if (int rc = fe->ev_user[idx].ensure(hipEventDisableTiming)) return rc;
    HIPCHK(hipEventRecord(fe->ev_user[idx], fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_fe_event_wait(vslam_fe* waiter, vslam_fe* signal, int idx) {
    if (!waiter || !signal || idx < 0 || idx >= 4 || waiter->p.device != signal->p.device) return VSLAM_ERR_INVALID;
    if (!signal->ev_user[idx] || waiter == signal) return VSLAM_OK;
    HIPCHK(hipSetDevice(waiter->p.device));
    HIPCHK(hipStreamWaitEvent(waiter->stream, signal->ev_user[idx], 0));
    return VSLAM_OK;
}

/* Pacing of the one kernel that takes a CU's whole LDS: with a gate set, the FAST launch of every pass of `fe` waits (GPU side)
 * for the FAST launch of `signal`'s latest pass to have finished, so that a pipelined caller who keeps several contexts in
 * flight never has two FAST launches resident at once (bench.py --fast-chain).  signal == NULL removes the gate.  Passes
 * with a gate are not captured into graphs (an event of another stream cannot be waited for inside a capture). */
extern "C" int vslam_fe_set_fast_gate(vslam_fe* fe, vslam_fe* signal) {
    if (!fe || (signal && (signal == fe || signal->p.device != fe->p.device))) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_gate_mu);
    gate_unlink(fe);
    if (signal) {
        fe->fast_gate = signal;
        signal->gate_waiters.push_back(fe);
        HIPCHK(hipSetDevice(signal->p.device));
        if (int rc = signal->ev_fast.ensure(hipEventDisableTiming)) return rc;
        signal->fast_gated_by_someone = true;
        fe->use_graph = false;
        signal->use_graph = false;
    }
    return VSLAM_OK;
}

extern "C" int vslam_fe_set_profiling(vslam_fe* fe, int on) {
    if (!fe) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(fe->p.device));
    for (int i = 0; i < 10 && on; i++)
        if (int rc = fe->ev_prof[i].ensure()) return rc;
    fe->profiling = on != 0;
    for (int i = 0; i < 5; i++) fe->prof_ms[i] = 0;
    fe->prof_batches = fe->prof_images = 0;
    fe->reset_span_timers();
    return VSLAM_OK;
}

extern "C" int vslam_fe_get_profile(vslam_fe* fe, double stage_ms[5], long* batches, long* images) {
    if (!fe || !stage_ms) return VSLAM_ERR_INVALID;
    for (int i = 0; i < 5; i++) stage_ms[i] = fe->prof_ms[i];
    if (batches) *batches = fe->prof_batches;
    if (images) *images = fe->prof_images;
    return VSLAM_OK;
}

static int pack_range(vslam_fe* fe, int first, int nslots, void* dev_dst, size_t slot_bytes, bool sync) {
    if (!fe || first < 0 || nslots < 0 || first + nslots > fe->B || !dev_dst ||
        slot_bytes < 16 + (size_t)fe->cap * 60 || (slot_bytes & 15) || ((uintptr_t)dev_dst & 15)) {
        g_err = "invalid arguments (slot_bytes and dev_dst must be 16-byte aligned)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    /* one kernel; the keypoint counts are read from HBM, so this may be enqueued before the host knows them */
    vk_pack_slots(fe->stream, fe->d_kps, fe->d_desc, fe->d_counts, fe->cap, first, nslots, (uint8_t*)dev_dst, slot_bytes);
    HIPCHK(hipGetLastError());
    if (sync) HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_fe_pack_slot_range(vslam_fe* fe, int first, int nslots, void* dev_dst, size_t slot_bytes) {
    return pack_range(fe, first, nslots, dev_dst, slot_bytes, true);
}

/* same, but only enqueued on the context's stream (ordered after the extraction that produced the slots) */
extern "C" int vslam_fe_pack_slot_range_async(vslam_fe* fe, int first, int nslots, void* dev_dst,
                                              size_t slot_bytes) {
    return pack_range(fe, first, nslots, dev_dst, slot_bytes, false);
}

extern "C" int vslam_fe_pack_slots(vslam_fe* fe, int nslots, void* dev_dst, size_t slot_bytes) {
    return vslam_fe_pack_slot_range(fe, 0, nslots, dev_dst, slot_bytes);
}

extern "C" int vslam_fe_level_size(const vslam_fe* fe, int level, int* w, int* h) {
    if (!fe || level < 0 || level >= fe->p.nlevels) return VSLAM_ERR_INVALID;
    if (w) *w = fe->geom.lv[level].w;
    if (h) *h = fe->geom.lv[level].h;
    return VSLAM_OK;
}

extern "C" int vslam_fe_level_copy(vslam_fe* fe, int slot, int level, int blurred, uint8_t* dst,
                                   size_t dst_pitch) {
    if (!fe || slot < 0 || slot >= fe->B || level < 0 || level >= fe->p.nlevels || !dst) return VSLAM_ERR_INVALID;
    const LevelGeom& g = fe->geom.lv[level];
    if (dst_pitch < (size_t)g.w) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(fe->p.device));
    const uint8_t* s;
    size_t spitch;
    if (!blurred && level == 0) {
        s = fe->src.l0[slot];
        spitch = fe->src.pitch0[slot];
        if (!s) return VSLAM_ERR_INVALID;
    } else {
        s = (blurred ? fe->d_blur : fe->d_pyr) + (size_t)slot * fe->slot_stride + g.off;
        spitch = g.pitch;
    }
    HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, s, spitch, g.w, g.h, hipMemcpyDeviceToHost, fe->stream));
    HIPCHK(vslam_stream_wait(fe->stream));
    return VSLAM_OK;
}

extern "C" int vslam_fe_slot_count_ptr(vslam_fe* fe, int slot, const int32_t** dev_n) {
    if (!fe || slot < 0 || slot >= fe->B || !dev_n) return VSLAM_ERR_INVALID;
    *dev_n = fe->d_counts + slot * 4;
    return VSLAM_OK;
}

extern "C" int vslam_fe_slot_buffers(vslam_fe* fe, int slot, const vslam_kp** dev_kps, const uint8_t** dev_desc,
                                     int* n) {
    if (!fe || slot < 0 || slot >= fe->B) return VSLAM_ERR_INVALID;
    if (dev_kps) *dev_kps = fe->d_kps + (size_t)slot * fe->cap;
    if (dev_desc) *dev_desc = fe->d_desc + (size_t)slot * fe->cap * 32;
    if (n) *n = fe->n_out[slot];
    return VSLAM_OK;
}

extern "C" int vslam_fe_capacity(const vslam_fe* fe) { return fe ? fe->cap : VSLAM_ERR_INVALID; }

extern "C" int vslam_fe_slot_host_views(vslam_fe* fe, int slot, const vslam_kp** host_kps,
                                        const uint8_t** host_desc) {
    if (!fe || slot < 0 || slot >= fe->B) return VSLAM_ERR_INVALID;
    if (host_kps) *host_kps = fe->h_kps + (size_t)slot * fe->cap;
    if (host_desc) *host_desc = fe->h_desc + (size_t)slot * fe->cap * 32;
    return VSLAM_OK;
}
