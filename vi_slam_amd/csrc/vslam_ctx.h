/* vslam_ctx.h -- private: the vslam_fe context (HBM layout, scratch, worker pool) shared by
 * vslam_context.hip (its life and accessors), vslam_upload.hip (host images into level 0), vslam_fe.hip (the extraction
 * pipeline) and by the matcher ABI: vslam_stereo.hip (stereo, RGB-D), vslam_match.hip (SearchForInitialization),
 * vslam_projection.hip (SearchByProjection family, Fuse), vslam_local_points.hip (isInFrustum, SearchLocalPoints),
 * vslam_projection_rig.hip (the rig forms), vslam_two_view.hip (CheckHomography / CheckFundamental), vslam_bow.hip,
 * vslam_bow_rig.hip and vslam_kfdb.hip. */
#ifndef VSLAM_CTX_H
#define VSLAM_CTX_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vslam_orb_pattern.h"
#include "vslam_host.h"
#include "vslam_pool.h"
#include "vslam_kernels.h"
#include "vslam_tuning.h"
#include "vslam_mem.h" /* g_err, HIPCHK, the owning buffers and events */
#include "vslam_staging.h"
#include "vslam_async.h" /* vslam_pending, vslam_span_timer */

/* ------------------------------------------------------------------ context */
enum { VSLAM_REGION_NONE = 0, VSLAM_REGION_INIT = 1, VSLAM_REGION_STEREO = 2 };
enum { LP_SINGLE = 0, LP_RIG = 1 }; /* vslam_fe::lp_op.kind */
/* Every vslam_dbuf / vslam_hbuf / vslam_event member is owned and goes with the context (vslam_mem.h); a raw d_* / h_*
 * pointer is a view into one of them and is commented as such. */
struct vslam_fe {
    vslam_fe_params p;
    vslam_tuning tune; /* the context's behaviour switches, resolved once by vslam_fe_create (vslam_tuning.h) */
    vslam::ExtractorTables tab;
    PyramidGeom geom;
    size_t slot_stride = 0; /* bytes per slot in d_pyr / d_blur */
    int B = 1, cap = 0;

    hipStream_t stream = nullptr;
    vslam_event ev_cand;
    vslam_event ev_x; /* cross-context ordering (vslam_fe_wait_for) */
    vslam_event ev_user[4];      /* vslam_fe_event_record / _wait */
    int desc_kpw_hint = -1;           /* keypoints per wave of the descriptor kernel for the pass being enqueued (-1: by batch size) */
    vslam_event ev_fast;              /* recorded behind the FAST launch of every pass once a gate refers to this context */
    vslam_fe* fast_gate = nullptr;    /* vslam_fe_set_fast_gate: this context's FAST waits for that context's last FAST */
    bool fast_gated_by_someone = false;
    std::vector<vslam_fe*> gate_waiters; /* contexts whose fast_gate is this one: un-gated when this context is destroyed */

    vslam_dbuf<uint8_t> d_pyr;
    vslam_dbuf<uint8_t> d_blur;
    /* resize tables, one set per destination level >= 1 */
    vslam_dbuf<uint16_t> d_xtab[VSLAM_MAX_LEVELS];
    vslam_dbuf<int16_t> d_xa[VSLAM_MAX_LEVELS];
    vslam_dbuf<uint16_t> d_ytab[VSLAM_MAX_LEVELS];
    vslam_dbuf<int16_t> d_yb[VSLAM_MAX_LEVELS];
    vslam_dbuf<uint16_t> d_qbase[VSLAM_MAX_LEVELS];    /* k_resize_level_v2 quad tables (nullptr: generic k_resize_level) */
    vslam_dbuf<ResizeQuad> d_quads[VSLAM_MAX_LEVELS];
    /* fused pyramid: groups of levels per launch (k_pyramid_group); empty -> one launch per level */
    struct PyrGroupCtx { /* move-only: owns its tile table */
        PyrGroupDev dev;
        size_t lds_bytes;
        bool fit; /* ping-pong plan: k_pyramid_group<.., true> */
        vslam_dbuf<PyrTileDev> d_tiles;
    };
    std::vector<PyrGroupCtx> pyr_groups;
    /* the resident plan beside a default ping-pong one, for the passes of the stereo-frame entry (empty: pyr_groups serves every
     * entry -- a shape set through vslam_tuning, contexts of one or two images, frames above a megapixel) */
    std::vector<PyrGroupCtx> pyr_groups_resident;
    bool pyr_resident_hint = false;   /* the pass being enqueued takes pyr_groups_resident (set by the stereo-frame entry) */
    /* FAST cells */
    std::vector<vslam::HostCell> cells;
    int level_cell_first[VSLAM_MAX_LEVELS + 1] = {};
    vslam_dbuf<CellDesc> d_cells;
    int tile_pitch = 0, tile_rows = 0, max_px = 0;
    /* FAST bands (k_fast_bands): up to four cells of a cell row per workgroup; nbands == 0: not available for this geometry */
    vslam_dbuf<BandDesc> d_bands;
    vslam_dbuf<uint8_t> d_band_classes; /* 272-byte column tables, BandDesc::lnw >> 16 indexes them */
    int nbands = 0, band_max_wh = 0, band_max_iw = 0;
    /* candidates: per slot [total, overflow, CellOut[ncells], cand[cand_cap]] */
    vslam_dbuf<uint8_t> d_cand;
    vslam_hbuf<uint8_t> h_cand;
    size_t cand_stride = 0;
    int cand_cap = 0;
    int32_t taps[7];
    vslam_dbuf<uint32_t> d_blur_tasks;
    int n_blur_tasks = 0;
    int oct_threads = 1024; /* threads per quadtree problem (k_octree_v4), chosen at creation */
    int blur_rows = 32; /* output rows per wave task of k_blur7_v2 (VSLAM_BLUR_ROWS) */
    /* selection + outputs */
    vslam_dbuf<SelKp> d_sel;
    vslam_hbuf<SelKp> h_sel; /* B*cap */
    vslam_dbuf<uint8_t> d_res; /* the context's result block: counts (res_counts_bytes) | kps B*cap | desc B*cap*32 */
    vslam_hbuf<uint8_t> h_res; /* pinned mirror, same layout */
    size_t res_bytes = 0, res_counts_bytes = 0, res_feat_bytes = 0, res_init_bytes = 0;
    bool init_in_block = false;    /* d_init / h_init are the block's own matcher region (not d_init_own / h_init_own) */
    /* result deliveries of the extraction / SearchForInitialization paths so far (vslam_fe_delivery_stats) */
    unsigned long long n_deliveries = 0, n_delivery_bytes = 0, graph_deliveries = 0, graph_delivery_bytes = 0;
    bool deliver_deferred = false; /* an extraction with want_host = 2 is waiting for the matcher call that delivers both */
    vslam_kp* d_kps = nullptr; /* views into d_res / h_res */
    uint8_t* d_desc = nullptr;
    vslam_kp* h_kps = nullptr;
    uint8_t* h_desc = nullptr;
    vslam_dbuf<int8_t> d_pattern;
    BatchSrc src;
    int n_out[VSLAM_MAX_BATCH] = {};
    int mono_out[VSLAM_MAX_BATCH] = {};
    /* quadtree statistics (vslam_fe_octree_stats): (slot, level) problems distributed on the device so far, on how many
     * of them k_octree_v4 split nodes below its fine grid, and the per-slot level masks of the last pass */
    unsigned long long oct_problems = 0, oct_deep = 0;
    uint32_t oct_last_mask[VSLAM_MAX_BATCH] = {};
    int32_t pack_hdr[VSLAM_MAX_BATCH][4] = {}; /* headers of vslam_fe_pack_slots while the copy is in flight */
    std::vector<std::vector<vslam::Cand>> sel_level; /* [slot*nlevels + level] */
    std::vector<std::vector<vslam::Cand>> cand_level;
    /* matcher scratch (grown on demand) */
    vslam_hbuf<uint8_t> h_top2; /* idx2 | dist2 of the batched brute-force matcher */
    vslam_dbuf<uint32_t> d_part;
    vslam_dbuf<int32_t> d_idx2; /* rows x 2, as d_dist2 */
    vslam_dbuf<int32_t> d_dist2;
    vslam_dbuf<uint8_t> d_dmat;
    vslam_dbuf<uint8_t> d_tmp_desc[2];
    /* device SearchForInitialization: matches12 | prevMatched | nmatches of every pair.  d_init / h_init are views: of the
     * result block's matcher region (init_in_block), or of the pair below once there are more pairs than image slots or
     * the stereo matcher's outputs live in the region (init_scratch in vslam_match.hip decides) */
    uint8_t* d_init = nullptr;
    uint8_t* h_init = nullptr;
    size_t init_bytes = 0; /* bytes behind either view */
    vslam_dbuf<uint8_t> d_init_own;
    vslam_hbuf<uint8_t> h_init_own;
    int init_pairs = 0;
    bool init_lds_set = false;
    /* vslam_fe_set_camera: Frame::UndistortKeyPoints behind every pass when has_cam && ud.dist[0] != 0 */
    bool has_cam = false;
    UdCam ud;
    vslam_dbuf<vslam_kp> d_ukps; /* B x cap, allocated by the first camera with k1 != 0 */
    /* vslam_fe_set_grid_bounds: Frame::mnMinX.. for the SearchByProjection / Fuse / SearchBySim3 matchers */
    bool has_grid_bounds = false;
    SiBounds grid_bounds = {0.0f, 0.0f, 0.0f, 0.0f};
    vslam_dbuf<uint8_t> d_init_scratch; /* k_si_topm -> k_si_replay: compacted octave-0 lists + sorted prefixes */
    vslam_dbuf<int> d_init_fb; /* 4 words, by vslam_init_fb_ensure: number of full re-scans in k_si_replay / k_sbp_replay (diagnostics) */
    /* one staging block for the single-call matchers (SearchByProjection, Fuse, ComputeDistinctiveDescriptors, SearchByBoW,
     * SearchForTriangulation): inputs | scratch | results, carved anew by every call */
    vslam_staging proj;
    bool proj_lds_set = false, dist_lds_set = false;
    vslam_staging bow;          /* ComputeBoW: per-feature weight | word | node for nslots x cap features */
    int bow_jobs = 0;
    vslam_staging kfdb;         /* KeyFrameDatabase query: uploaded BowVectors | dense per-slot results (vslam_kfdb.hip) */
    vslam_staging lp;           /* SearchLocalPoints: inputs | frustum records | compacted arrays | matcher scratch | results (vslam_local_points.hip) */
    vslam_pending lp_op;        /* kind LP_SINGLE or LP_RIG (vslam_search_local_points_rig_async); n: the keypoints, of a rig both sides' */
    int lp_n_mp = 0, lp_cap = 0;
    size_t lp_o_track = 0, lp_o_res = 0, lp_o_cnt = 0, lp_o_idx = 0; /* where the records and the result block (matches | counts | indices) start */
    size_t lp_o_track_r = 0;    /* a rig search: the right camera's records */
    bool use_graph = true;          /* host-image passes replay a captured HIP graph (VSLAM_GRAPH=0 disables) */
    hipGraphExec_t graph_exec = nullptr;
    long long graph_key = 0;
    size_t graph_pitch = 0;                          /* pinned-image passes: the captured pull reads these */
    const uint8_t* graph_imgs[VSLAM_MAX_BATCH] = {};
    int graph_lap0 = 0, graph_lap1 = 0;
    vslam_hbuf<uint8_t> h_img;  /* staging for host images: B x height x level-0 pitch (sized for the pixel format in force) */
    size_t h_img_pitch = 0;     /* row pitch of the images staged last: the level-0 pitch, or the width for dense sources */
    vslam_dbuf<uint8_t> d_stage; /* device staging of pinned caller images copied by the DMA engines (VSLAM_H2D=sdma) */
    vslam_staging sbp;          /* batched device-resident SearchByProjection: scratch of every job | results of all jobs */
    int sbp_jobs = 0, sbp_M = 8;
    size_t sbp_o_res = 0;       /* where the results (match tables | counts) start */
    vslam_dbuf<float> d_x3dw;    /* stereo points per pair: B x cap x 3 */
    vslam_dbuf<uint8_t> d_mpflags; /* B x cap */
    /* stereo scratch */
    vslam_dbuf<void> d_stereo;
    vslam_hbuf<float> h_stereo; /* [uRight | depth] x pairs x cap */
    float *d_stereo_u = nullptr, *d_stereo_depth = nullptr; /* views: mvuRight / mvDepth of the last stereo pass on the device */
    float* h_stereo_cur = nullptr; /* view: where the last stereo pass delivered: h_stereo, or the result block's matcher region */
    int block_region_owner = 0;    /* VSLAM_REGION_*: which matcher's outputs live in the result block's extra region */
    int stereo_pairs = 0;
    int stereo_capR = 0; /* slot capacity of the right context of the last stereo enqueue (scratch carving) */
    int stereo_slotL[VSLAM_MAX_BATCH] = {}; /* an RGB-D pass has one "pair" per image slot */
    /* vslam_fe_set_pixel_format: interleaved colour input, converted to gray into level 0 by k_gray_images */
    int pix_fmt = VSLAM_PIX_GRAY8, gray_shift = 15;
    vslam_hbuf<uint8_t> h_depth; /* staging of pageable depth images (vslam_frame_rgbd_batch_async, VSLAM_IMGS_HOST) */
    bool last_rgbd = false;     /* the last pass enqueued was an RGB-D pass: vslam_frame_rgbd_wait may deliver it */
    vslam_span_timer<1> t_rgbd; /* around k_rgbd_depth */
    /* two-view scoring (vslam_two_view.hip): job table | hypotheses | host inputs | results of every job; the gathered pairs
     * and the flag bytes of every hypothesis stay in HBM */
    vslam_staging tv;
    vslam_dbuf<uint8_t> d_tv_scratch;
    vslam_pending tv_op;            /* jobs: the jobs of the scoring in flight */
    struct TvJobHost {              /* where a job's results start in the block, and the counts _wait copies by */
        size_t o_hdr, o_pairs, o_sh, o_sf, o_ih, o_if;
        int cap, nH, nF;
    } tv_jobs[VSLAM_TWO_VIEW_MAX_JOBS] = {};
    vslam_span_timer<3> t_tv;   /* before k_tv_pairs | k_tv_score | k_tv_select | behind it */
    vslam_span_timer<2> t_lp;   /* before k_frustum | between | behind k_frustum_compact */
    vslam_span_timer<2> t_rig;  /* a rig search: before k_sbp_rank | between | behind k_rig_resolve */
    /* SearchByProjection(CurrentFrame, LastFrame) of a rig (vslam_search_by_projection_frame_rig_async): a block of its own, so
     * that the blocking matchers, which fill `proj` on the host at once, can run while a search is in flight */
    vslam_staging fr;           /* inputs | scratch of both sides | match table | nmatches, needSeq */
    vslam_pending fr_op;        /* n: n_left + n_right */
    size_t fr_o_m = 0, fr_o_n = 0;
    vslam_span_timer<2> t_fr;   /* before k_sbp_rank_rig | between | behind k_sbp_rig_replay */
    /* SearchByBoW(KeyFrame, Frame) of a rig against up to 16 keyframes (vslam_search_by_bow_rig_async, vslam_bow_rig.hip): a
     * block of its own for the same reason */
    vslam_staging sbr;          /* frame FeatureVector | per job: flags, angles, FeatureVector | match tables | bins | nmatches, overflow */
    vslam_pending sbr_op;       /* jobs: keyframe jobs, n: n_left + n_right of the frame */
    size_t sbr_o_m = 0, sbr_o_n = 0;
    vslam_span_timer<2> t_sbr;  /* before k_sbow_nodes_rig | between | behind k_sbow_finish_rig */
    /* the search half of Fuse for a fisheye KeyFrame / a rig, up to 16 (KeyFrame, camera) jobs (vslam_fuse_search_rig_async,
     * vslam_fuse_rig.hip): a block of its own for the same reason */
    vslam_staging fsr;          /* points | descriptors (host points only) | per job: validity bytes | best_idx | best_dist of every job */
    vslam_pending fsr_op;       /* jobs: the jobs, n: the MapPoints */
    size_t fsr_o_bi = 0, fsr_o_bd = 0;
    vslam_span_timer<1> t_fsr;  /* around k_fuse_rank_rig */
    /* SearchByProjection(pKF, Scw, ..) for fisheye KeyFrames, up to 16 (KeyFrame, Scw) jobs over one MapPoint list
     * (vslam_search_by_projection_sim3_kb8_async, vslam_sim3_kb8.hip): a block of its own for the same reason */
    vslam_staging s3k;          /* points | descriptors (host points only) | per job: validity bytes | per job: vpMatched bytes | per job: match_kf | nmatches, n_gated */
    vslam_dbuf<uint8_t> d_s3k;  /* HBM only: gate records | chunk counts | counts | needSeq | per job: matcher scratch, compacted arrays */
    vslam_pending s3k_op;       /* jobs: the jobs, n: the MapPoints */
    int s3k_nkf[16] = {};       /* keypoints per job: what _wait sizes match_kf by */
    size_t s3k_o_m[16] = {}, s3k_o_res = 0;
    vslam_span_timer<3> t_s3k;  /* before k_s3k_gate | behind k_s3k_compact | behind k_sbp_rank_kb8 | behind k_s3k_finish */

    /* GPU quadtree distribution */
    bool dev_octree = false;
    OctParams oct;
    vslam_dbuf<unsigned long long> d_oct_dbg;  /* vslam_tuning.oct_debug: the 64 stamps oct.dbg points at */
    vslam_dbuf<uint32_t> d_pts;               /* k_octree_v4: every level's keys in key order, B x cand_cap */
    vslam_dbuf<uint8_t> d_oct_sorted;         /* k_octree_v4: {key, position} sorted by fine cell, B x cand_cap x 8 bytes (written only by problems that split below the grid) */
    vslam_dbuf<uint32_t> d_oct_lut;           /* k_octree_v4: per level the x and y path tables (vslam::build_oct_lut) */
    vslam_dbuf<int32_t> d_oct_redo;           /* k_octree_v4: (slot, level) split nodes finer than the grid, B x VSLAM_MAX_LEVELS */
    vslam_dbuf<uint32_t> d_sel_xyr;           /* per slot / level result lists */
    vslam_dbuf<int32_t> d_sel_cnt;
    int32_t* d_counts = nullptr;              /* view into d_res: [slot][4] = n, monoIndex, -, - ; then [B*4] = error flags */
    int32_t* h_counts = nullptr;              /* view into h_res */
    bool cand_on_host = false;                /* h_cand holds the last batch's candidates */
    int last_nimg = 0;

    /* optional HIP-event timing of the kernel stages (bench.py roofline): resize x7, fast, blur, describe,
     * quadtree (+ output order) */
    bool profiling = false;
    vslam_event ev_prof[10];
    double prof_ms[5] = {0, 0, 0, 0, 0};
    long prof_batches = 0, prof_images = 0;
    /* every span timer of the enqueue / wait operations above, once: vslam_fe_set_profiling starts their sums anew */
    void reset_span_timers() {
        t_rgbd.reset();
        t_tv.reset();
        t_lp.reset();
        t_rig.reset();
        t_fr.reset();
        t_sbr.reset();
        t_fsr.reset();
        t_s3k.reset();
    }

    WorkerPool* pool = nullptr;

    /* vslam_fe_set_kb8_camera: the frustum stage projects with KannalaBrandt8::project, the entry points that project with
     * intrinsics of their own refuse (vslam_kb8.hip).  Behind everything an extraction pass reads. */
    bool has_kb8 = false;
    vslam_kb8_camera kb8 = {};
};


/* bytes per pixel of the context's input format, and bytes of one input row */
static inline int vslam_pix_bpp(int fmt) { return fmt == VSLAM_PIX_GRAY8 ? 1 : fmt <= VSLAM_PIX_BGR8 ? 3 : 4; }
static inline size_t vslam_row_bytes(const vslam_fe* fe) { return (size_t)fe->p.width * vslam_pix_bpp(fe->pix_fmt); }

/* vslam_upload.hip, for the extraction pipeline: pageable rows into the pinned staging, the widest pitch that leaves
 * there, the DMA route's device buffer (grown outside any capture), and the upload itself on fe's stream */
int vslam_stage_host_images(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch);
size_t vslam_host_stage_pitch(const vslam_fe* fe);
int vslam_stage_ensure(vslam_fe* fe, size_t spitch, int nimg);
int vslam_upload_host_rows(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int where);
int vslam_enqueue_extract(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int on_device,
                          int lap0, int lap1, int want_host);
int vslam_finish_extract(vslam_fe* fe, int nimg);
/* k_undistort_kps behind the descriptors of a pass, if the context has a camera with k1 != 0 (vslam_undistort.hip) */
int vslam_enqueue_undistort(vslam_fe* fe, int nimg);
int vslam_deliver(vslam_fe* fe, int nimg, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                  int* mono_index);


/* Host wait for a stream.  hipStreamSynchronize blocks on an interrupt after a short spin; VSLAM_WAIT=spin polls
 * hipStreamQuery instead (a core per waiting thread, lower wake-up latency). */
static inline hipError_t vslam_stream_wait(hipStream_t st) {
    const bool spin = vslam_process_tuning().wait_spin == 1; /* process-wide switch, resolved once (vslam_tuning.h) */
    if (!spin) return hipStreamSynchronize(st);
    hipError_t r;
    while ((r = hipStreamQuery(st)) == hipErrorNotReady) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return r;
}

/* bookkeeping of the result deliveries (vslam_fe_delivery_stats): `ops` copy operations carrying the ranges of R */
static inline void vslam_count_delivery(vslam_fe* fe, int ops, const CopyRanges& R) {
    fe->n_deliveries += (unsigned long long)ops;
    for (int r = 0; r < R.n; r++) fe->n_delivery_bytes += R.bytes[r];
}
static inline void vslam_count_delivery(vslam_fe* fe, int ops, size_t bytes) { /* a single range (vslam_copy_range) */
    fe->n_deliveries += (unsigned long long)ops;
    fe->n_delivery_bytes += bytes;
}

/* The result block -- counts | keypoints | descriptors -- and the `extra` bytes a matcher put behind them, from HBM to
 * the pinned mirror in ONE transfer on the context's stream. */
static inline int vslam_deliver_block(vslam_fe* fe, size_t extra) {
    const size_t bytes = fe->res_feat_bytes + extra;
    vslam_count_delivery(fe, vslam_copy_range(fe->stream, fe->h_res, fe->d_res, bytes, fe->tune), bytes);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

/* the diagnostics words of k_si_replay / k_sbp_replay (d_init_fb), zeroed when they are first allocated */
static inline int vslam_init_fb_ensure(vslam_fe* fe) {
    if (fe->d_init_fb) return VSLAM_OK;
    if (int rc = fe->d_init_fb.alloc(4)) return rc;
    HIPCHK(hipMemset(fe->d_init_fb, 0, 16));
    return VSLAM_OK;
}

/* the grid bounds of the _ex entry points: finite, non-empty (the reference divides by mnMaxX - mnMinX) */
static inline bool bounds_ok(const vslam_bounds* b) {
    return b && std::isfinite(b->min_x) && std::isfinite(b->max_x) && std::isfinite(b->min_y) && std::isfinite(b->max_y) &&
           b->max_x > b->min_x && b->max_y > b->min_y;
}
/* The img_w / img_h entry points pass {0, (float)img_w, 0, (float)img_h}: with mnMinX = mnMinY = 0 every expression of
 * the float-bounds matcher -- x - 0.0f, (float)W - 0.0f, the window and PosInGrid -- equals the integer-bounds one bit for
 * bit, so their results do not change. */
static inline SiBounds int_bounds(int img_w, int img_h) { return SiBounds{0.0f, (float)img_w, 0.0f, (float)img_h}; }
/* SearchByProjection / Fuse / SearchBySim3: the context's grid bounds (vslam_fe_set_grid_bounds) while they are set, else
 * the call's own img_w / img_h.  SearchForInitialization does not come here: its bounds are an argument. */
static inline SiBounds matcher_bounds(const vslam_fe* fe, int img_w, int img_h) {
    return fe->has_grid_bounds ? fe->grid_bounds : int_bounds(img_w, img_h);
}

#endif
