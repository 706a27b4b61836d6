/* include/vslam_fe.h -- C ABI of the MI355X-native visual front-end (libvslam_fe.so).
 *
 * Drop-in boundary for ONE hot path of KMS-TEAM/vi_slam: ORB extraction + 256-bit Hamming matching.
 * Every entry point names the reference interface it replaces (paths relative to the reference root).
 * Plain pointers and sizes only; all functions return VSLAM_OK (0) or a negative error code and never
 * abort (the reference asserts / exit()s, see fextractor.cpp:1041, cuda_common.h:49-82).
 *
 * The library is HIP-only: there is no CPU fallback.  If no gfx950 device is usable, vslam_fe_create()
 * fails with VSLAM_ERR_NO_DEVICE.
 *
 * Threading: a vslam_fe context is stateful (it owns the image pyramids, like FExtractor owns
 * mvImagePyramid, fextractor.h:64) and is NOT re-entrant; use one context per concurrent stream, exactly
 * as the reference allocates Left/Right/Ini extractors (tracking.cpp:1087-1093).  Different contexts may
 * be driven from different host threads (frame.cpp:107-108).
 */
#ifndef VSLAM_FE_H
#define VSLAM_FE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_OK 0
#define VSLAM_ERR_INVALID (-1)     /* bad argument / empty image (FExtractor::compute returns -1, :1037) */
#define VSLAM_ERR_NO_DEVICE (-2)   /* no usable HIP device */
#define VSLAM_ERR_HIP (-3)         /* a HIP runtime call failed; see vslam_last_error() */
#define VSLAM_ERR_CAPACITY (-4)    /* caller buffer or an internal candidate buffer too small */
#define VSLAM_ERR_UNSUPPORTED (-5) /* geometry the reference itself cannot process (e.g. nIni == 0) */
#define VSLAM_ERR_COMM (-6)        /* RCCL missing or a collective failed; see vslam_last_error() */

#define VSLAM_MAX_LEVELS 16
#define VSLAM_MAX_BATCH 64

/* values of the imgs_on_device argument (where the input images live) */
#define VSLAM_IMGS_HOST 0
#define VSLAM_IMGS_DEVICE 1
#define VSLAM_IMGS_PINNED 2
#define VSLAM_IMGS_STAGED 3 /* already in the slots' level 0: put there by vslam_fe_stage_images_async (imgs is ignored) */

/* flags for vslam_fe_params.flags: OpenCV build-dependent arithmetic the reference inherits */
#define VSLAM_FLAG_ATAN_FMA 1u /* cv::fastAtan2 Horner polynomial FMA-contracted (AVX2/FMA3 dispatch, aarch64) */
/* Run FExtractor::DistributeOctTree on the host worker pool instead of the GPU kernel (k_octree).  Only the selection
 * stage of a pass differs: the candidates are fetched to the host, distributed while the blur runs, and the selected
 * keypoints and counts uploaded in the layout the kernel leaves; description, undistortion and every form of delivery
 * (one transfer for a full batch, want_host = 2 included) are the device placement's.  Such a pass waits on the host
 * inside the enqueue call and is never replayed from a captured graph.  The library picks this placement by itself only
 * when a level's node list cannot fit LDS (nfeatures above about 12500 at scale factor 1.2 and 8 levels). */
#define VSLAM_FLAG_HOST_OCTREE 2u

/* Same 28-byte layout and field order as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave,
 * class_id) so std::vector<cv::KeyPoint> storage can be handed over directly. */
typedef struct vslam_kp {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} vslam_kp;

/* Behaviour switches of a context.  Every field: -1 = library default (vslam_tuning_init sets all of them to -1).
 * vslam_fe_create resolves them ONCE: a field the caller set wins, then the process default, which is read from the
 * environment variable named in the comment a single time per process (under std::call_once; documented for A/B runs of
 * whole programs), then the built-in default.  Nothing reads the environment after that, and no switch is cached in
 * unsynchronised statics, so two threads creating and using two contexts (frame.cpp:107-108) share no mutable state. */
typedef struct vslam_tuning {
    int32_t pyramid_per_level;    /* VSLAM_PYRAMID=levels: 1 = one launch per pyramid level instead of the fused groups */
    int32_t pyr_rows;             /* VSLAM_PYR_ROWS: rows of the first computed level per fused-pyramid tile (4..64; default 16 for contexts of
                                     one or two images, else 32 with pyr_pingpong, 48 / 40 above a megapixel without)  */
    int32_t pyr_threads;          /* retired: accepted and ignored (the fused pyramid runs 256 threads per tile) */
    int32_t blur_rows;            /* VSLAM_BLUR_ROWS: output rows per wave task of the blur (8..512, default 32) */
    int32_t fast_threads;         /* retired: accepted and ignored (128 threads per FAST cell) */
    int32_t fast_pitch;           /* retired: accepted and ignored */
    int32_t fast_lds_pad;         /* retired: accepted and ignored */
    int32_t octree_walk_kernel;   /* retired: accepted and ignored */
    int32_t oct_fine_depth;       /* VSLAM_OCT_FINE_D: depth of the one-walk kernel's fine grid (tests force 1 or 3) */
    int32_t oct_lds_budget_kb;    /* VSLAM_OCT_LDS_BUDGET_KB: LDS a quadtree workgroup may take (16..150, default 128) */
    int32_t oct_regkeys;          /* VSLAM_OCT_REGKEYS: deprecated alias, 1 = oct_threads 1024 */
    int32_t oct_max_iter;         /* VSLAM_OCT_MAXITER: split-pass limit (default 64) */
    int32_t oct_debug;            /* VSLAM_OCT_DBG: 1 = allocate the stamp buffer of diagnostic builds */
    int32_t graphs;               /* VSLAM_GRAPH: 0 = never capture / replay HIP graphs */
    int32_t h2d_route;            /* VSLAM_H2D=pull|sdma: 1 = kernel reads pinned memory, 2 = DMA engines (default by batch size) */
    int32_t d2h_route;            /* VSLAM_D2H=kernel|sdma: 1 = copy kernel, 2 = hipMemcpyAsync for every result transfer */
    int32_t copy_wgs;             /* VSLAM_COPY_WGS: workgroup cap of the copy kernel (default 16) */
    int32_t pull_depth;           /* VSLAM_PULL_DEPTH: loads in flight per lane of the pull kernel */
    int32_t init_topm;            /* VSLAM_INIT_TOPM: sorted candidate prefix per query of SearchForInitialization (1..16, default 8) */
    int32_t init_match_host;      /* VSLAM_INIT_MATCH=host: 1 = order-dependent replay on the host (cross-check path) */
    int32_t sbp_topm;             /* VSLAM_SBP_TOPM: the same for SearchByProjection */
    int32_t sbp_sequential;       /* VSLAM_SBP_MODE=seq: 1 = skip the parallel resolution (cross-check path) */
    int32_t si_queries_per_block; /* VSLAM_SI_QPB: 8 | 16 | 32 queries per k_si_topm workgroup (default 16) */
    int32_t fg_threads;           /* VSLAM_FG_NT: 64 | 128 | 256 threads per grid-detector cell (default 128) */
    int32_t wait_spin;            /* VSLAM_WAIT=spin: 1 = host waits poll hipStreamQuery instead of blocking */
    int32_t numa;                 /* VSLAM_NUMA: 0 = do not allocate pinned memory from the CPUs next to the device */
    int32_t host_prof;            /* VSLAM_HOST_PROF: 1 = host-side wall time per API phase, printed at destroy */
    int32_t stream_priority;      /* VSLAM_STREAM_PRIORITY: 0 normal (default), 1 low, 2 high priority of the context's HIP stream: a
                                     priority of its own gives the context hardware queues it does not share with the host
                                     application's other streams -- and, being a priority, lets the context's kernels
                                     pre-empt the application's default-priority work: opt in (bench.py does), see
                                     INTEGRATION.md */
    int32_t stage_split_event;    /* 0..3: uploads of more than one image go as two transfers with the context's user event of that
                                     index (vslam_fe_event_wait) recorded between them; see vslam_fe_stage_images_async */
    int32_t oct_threads;          /* VSLAM_OCT_THREADS: 256 | 512 | 1024 threads per quadtree problem (default: 1024 for contexts of
                                     one or two images, 512 for frames above a megapixel, else 256) */
    int32_t fast_kernel;          /* VSLAM_FAST_KERNEL: 3 = one workgroup per FAST cell (k_fast_cells_v3; default for contexts of one
                                     or two images), 4 = one workgroup per band of cells of a cell row sharing one staged
                                     window (k_fast_bands; default for batches) */
    int32_t fast_band_cells;      /* VSLAM_FAST_BAND_CELLS: cells per band of k_fast_bands (1..4, default 4; fewer where 4 cell
                                     interiors are wider than 128 px) */
    int32_t wave_prio;            /* retired: accepted and ignored */
    int32_t oct_precount;         /* retired: accepted and ignored */
    int32_t desc_kpw;             /* VSLAM_DESC_KPW: 1 | 4 keypoints per wave of the descriptor kernel (default: 1 for contexts of one or
                                     two images, else 4) */
    int32_t pyr_pingpong;         /* VSLAM_PYR_PINGPONG: LDS layout of a fused-pyramid tile.  1 = two regions that alternate levels
                                     reuse, at most 20 KB per tile, so a tile fits where a k_fast_bands workgroup retired; 0 = every
                                     level of the group resident, up to 64 KB.  Default: contexts of more than two images of up to a megapixel
                                     run 1, except for the passes of the stereo-frame entry, which run 0; everything else 0.  A value
                                     set here holds for every entry */
    int32_t reserved[1];
} vslam_tuning;
void vslam_tuning_init(vslam_tuning* t); /* every field = -1 (library default) */

typedef struct vslam_fe_params {
    int32_t width, height;   /* level-0 image size (reference: image.cols/rows at compute()) */
    int32_t nfeatures;       /* ORBextractor.nFeatures   (tracking.cpp:1021-1085) */
    float scale_factor;      /* ORBextractor.scaleFactor */
    int32_t nlevels;         /* ORBextractor.nLevels     */
    int32_t ini_th_fast;     /* ORBextractor.iniThFAST   */
    int32_t min_th_fast;     /* ORBextractor.minThFAST   */
    int32_t device;          /* HIP device ordinal */
    int32_t max_batch;       /* image slots processed per batched call, 1..VSLAM_MAX_BATCH */
    uint32_t flags;          /* VSLAM_FLAG_* */
    int32_t gauss_taps[7];   /* all zero -> OpenCV 4.2 taps {18,34,48,56,48,34,18} */
    const vslam_tuning* tuning; /* NULL: library defaults; copied by vslam_fe_create */
} vslam_fe_params;

typedef struct vslam_fe vslam_fe;

/* ---------------------------------------------------------------- extractor (FExtractor) */

/* FExtractor::FExtractor (fextractor.cpp:401-461): allocates pyramids for max_batch image slots, builds
 * scale tables, per-level quotas, resize coefficient tables and the FAST cell list. */
int vslam_fe_create(const vslam_fe_params* params, vslam_fe** out);
/* Change switches of an existing context between calls (fields >= 0 of *t overwrite the context's; like every other
 * call on a context this is not re-entrant).  Takes effect for what is consulted per call -- the transport routes
 * (h2d_route, d2h_route, pull_depth, copy_wgs), the matcher switches (init_topm, init_match_host, sbp_topm,
 * sbp_sequential, si_queries_per_block), oct_regkeys, the FAST kernel (fast_kernel), graphs = 0; switches that shaped
 * the context's buffers at creation (pyramid plan, blur rows, quadtree grid depth and LDS placement) stay as created. */
int vslam_fe_set_tuning(vslam_fe* fe, const vslam_tuning* t);
void vslam_fe_destroy(vslam_fe* fe);
const char* vslam_last_error(void);

/* FExtractor::GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (fextractor.h:42-62) + mnFeaturesPerLevel.  Arrays of nlevels; any may be NULL. */
int vslam_fe_tables(const vslam_fe* fe, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                    int32_t* features_per_level);

/* FExtractor::compute (fextractor.h:38-40, fextractor.cpp:1034-1133) for one host image, synchronous.
 *   img/pitch : CV_8UC1 rows (or the context's pixel format, vslam_fe_set_pixel_format).   lap0/lap1 : vLappingArea (frame.cpp:107-108 passes {0,0}, :289 {0,1000}).
 *   kps/desc  : caller storage for cap keypoints / cap*32 descriptor bytes; cap >= vslam_fe_capacity(fe).
 *   *n        : keypoints written;  *mono_index : the reference's return value.
 * Uses image slot 0. */
int vslam_fe_extract(vslam_fe* fe, const uint8_t* img, size_t pitch, int lap0, int lap1, vslam_kp* kps,
                     uint8_t* desc, int cap, int* n, int* mono_index);

/* Batched form: nimg (<= max_batch) images in one pass of the kernels; slot i <- imgs[i].
 *   imgs_on_device == VSLAM_IMGS_DEVICE (1): imgs[i] are device pointers, used in place as level 0 (zero
 *   copy).  They must stay valid until the LAST consumer of this pass's level 0 has run: the stereo refinement of
 *   vslam_stereo_match(_batch) / vslam_frame_stereo_* and vslam_fe_level_copy(level 0) read them again -- i.e.
 *   until the next extraction on this context, or until the context is destroyed.
 *   == VSLAM_IMGS_HOST (0): pageable host pointers; rows are copied into the context's pinned staging by its
 *   worker pool, then pulled over PCIe.   == VSLAM_IMGS_PINNED (2): host pointers into pinned (hipHostMalloc /
 *   hipHostRegister'ed, e.g. vslam_host_alloc) memory that the GPU reads directly -- no host-side copy at all;
 *   the memory must stay untouched until the pass has been waited for.
 *   kps/desc/n/mono_index are host arrays of nimg entries;
 *   kps[i] holds cap keypoints, desc[i] cap*32 bytes.  kps/desc may be NULL to keep results on the
 *   device only (read them with vslam_fe_slot_buffers). */
int vslam_fe_extract_batch(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch,
                           int imgs_on_device, int lap0, int lap1, vslam_kp* const* kps,
                           uint8_t* const* desc, int cap, int* n, int* mono_index);

/* Upload only: pull nimg pinned (VSLAM_IMGS_PINNED) or pageable (VSLAM_IMGS_HOST) host images into level 0 of slots
 * 0..nimg-1, enqueued on fe's stream, and return.  A following extraction with imgs_on_device == VSLAM_IMGS_STAGED uses
 * them.  Splitting the upload from the extraction lets a pipelined caller start the PCIe transfer of the next pass
 * before the GPU-side dependencies of the extraction itself (e.g. another context's matcher still reading this
 * context's previous RESULTS -- the upload only overwrites level 0, which nothing outside the context reads). */
int vslam_fe_stage_images_async(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch, int imgs_where);

/* The same in two halves, so a caller can keep several contexts (streams) in flight: _async enqueues the
 * whole pass and returns without waiting for the GPU (with the device quadtree nothing in it touches the
 * host); _wait blocks until that pass is done and delivers the results like vslam_fe_extract_batch.
 * want_host = 1 also enqueues the D2H of keypoints and descriptors (0: they stay in HBM, only the counts travel).
 * want_host = 2 (full batches): the delivery is DEFERRED to the device SearchForInitialization that follows on this
 * context (vslam_search_init_dev_async with at most max_batch pairs): counts, keypoints, descriptors and the matcher's
 * outputs lie in one block and leave in ONE transfer behind the matcher; if no such call follows, _wait delivers.
 * Device images: lifetime as above; pinned host images must stay untouched until _wait returns. */
int vslam_fe_extract_batch_async(vslam_fe* fe, int nimg, const uint8_t* const* imgs, size_t pitch,
                                 int imgs_on_device, int lap0, int lap1, int want_host);
int vslam_fe_extract_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                          int* mono_index);

/* FExtractor::mvImagePyramid[level] (fextractor.h:64; read by frame.cpp:830,920,932,937).  Copies the
 * borderless level image of a slot into dst (dst_pitch >= level width).  blurred != 0 returns the
 * GaussianBlur'ed clone used for the descriptors (fextractor.cpp:1085-1086). */
int vslam_fe_level_size(const vslam_fe* fe, int level, int* w, int* h);

/* Keypoint capacity of one image slot = the most keypoints one extraction can return: nfeatures + 4*nlevels + 8
 * rounded up to a multiple of 4, or -- for very small nfeatures -- the exact bound of the quadtree
 * (sum over levels of max(quota + 3, 4 * initial nodes)) if that is larger.  Size caller arrays with it. */
int vslam_fe_capacity(const vslam_fe* fe);
int vslam_fe_level_copy(vslam_fe* fe, int slot, int level, int blurred, uint8_t* dst, size_t dst_pitch);

/* Stage taps for parity tests and profilers: per-level FAST candidates of the last extract of a slot in
 * the reference's vToDistributeKeys order (fextractor.cpp:769-817): x,y relative to the 16-px border,
 * response = FAST score.  Returns the count (or a negative error); writes at most cap entries. */
int vslam_fe_candidates(vslam_fe* fe, int slot, int level, vslam_kp* out, int cap);

/* Device-resident outputs of the last extract of a slot (valid until the next extract on this context):
 * keypoints (vslam_kp[n]) and descriptors (n*32 bytes) in HBM, for device-side matching / RCCL. */
int vslam_fe_slot_buffers(vslam_fe* fe, int slot, const vslam_kp** dev_kps, const uint8_t** dev_desc,
                          int* n);

/* Host-side views of the same results: the context's pinned staging that the result kernel fills
 * (vslam_kp[cap] / cap*32 bytes per slot).  After vslam_fe_extract_wait / vslam_frame_stereo_wait with
 * kps == desc == NULL (n != NULL) the first n[slot] entries are valid until the next enqueue on this context --
 * a consumer that reads them in place saves the copy into its own arrays. */
int vslam_fe_slot_host_views(vslam_fe* fe, int slot, const vslam_kp** host_kps, const uint8_t** host_desc);

/* GPU-side ordering between two contexts of one device: work enqueued on `waiter` after this call runs
 * after everything enqueued on `signal` so far (event record + stream wait, no host synchronisation). */
int vslam_fe_wait_for(vslam_fe* waiter, vslam_fe* signal);
/* Finer grain: four user events per context.  _record marks the current end of fe's stream; _wait makes the
 * waiter's stream wait for the last recorded instance of the signal context's event idx (0..3). */
int vslam_fe_event_record(vslam_fe* fe, int idx);
int vslam_fe_event_wait(vslam_fe* waiter, vslam_fe* signal, int idx);

/* Pacing between contexts kept in flight: with a gate set, the FAST launch of every later pass of `fe` starts only when the
 * FAST launch of `signal`'s latest pass has finished (GPU-side event; no host synchronisation).  FAST takes a CU's whole
 * LDS while it runs; chaining the contexts' FAST launches keeps two of them from being resident at once.  NULL removes it.
 * Destroying `signal` removes the gate (later passes of `fe` run un-gated); do not destroy it from another thread while a
 * pass of `fe` is being enqueued.  Passes of gated contexts are not replayed from captured graphs. */
int vslam_fe_set_fast_gate(vslam_fe* fe, vslam_fe* signal);

/* Stream the context launches on (hipStream_t as void*), for event timing by the caller. */
void* vslam_fe_stream(vslam_fe* fe);

/* Pack the results of slots 0..nslots-1 into caller device memory (e.g. this rank's send buffer of an
 * RCCL exchange): per slot `slot_bytes` >= 16 + cap*60 laid out as
 *   int32 n, mono_index, cap, 0 | vslam_kp[cap] | uint8 desc[cap][32]      (cap = vslam_fe_capacity(fe))
 * Returns after the copies have completed. */
int vslam_fe_pack_slots(vslam_fe* fe, int nslots, void* dev_dst, size_t slot_bytes);
/* the same for slots first .. first+nslots-1 (packed from offset 0 of dev_dst) */
int vslam_fe_pack_slot_range(vslam_fe* fe, int first, int nslots, void* dev_dst, size_t slot_bytes);
/* enqueue-only variant: the copies run on fe's stream after the pass that produced the slots; the caller
 * orders later readers (stream sync / event) itself */
int vslam_fe_pack_slot_range_async(vslam_fe* fe, int first, int nslots, void* dev_dst, size_t slot_bytes);

/* ---------------------------------------------------------------- multi-GPU exchange step (RCCL over xGMI)
 *
 * The reference is single-GPU/CPU; BASELINE.json's north_star shards frames one per GPU and names
 * ONE exchange: the predecessor frame's descriptors + keypoint geometry for the cross-frame matchers
 * (FMatcher::SearchForInitialization fmatcher.cpp:983-1098, SearchByProjection(Current, Last) :2471-2687).
 * One process per GPU; rank 0 makes an id (vslam_comm_unique_id), the launcher distributes its 128 bytes (any
 * channel: torch.distributed store, MPI, a file), every rank calls vslam_comm_create.  The exchange functions only
 * ENQUEUE on fe's stream (behind vslam_fe_pack_slot_range_async, ahead of the matcher): no host synchronisation.
 * RCCL is loaded at run time (librccl.so.1); without it these return VSLAM_ERR_COMM and everything else works. */
#define VSLAM_COMM_ID_BYTES 128
typedef struct vslam_comm vslam_comm;
int vslam_comm_unique_id(uint8_t id[VSLAM_COMM_ID_BYTES]);
int vslam_comm_create(int device, int rank, int world, const uint8_t id[VSLAM_COMM_ID_BYTES], vslam_comm** out);
void vslam_comm_destroy(vslam_comm* comm);
int vslam_comm_rank(const vslam_comm* comm);
int vslam_comm_world(const vslam_comm* comm);
/* Ring shift: `bytes` of dev_send go to rank+1, dev_recv receives rank-1's block (frame g lives on rank g % world,
 * so every predecessor frame lives on the left neighbour): one ncclSend/ncclRecv pair in a group. */
int vslam_exchange_ring(vslam_fe* fe, vslam_comm* comm, const void* dev_send, void* dev_recv, size_t bytes);
/* The north_star-literal variant: all-gather, dev_recv_all = world x bytes_per_rank (rank r's block at r*bytes). */
int vslam_exchange_allgather(vslam_fe* fe, vslam_comm* comm, const void* dev_send, void* dev_recv_all,
                             size_t bytes_per_rank);

/* Pinned host memory for VSLAM_IMGS_PINNED inputs (hipHostMalloc: the GPU reads it over PCIe without a staging copy). */
int vslam_host_alloc(size_t bytes, void** out);
void vslam_host_free(void* p);

/* Stage timing with HIP events on the context's stream (the reference's REGISTER_TIMES spans,
 * frame.cpp:103-132, broken down per kernel stage): stage_ms[0..4] = pyramid (7 launches), FAST cells,
 * Gaussian blur, orientation+descriptor, quadtree distribution + output order (with the host quadtree a zero-length
 * span behind the upload of the selected keypoints: that work is host time inside the enqueue call, not stream time),
 * accumulated over `batches` batched calls / `images` images since profiling was switched on. */
int vslam_fe_set_profiling(vslam_fe* fe, int on);
int vslam_fe_get_profile(vslam_fe* fe, double stage_ms[5], long* batches, long* images);

/* ---------------------------------------------------------------- matcher (FMatcher / Frame) */

/* FMatcher::DescriptorDistance (fmatcher.h:77, fmatcher.cpp:2859-2875) over device arrays: all-pairs
 * 256-bit Hamming, two nearest train descriptors per query (the cv::BFMatcher::knnMatch(…,2) sites,
 * frame.cpp:1167-1174; fmatcher.cpp:204-229).  q/t: nq*32 / nt*32 bytes in HBM.  idx2/dist2: host arrays
 * of nq*2 (first = best; ties -> lower train index; missing -> idx -1, dist 2^31-1).
 * Runs on fe's stream and device. */
int vslam_hamming_top2(vslam_fe* fe, const uint8_t* dev_q, int nq, const uint8_t* dev_t, int nt,
                       int32_t* idx2, int32_t* dist2);

/* The same for nprob (<= 32) INDEPENDENT problems in one launch -- e.g. the brute-force matches of all stereo pairs of a
 * step (frame.cpp:1167-1174 once per frame): problem p matches dev_q[p] (nq[p] x 32 bytes in HBM) against dev_t[p]
 * (nt[p] <= 65535).  idx2[p] / dist2[p]: host arrays of nq[p] * 2 entries, semantics as above. */
int vslam_hamming_top2_batch(vslam_fe* fe, int nprob, const uint8_t* const* dev_q, const int32_t* nq,
                             const uint8_t* const* dev_t, const int32_t* nt, int32_t* const* idx2, int32_t* const* dist2);
/* Enqueue-only form for pipelines and profilers: the same launch on fe's stream, nothing waited for or copied; the results
 * stay in the context's device arrays (rows of all problems back to back).  Sizes as in a previous vslam_hamming_top2_batch
 * on this context (which allocates); VSLAM_ERR_INVALID otherwise. */
int vslam_hamming_top2_batch_dev_async(vslam_fe* fe, int nprob, const uint8_t* const* dev_q, const int32_t* nq,
                                       const uint8_t* const* dev_t, const int32_t* nt);

/* Frame::ComputeStereoFishEyeMatches (frame.cpp:1149-1174), descriptor half: cv::BFMatcher(NORM_HAMMING).knnMatch of the
 * lapping-area descriptors -- left rows [mono_left, n_left) against right rows [mono_right, n_right), k = 2 -- and the
 * ratio test `m[0].distance < m[1].distance * 0.7` (a float times a double literal: compared in double).
 * left_to_right[i] (n_left entries, host): index of the right keypoint (in the FULL right list, i.e. + mono_right) for every
 * left keypoint that passes, else -1; best_dist / second_dist (nullable): the two Hamming distances; *n_candidates = the
 * reference's descMatches.  The triangulation that decides mvLeftToRightMatch / mvDepth from these pairs
 * (KannalaBrandt8::TriangulateMatches, :1176-1188) belongs to the camera model and stays with the caller. */
int vslam_stereo_fisheye_candidates(vslam_fe* fe, const uint8_t* dev_desc_left, int n_left, int mono_left,
                                    const uint8_t* dev_desc_right, int n_right, int mono_right, int32_t* left_to_right,
                                    int32_t* best_dist, int32_t* second_dist, int* n_candidates);

/* Dense distance matrix (nq x nt, uint8, 255 = distance >= 255) on the device -> host; used by the
 * order-dependent matchers whose sequential part is replayed on the host. */
int vslam_hamming_matrix(vslam_fe* fe, const uint8_t* dev_q, int nq, const uint8_t* dev_t, int nt,
                         uint8_t* out);

/* Frame::ComputeStereoMatches (frame.h:293, frame.cpp:823-997) for the pair (feL slot sL, feR slot sR)
 * after both have been extracted.  bf = Camera.bf, fx = Camera.fx.  u_right/depth: host arrays of the
 * left keypoint count (mvuRight, mvDepth; -1 = no match).  feL and feR may be the same context. */
int vslam_stereo_match(vslam_fe* feL, int sL, vslam_fe* feR, int sR, float bf, float fx, float* u_right,
                       float* depth);

/* The same for npairs (<= 32) stereo pairs in one pass of the kernels: pair j = (feL slot slotsL[j],
 * feR slot slotsR[j]); u_right[j]/depth[j] are host arrays of that pair's left keypoint count. */
int vslam_stereo_match_batch(vslam_fe* feL, vslam_fe* feR, int npairs, const int* slotsL, const int* slotsR,
                             float bf, float fx, float* const* u_right, float* const* depth);

/* The extraction + stereo-match section of Frame::Frame(imLeft, imRight, ...) (frame.cpp:102-132) for
 * npairs (<= 32, 2*npairs <= max_batch) stereo frames in ONE enqueue on fe's stream: imgs = L0,R0,L1,R1,...
 * (slot 2j = left, 2j+1 = right of frame j; vLappingArea {0,0} as the reference passes, frame.cpp:107-108).
 * _async returns without waiting; _wait delivers keypoints/descriptors of all 2*npairs images (arrays of
 * 2*npairs entries, may be NULL) and mvuRight/mvDepth of the npairs left images. */
int vslam_frame_stereo_batch_async(vslam_fe* fe, int npairs, const uint8_t* const* imgs, size_t pitch,
                                   int imgs_on_device, float bf, float fx, int want_host);
int vslam_frame_stereo_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                            float* const* u_right, float* const* depth);

/* The extraction + depth section of Frame::Frame(imGray, imDepth, ...) (frame.cpp:185-257) for nframes (<= max_batch) RGB-D
 * frames in ONE enqueue on fe's stream: slot j <- imgs[j] (the context's pixel format; vLappingArea {0,0},
 * ExtractORB(0, imGray, 0, 0)), Frame::UndistortKeyPoints if the context has a camera, then Frame::ComputeStereoFromRGBD
 * (:1000-1021) on the device, one lane per keypoint:
 *     d = imDepth.at<float>((int)kp.y, (int)kp.x)       kp = keypoints_[i]: truncation toward zero
 *     d > 0:  mvDepth[i] = d,  mvuRight[i] = ukeypoints_[i].pt.x - bf / d          else both -1 (NaN, zero, negative)
 * imDepth is the caller's depth image after Tracking::GrabImageRGBD's conversion (tracking.cpp:1305-1306): a sample is
 * multiplied by depth_map_factor in float if depth_type != VSLAM_DEPTH_F32 or fabsf(depth_map_factor - 1.0f) > 1e-5, and
 * taken raw otherwise.  depth_map_factor is the reference's mDepthMapFactor, i.e. the MULTIPLIER 1 / DepthMapFactor
 * (tracking.cpp:1108-1113).  A sample position outside the depth image gives -1; keypoints of this extractor never lie
 * there and the reference does not test for it.
 * depth[j]: width x height samples of the context's size, rows depth_pitch bytes apart.  depth_where = VSLAM_IMGS_DEVICE or
 * VSLAM_IMGS_PINNED: read IN PLACE by the kernel (only the samples under keypoints are touched); VSLAM_IMGS_HOST (pageable):
 * copied into pinned staging of the context first -- the context has ONE such staging, so with pageable depth images the
 * call first waits on the host for everything enqueued on fe's stream before (it is synchronous with the previous pass;
 * pin the depth images to keep several passes in flight).  Pinned and pageable depth images must stay untouched until _wait
 * returns.  The depth gather is a plain launch behind the (possibly replayed) extraction: no captured graph holds a depth
 * pointer.
 * mvuRight / mvDepth lie where vslam_frame_stereo_batch_async puts them (full batches with want_host != 0: behind the
 * extraction's results, the step leaves in one transfer), "pair j" = frame j = slot j: vslam_stereo_points_dev_async and
 * vslam_stereo_points_buffers work after an RGB-D pass as after a stereo pass, with their own limit: at most 16 pairs per call
 * and pair indices below 16, so only frames 0..15 of a larger RGB-D batch can be unprojected (mvuRight / mvDepth of all frames
 * are delivered by _wait).  want_host: 0 keypoints and descriptors
 * stay in HBM (counts, mvuRight and mvDepth still travel), 1 or 2 delivered.  _wait delivers like vslam_frame_stereo_wait:
 * arrays of nframes entries, any may be NULL. */
#define VSLAM_DEPTH_U16 0 /* CV_16UC1 */
#define VSLAM_DEPTH_F32 1 /* CV_32FC1 */
int vslam_frame_rgbd_batch_async(vslam_fe* fe, int nframes, const uint8_t* const* imgs, size_t pitch, int imgs_where,
                                 const void* const* depth, size_t depth_pitch, int depth_type, int depth_where,
                                 float depth_map_factor, float bf, int want_host);
/* VSLAM_ERR_INVALID unless the last pass enqueued on fe was an RGB-D pass. */
int vslam_frame_rgbd_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                          float* const* u_right, float* const* depth);
/* With vslam_fe_set_profiling on: HIP-event time of the depth gather (k_rgbd_depth) alone, summed over the RGB-D passes
 * waited for since profiling was switched on.  Either pointer may be NULL. */
int vslam_fe_get_rgbd_profile(vslam_fe* fe, double* depth_ms, long* passes);

/* FMatcher::SearchForInitialization (fmatcher.h:106, fmatcher.cpp:983-1098).  Frame 1 / frame 2
 * keypoints+descriptors are device arrays (e.g. from vslam_fe_slot_buffers, or a slot of an RCCL
 * exchange buffer); kps1_host/kps2_host are the same keypoints on the host.  prev_matched: 2*n1 floats
 * in/out (vbPrevMatched).  matches12: n1 ints out.  Returns the match count in *nmatches. */
int vslam_search_for_initialization(vslam_fe* fe, const vslam_kp* kps1_host, const uint8_t* dev_desc1,
                                    int n1, const vslam_kp* kps2_host, const uint8_t* dev_desc2, int n2,
                                    int img_w, int img_h, float* prev_matched, int32_t* matches12,
                                    int window, float nnratio, int check_orientation, int* nmatches);

/* npairs (<= 32) independent SearchForInitialization problems in one pass: the dense distance matrices of
 * all pairs come from one kernel launch, the order-dependent replays run in parallel on the host pool.
 * Every per-pair argument of the single form becomes an array of npairs entries. */
int vslam_search_for_initialization_batch(vslam_fe* fe, int npairs, const vslam_kp* const* kps1_host,
                                          const uint8_t* const* dev_desc1, const int* n1,
                                          const vslam_kp* const* kps2_host, const uint8_t* const* dev_desc2,
                                          const int* n2, int img_w, int img_h, float* const* prev_matched,
                                          int32_t* const* matches12, int window, float nnratio,
                                          int check_orientation, int* nmatches);

/* Device-resident form: every pointer of a job is a DEVICE pointer -- keypoints/descriptors as returned by
 * vslam_fe_slot_buffers (or a slot of an RCCL exchange buffer packed by vslam_fe_pack_slots), the keypoint
 * counts as int32 in HBM (vslam_fe_slot_count_ptr, or the header word of a packed slot).  The whole matcher
 * (window query, Hamming distances, stealing, ratio test, rotation histogram) runs in one kernel, one wave per
 * pair, on fe's stream; _async returns without waiting, _wait delivers n1[j] entries of vnMatches12 and the
 * updated vbPrevMatched per pair plus the match counts.  dev_prev_matched == NULL means "frame 1's keypoint
 * positions" (tracking.cpp:2281-2288 initialises vbPrevMatched that way). */
typedef struct vslam_init_job {
    const vslam_kp* dev_kps1;
    const uint8_t* dev_desc1;
    const int32_t* dev_n1;
    const vslam_kp* dev_kps2;
    const uint8_t* dev_desc2;
    const int32_t* dev_n2;
    const float* dev_prev_matched;
} vslam_init_job;
int vslam_search_init_dev_async(vslam_fe* fe, int npairs, const vslam_init_job* jobs, int img_w, int img_h,
                                int window, float nnratio, int check_orientation);
int vslam_search_init_dev_wait(vslam_fe* fe, const int* n1, int32_t* const* matches12, float* const* prev_matched,
                               int* nmatches);
/* device address of a slot's keypoint count (int32), valid for the life of the context */
int vslam_fe_slot_count_ptr(vslam_fe* fe, int slot, const int32_t** dev_n);

/* ---------------------------------------------------------------- two-view consensus (MotionEstimator::Reconstruct)
 *
 * The monocular initialiser calls mpCamera->ReconstructWithTwoViews right behind SearchForInitialization
 * (tracking.cpp:2324 -> :2339; pinhole.cpp:98-106; motion_estimation.cpp:2006-2094).  Its two RANSAC loops, FindHomography
 * and FindFundamental (:2096-2195), have no early exit: mMaxIterations hypotheses each, every one scored over every match by
 * CheckHomography (:2277-2360) or CheckFundamental (:2362-2440), plain float arithmetic without an OpenCV call.  This
 * section is that scoring and the selection of the loops (:2137-2142, :2188-2193) for all hypotheses of both models and
 * for a batch of frame pairs, in one enqueue.  HYPOTHESIS GENERATION STAYS WITH THE CALLER: the 8-point sets
 * (DUtils::Random on the process-global rand() state), Normalize, ComputeH21 / ComputeF21 (cv::SVDecomp, whose arithmetic
 * depends on how OpenCV was built), T2inv*Hn*T1, H21i.inv() and T2t*Fn*T1 -- the caller runs loop one to fill H21 / H12 /
 * F21, calls this once, and goes on with RH = SH / (SH + SF) and ReconstructH / ReconstructF.
 *
 * The pair list (:2017-2029) is (i, matches12[i]) for ascending i with matches12[i] >= 0; every result is in that order.
 * Arithmetic: vi_slam_amd/csrc/vslam_two_view.h -- each operation rounded on its own, associated as the C source reads,
 * subnormals kept, the score a serial float chain over the pairs (image 1 term, then image 2 term) from zero.  A NaN chi
 * (a projective w of exactly zero, 0/0 in the epipolar distance) is not `> th`: the pair counts as an inlier and the score
 * becomes NaN, which never wins (`currentScore > score` is false).  The winner is the lowest index with the maximal score,
 * if that score is > 0; otherwise best = -1, the score is 0 and the mask all zero.
 * Deviations: without a winner the reference's FindFundamental leaves a mask of length 0 (:2150 reads the size of an empty
 * vector), here it has n_pairs zeros; a NaN score is reported as the quiet NaN 0x7fc00000 whatever sign and payload the
 * host's arithmetic would leave (nothing in the reference observes them).
 * Limits: njobs <= VSLAM_TWO_VIEW_MAX_JOBS, nH / nF <= VSLAM_TWO_VIEW_MAX_HYP, n1 <= 65536.  A job with more than
 * VSLAM_TWO_VIEW_MAX_PAIRS pairs makes _wait return VSLAM_ERR_UNSUPPORTED, a matches12 entry >= n2 (the reference would
 * read out of bounds) VSLAM_ERR_INVALID; n_pairs of every job is delivered all the same, the failing job has no winner.
 * sigma must be finite and not zero.  n_pairs == 0 is valid: no winner, both scores 0. */
#define VSLAM_TWO_VIEW_MAX_JOBS 32
#define VSLAM_TWO_VIEW_MAX_HYP 1024
#define VSLAM_TWO_VIEW_MAX_PAIRS 8192
typedef struct vslam_two_view_job {
    const vslam_kp* kps1; const vslam_kp* kps2;   /* ukeypoints_ of frame 1 / 2 */
    int32_t n1, n2;
    const int32_t* matches12;                     /* n1 entries, -1 = unmatched */
    int32_t kps_on_device, matches_on_device;     /* 0 host (uploaded with the block), 1 HBM */
    const float* H21; const float* H12; int32_t nH; /* host, nH x 9 row-major each; nH may be 0 */
    const float* F21; int32_t nF;                   /* host, nF x 9; nF may be 0 */
    float sigma;                                    /* MotionEstimator's mSigma (1.0) */
} vslam_two_view_job;

typedef struct vslam_two_view_result {            /* caller storage; any pointer may be NULL */
    int32_t n_pairs, best_h, best_f;  float score_h, score_f;   /* SH, SF of Reconstruct */
    int32_t* pairs;                   /* 2 * n_pairs: (i, matches12[i]) */
    float* scores_h; float* scores_f; /* nH / nF: every hypothesis' currentScore */
    uint8_t* inliers_h; uint8_t* inliers_f;       /* n_pairs each, the winner's */
} vslam_two_view_result;

/* upload (job table | hypotheses | host keypoints and matches, one range) -> k_tv_pairs -> k_tv_score -> k_tv_select ->
 * one result copy, all on fe's stream without a host wait.  One enqueue per context may be in flight; device arrays must
 * stay valid and unchanged until _wait.  `results`: njobs entries; the arrays a job's result points to hold n1 pairs at
 * most (min(n1, VSLAM_TWO_VIEW_MAX_PAIRS)). */
int vslam_two_view_score_async(vslam_fe* fe, int njobs, const vslam_two_view_job* jobs);
int vslam_two_view_score_wait(vslam_fe* fe, vslam_two_view_result* results);
int vslam_two_view_score(vslam_fe* fe, const vslam_two_view_job* job, vslam_two_view_result* result);
/* With vslam_fe_set_profiling on: HIP-event time of k_tv_pairs, k_tv_score and k_tv_select alone, summed over the calls
 * waited for since vslam_fe_set_profiling was last called: it starts these sums anew.  Any pointer may be NULL. */
int vslam_fe_get_two_view_profile(vslam_fe* fe, double* pairs_ms, double* score_ms, double* select_ms, long* passes);

/* ---------------------------------------------------------------- distorted pinhole cameras (Frame::ukeypoints_)
 *
 * Frame::UndistortKeyPoints (frame.cpp:758-790) runs cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) on
 * the keypoints right after extraction, and Frame::ComputeImageBounds (:793-821) undistorts the image corners into the
 * float grid bounds mnMinX/mnMaxX/mnMinY/mnMaxY.  With a camera set, every extraction pass of the context
 * (vslam_fe_extract*, the async/wait forms, vslam_frame_stereo_batch_async) also writes the undistorted keypoints of
 * each slot to the device (one small launch behind the descriptors; captured graphs include it).  The reference only
 * tests k1: with k1 == 0 ukeypoints_ = keypoints_ even if k2, p1, p2 or k3 are not zero, and so does this library (no
 * launch; the slot's keypoint array doubles as its undistorted one).  Contexts without a camera launch nothing extra. */
typedef struct vslam_camera {
    float fx, fy, cx, cy; /* Pinhole::toK (CV_32F) */
    float dist[5];        /* mDistCoef: k1, k2, p1, p2[, k3] */
    int32_t ndist;        /* 4 or 5 */
} vslam_camera;
/* NULL = no camera (the default).  Drops the context's captured graph, so the next pass captures with the new one. */
int vslam_fe_set_camera(vslam_fe* fe, const vslam_camera* cam);
/* Device address of a slot's ukeypoints_ (vslam_kp[cap], n = the slot's count; valid until the next extraction, fixed
 * for the life of the context): the slot's keypoint array itself when k1 == 0.  VSLAM_ERR_INVALID without a camera. */
int vslam_fe_slot_ukps(vslam_fe* fe, int slot, const vslam_kp** dev_ukps);
/* Waits for fe's stream, then copies the slot's ukeypoints_ (*n entries) to dst; VSLAM_ERR_CAPACITY if cap < *n. */
int vslam_fe_ukps_copy(vslam_fe* fe, int slot, vslam_kp* dst, int cap, int* n);
/* cv::undistortPoints with the context's camera (k1 == 0: unchanged) of n points, xy / out_xy interleaved host arrays;
 * evaluated on the device by the arithmetic of the keypoint kernel.  VSLAM_ERR_INVALID without a camera. */
int vslam_undistort_points(vslam_fe* fe, const float* xy, int n, float* out_xy);
/* Frame::ComputeImageBounds on level 0: bounds = minX, maxX, minY, maxY; {0, width, 0, height} without a camera or
 * with k1 == 0. */
int vslam_fe_image_bounds(vslam_fe* fe, float bounds[4]);

/* The three SearchForInitialization entry points over frame 2's float grid bounds (vslam_fe_image_bounds) instead of
 * img_w / img_h: mfGridElementWidthInv = (float)64 / (maxX - minX), PosInGrid = round((x - minX) * inv), window cells
 * floor((x - minX - r) * inv) .. ceil((x - minX + r) * inv) (frame.cpp:322-323, 678-756).  The img_w / img_h forms are
 * these with {0, img_w, 0, img_h}.  Keypoints are typically ukeypoints_ (vslam_fe_slot_ukps / vslam_fe_ukps_copy);
 * in a device job dev_prev_matched == NULL then means frame 1's undistorted positions (tracking.cpp:2286-2288).
 * The bounds must be finite with max > min (VSLAM_ERR_INVALID otherwise). */
typedef struct vslam_bounds {
    float min_x, max_x, min_y, max_y;
} vslam_bounds;
int vslam_search_for_initialization_ex(vslam_fe* fe, const vslam_kp* kps1_host, const uint8_t* dev_desc1, int n1,
                                       const vslam_kp* kps2_host, const uint8_t* dev_desc2, int n2, const vslam_bounds* b,
                                       float* prev_matched, int32_t* matches12, int window, float nnratio,
                                       int check_orientation, int* nmatches);
int vslam_search_for_initialization_batch_ex(vslam_fe* fe, int npairs, const vslam_kp* const* kps1_host,
                                             const uint8_t* const* dev_desc1, const int* n1,
                                             const vslam_kp* const* kps2_host, const uint8_t* const* dev_desc2,
                                             const int* n2, const vslam_bounds* b, float* const* prev_matched,
                                             int32_t* const* matches12, int window, float nnratio, int check_orientation,
                                             int* nmatches);
int vslam_search_init_dev_async_ex(vslam_fe* fe, int npairs, const vslam_init_job* jobs, const vslam_bounds* b,
                                   int window, float nnratio, int check_orientation);

/* The grid bounds of every matcher that runs after initialisation.  In the reference mnMinX / mnMaxX / mnMinY / mnMaxY
 * are static members of Frame (frame.cpp:28), computed once on the first frame and copied into every KeyFrame
 * (keyframe.cpp:44): a property of the camera, so here a property of the context, next to its camera.  While bounds are
 * set,
 *   vslam_search_by_projection_frame / _keyframe / _sim3 (both proj_variants) / _mappoints,
 *   vslam_search_by_projection_dev_async / _wait and vslam_fuse_search (sim3 = 0, 1, 2)
 * take them from the context -- the 64 x 48 grid (mfGridElementWidthInv = (float)64 / (maxX - minX), PosInGrid =
 * round((x - minX) * inv), frame.cpp:322-323, 746-756), the window cells of GetFeaturesInArea (frame.cpp:678-744,
 * keyframe.cpp:655-699) and the in-image test of the projection (u < mnMinX || u > mnMaxX in the Frame / KeyFrame-into-
 * Frame forms, fmatcher.cpp:2514-2517, 2719-2722; KeyFrame::IsInImage, x >= mnMinX && x < mnMaxX, in the Sim3 forms, Fuse
 * and SearchBySim3) -- and read the img_w / img_h of their own parameters only to validate them as before.  Keypoints are
 * then ukeypoints_ (vslam_fe_slot_ukps / vslam_fe_ukps_copy) and the bounds those of vslam_fe_image_bounds.
 * The KeyFrame-side forms (_sim3, vslam_fuse_search) reproduce what a KeyFrame does with them: it stores the four bounds as
 * `const int` (keyframe.h:255-258), truncated toward zero, keeps the Frame's cells and float grid inverses, and reads the
 * integers for the window origin of KeyFrame::GetFeaturesInArea and in KeyFrame::IsInImage -- a projection between mnMinX and
 * ceil(mnMinX), or between floor(mnMaxX) and mnMaxX, is outside for them.  The caller always passes the Frame's floats.
 * b == NULL = none (the default): every matcher uses {0, img_w, 0, img_h} of its own parameters, as before.  Bounds must
 * be finite with max > min; VSLAM_ERR_INVALID otherwise, and the previous setting stays in force.  Like every call on a
 * context the setter is not re-entrant: do not call it while another thread runs a matcher on fe.
 * The SearchForInitialization entry points above keep their explicit bounds argument (img_w / img_h or the _ex forms'
 * vslam_bounds) and do not consult the context's bounds. */
int vslam_fe_set_grid_bounds(vslam_fe* fe, const vslam_bounds* b);
/* The bounds in force; *is_set = 0 and {0, width, 0, height} of the context when none are set. */
int vslam_fe_get_grid_bounds(const vslam_fe* fe, vslam_bounds* b, int* is_set);

/* ---------------------------------------------------------------- colour input images
 *
 * Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular (tracking.cpp:1235-1258, 1285-1303, 1324-1336) turn a 3- or
 * 4-channel image into gray with cv::cvtColor(im, im, COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) before anything else.  The pixel
 * format is a property of the context, like its camera and its grid bounds.  With a format other than VSLAM_PIX_GRAY8
 * every entry that takes images -- vslam_fe_extract, _extract_batch, _extract_batch_async, vslam_fe_stage_images_async,
 * vslam_frame_stereo_batch_async, vslam_frame_rgbd_batch_async -- reads imgs[i] as interleaved pixels of 3 or 4 bytes,
 * rows `pitch` >= width * bytes-per-pixel bytes apart (any such pitch, odd ones included), and one kernel
 * (k_gray_images) writes the gray image into level 0 of the slot:
 *     gray = (R * cr + G * cg + B * cb + (1 << (shift - 1))) >> shift          alpha ignored
 *     shift 15: (cr, cg, cb) = (9798, 19235, 3735)   OpenCV 4.x 8-bit RGB2Gray (the default)
 *     shift 14: (cr, cg, cb) = (4899,  9617, 1868)   OpenCV 3.x
 * The coefficients are restated from OpenCV, not checked against a build of it here (tools/dump_opencv_cvtcolor.cpp is the
 * route to settle them), which is why the shift is a knob.  VSLAM_IMGS_DEVICE images of a colour format are NOT used in
 * place: level 0 lives in the context's pyramid and the caller's buffer is free once the pass has run.
 * Setting a format waits for the context's stream, drops its captured graph and sizes its pinned and device staging for
 * the wider rows.  VSLAM_PIX_GRAY8 restores the gray path exactly, zero copy for device images included.  The grid
 * detector (vslam_fastgrid.h) keeps gray input. */
#define VSLAM_PIX_GRAY8 0 /* default */
#define VSLAM_PIX_RGB8 1
#define VSLAM_PIX_BGR8 2
#define VSLAM_PIX_RGBA8 3
#define VSLAM_PIX_BGRA8 4
/* gray_shift: 0 = default (15), 14 or 15; VSLAM_ERR_INVALID for anything else or an unknown fmt (the setting in force stays) */
int vslam_fe_set_pixel_format(vslam_fe* fe, int fmt, int gray_shift);
int vslam_fe_get_pixel_format(const vslam_fe* fe, int* fmt, int* gray_shift);

/* ---------------------------------------------------------------- diagnostics */

/* FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * (fmatcher.h, fmatcher.cpp:2471-2687; pinhole frames, Nleft == -1) -- the tracking matcher of
 * TrackWithMotionModel (tracking.cpp:2728).  What the function reads of the two frames is passed explicitly:
 *   p            pose of CurrentFrame as rows [Rcw | tcw] (the reference's T_w_c_ member is used that way),
 *                pinhole intrinsics, mbf, th, bForward/bBackward (vslam_projection_direction), image bounds of
 *                CurrentFrame's grid (mnMinX = mnMinY = 0, mnMaxX = img_w, mnMaxY = img_h; the context's bounds
 *                instead while vslam_fe_set_grid_bounds has set some)
 *   last frame   host arrays of n_last entries: keypoints (octave from keypoints_, angle from ukeypoints_),
 *                flags (bit0: mvpMapPoints[i] != NULL && !mvbOutlier[i]; bit1: that MapPoint has
 *                Observations() > 0), world positions (3 floats), MapPoint descriptors (32 bytes)
 *   current      DEVICE keypoints/descriptors (vslam_fe_slot_buffers), n_cur <= 4096; host mvuRight (NULL =
 *                monocular, all -1) and the initial "mvpMapPoints[i2] with Observations() > 0" mask (NULL = none:
 *                tracking.cpp fills mvpMapPoints with NULL before the call)
 * Output: match_cur[i2] = index i of the last-frame keypoint whose MapPoint ends up in mvpMapPoints[i2], or -1;
 * *nmatches as the reference counts it. */
typedef struct vslam_proj_params {
    float Tcw[12];
    float fx, fy, cx, cy, mbf, th;
    int32_t forward, backward;
    int32_t check_orientation;
    int32_t img_w, img_h;
    int32_t gemm_float; /* 0: Rcw*x+tcw as cv::gemm evaluates it (double accumulation); 1: float arithmetic */
} vslam_proj_params;
int vslam_projection_direction(const float* Tcw, const float* Tlw, float mb, int mono, int gemm_float,
                               int* forward, int* backward);
int vslam_search_by_projection_frame(vslam_fe* fe, const vslam_proj_params* p, const vslam_kp* last_kps_host,
                                     int n_last, const uint8_t* last_flags, const float* last_x3dw,
                                     const uint8_t* mp_desc_host, const vslam_kp* dev_cur_kps,
                                     const uint8_t* dev_cur_desc, int n_cur, const float* cur_u_right_host,
                                     const uint8_t* cur_occupied_host, int32_t* match_cur, int* nmatches);

/* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (fmatcher.cpp:2689-2811) -- the matcher of Tracking::Relocalization.  p carries T_w_c_'s Rcw | tcw in Tcw, the camera,
 * th, check_orientation, the image bounds (img_w / img_h; CurrentFrame's float bounds of vslam_fe_set_grid_bounds while
 * some are set) and gemm_float (forward / backward / mbf are not used); Ow = -Rcw^T tcw as the
 * function computes it (:2695); log_scale_factor = CurrentFrame.mfLogScaleFactor; orb_dist 1..255.  Per KeyFrame
 * keypoint i: kf_kps_host = pKF->mvKeysUn, mp_flags[i] & 1 iff vpMPs[i] && !isBad() && !sAlreadyFound.count(it),
 * world position, Get{Min,Max}DistanceInvariance(), descriptor.  cur_occupied_host marks CurrentFrame.mvpMapPoints
 * entries that are not NULL.  match_cur[i2] = i (pKF's keypoint whose MapPoint is written to mvpMapPoints[i2]) or -1. */
int vslam_search_by_projection_keyframe(vslam_fe* fe, const vslam_proj_params* p, const float* Ow, float log_scale_factor,
                                        int orb_dist, const vslam_kp* kf_kps_host, int n_kf, const uint8_t* mp_flags,
                                        const float* mp_x3dw, const float* mp_min_dist, const float* mp_max_dist,
                                        const uint8_t* mp_desc_host, const vslam_kp* dev_cur_kps,
                                        const uint8_t* dev_cur_desc, int n_cur, const uint8_t* cur_occupied_host,
                                        int32_t* match_cur, int* nmatches);

/* FMatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched,
 * int th, float ratioHamming) (fmatcher.cpp:750-863; proj_variant 0) and the overload that also fills vpMatchedKF from
 * vpPointsKFs (:865-981; it projects as fx*(x*(1/z))+cx, proj_variant 1) -- the loop-closing matchers.  p carries
 * Rcw | tcw (= sRcw/scw, Scw's translation/scw, :760-763) in Tcw, the camera, th, the image bounds (img_w / img_h; while
 * vslam_fe_set_grid_bounds has set some, pKF's integer copies of them, see there) and gemm_float;
 * Ow = -Rcw^T tcw; log_scale_factor = pKF->mfLogScaleFactor.  Per candidate MapPoint: flag (!isBad() &&
 * !spAlreadyFound.count(pMP)), world position, normal, Get{Min,Max}DistanceInvariance(), descriptor.
 * kf_matched_host[idx] != 0 iff vpMatched[idx] != NULL on entry.  match_kf[idx] = iMP (vpMatched[idx] = vpPoints[iMP],
 * vpMatchedKF[idx] = vpPointsKFs[iMP]) or -1 for the keypoints this call assigns; *nmatches as returned. */
int vslam_search_by_projection_sim3(vslam_fe* fe, const vslam_proj_params* p, const float* Ow, float log_scale_factor,
                                    float ratio_hamming, int proj_variant, const uint8_t* mp_flags, const float* mp_x3dw,
                                    const float* mp_normals, const float* mp_min_dist, const float* mp_max_dist,
                                    const uint8_t* mp_desc_host, int n_points, const vslam_kp* dev_kf_kps,
                                    const uint8_t* dev_kf_desc, int n_kf, const uint8_t* kf_matched_host,
                                    int32_t* match_kf, int* nmatches);

/* FMatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints)
 * (fmatcher.cpp:321-411; pinhole frames) -- the local-map matcher of Tracking::SearchLocalPoints.  Each MapPoint
 * arrives with what Frame::isInFrustum left in it (mappoint.h:73-81):
 *   flags bit0 = mbTrackInView && !isBad() && !(bFarPoints && mTrackDepth > thFarPoints), bit1 = Observations() > 0.
 * cur_occupied_host marks keypoints whose mvpMapPoints entry already holds a MapPoint with observations (the
 * matches of TrackWithMotionModel).  match_cur[idx] = index of the MapPoint written to F.mvpMapPoints[idx], or -1.
 * nnratio is FMatcher::mfNNratio (>= 0.4 on the device).  img_w / img_h are F's grid bounds {0, img_w, 0, img_h}; while
 * vslam_fe_set_grid_bounds has set some, the grid takes those and img_w / img_h are only validated. */
typedef struct vslam_mp_track {
    float proj_x, proj_y, proj_xr, view_cos; /* mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos */
    int32_t level;                           /* mnTrackScaleLevel */
    uint32_t flags;
} vslam_mp_track;
int vslam_search_by_projection_mappoints(vslam_fe* fe, const vslam_mp_track* mps_host, const uint8_t* mp_desc_host,
                                         int n_mp, const vslam_kp* dev_cur_kps, const uint8_t* dev_cur_desc,
                                         int n_cur, const float* cur_u_right_host, const uint8_t* cur_occupied_host,
                                         int img_w, int img_h, float th, float nnratio, int32_t* match_cur,
                                         int* nmatches);

/* Frame::isInFrustum(pMP, viewingCosLimit) (frame.cpp:529-595; the pinhole branch Nleft == -1) over a local map, and the
 * second loop of Tracking::SearchLocalPoints with the matcher behind it (tracking.cpp:3214-3263) in one enqueue: the caller
 * hands in the MapPoints as the map holds them, not the records above, and the list may be longer than the matcher's cap.
 * With a KB8 camera set (vslam_fe_set_kb8_camera, below) the projection is KannalaBrandt8::project; isInFrustumChecks
 * (two-camera fisheye rigs, Nleft != -1) is vslam_frame_in_frustum_rig for the records and vslam_search_local_points_rig for the
 * whole chain (below).
 *
 * Per MapPoint the arithmetic of vi_slam_amd/csrc/vslam_frustum.h: Matx algebra in float, both cv::norm in double,
 * Pinhole::project, the closed-interval bounds test over the context's float grid bounds (vslam_fe_set_grid_bounds) or
 * {0, img_w, 0, img_h}, the scale-invariance range, Matx::dot in float, MapPoint::PredictScale with glibc's logf.
 * Record of a point (vslam_mp_track): flags bit 0 = mbTrackInView, bit 1 = the input's bit 1.  A point that is not in view
 * has bit 0 clear, proj_x / proj_y = -1, or uv when the bounds test passed (frame.cpp:557-558), and ZERO in every other
 * field and in its depth -- the reference leaves the values of an earlier frame there.  A point whose input bit 0 is clear is
 * not tested (tracking.cpp:3221-3224) and gets proj -1.  0/0 projections (PcZ == 0 with x == 0 or y == 0) are NaN, pass the
 * reference's bounds test and reach an undefined float-to-int cast in the matcher: not modelled.  PredictScale divides
 * max_dist, as vslam_fuse_point's and the KeyFrame / Sim3 forms' do. */
typedef struct vslam_map_point {      /* 36 bytes */
    float pos[3], normal[3];          /* GetWorldPos2(), GetNormal2() */
    float min_dist, max_dist;         /* Get{Min,Max}DistanceInvariance() */
    uint32_t flags;                   /* bit0: candidate (mnLastFrameSeen != frame id && !isBad()); bit1: Observations() > 0 */
} vslam_map_point;
typedef struct vslam_frustum_params {
    float Tcw[12];                    /* rows [mRcwx | mtcwx] */
    float Ow[3];                      /* mOwx, as the Frame holds it */
    float fx, fy, cx, cy, mbf;
    float viewing_cos_limit;          /* 0.5 in SearchLocalPoints */
    float log_scale_factor;           /* Frame::mfLogScaleFactor */
    int32_t img_w, img_h;
    int32_t far_points; float th_far_points; /* mpLocalMapper->mbFarPoints, mThFarPoints */
} vslam_frustum_params;
#define VSLAM_LOCAL_POINTS_MAX 65536 /* MapPoints per call */
/* The frustum stage alone, for callers that want mmProjectPoints or the IncreaseVisible bookkeeping: track_out[i] / depth_out[i]
 * (mTrackDepth; may be NULL) for every point, *n_in_view = nToMatch.  n <= VSLAM_LOCAL_POINTS_MAX, VSLAM_ERR_UNSUPPORTED
 * above.  Blocking. */
int vslam_frame_in_frustum(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points_host, int n,
                           vslam_mp_track* track_out, float* depth_out, int* n_in_view);
/* upload -> k_frustum -> k_frustum_compact -> the matcher of vslam_search_by_projection_mappoints -> one result copy, all on
 * the context's stream without a host wait in between.  points / mp_desc (32 bytes per MapPoint) are host arrays
 * (points_where = VSLAM_IMGS_HOST) or DEVICE arrays (VSLAM_IMGS_DEVICE: a map that lives in HBM pays no upload; mp_desc
 * 16-byte aligned, both untouched until _wait returns).  The points that go on to the matcher are those in view and not
 * beyond th_far_points when far_points is set (fmatcher.cpp:333), in their original order; at most 4096 of them.
 * dev_cur_kps / dev_cur_desc / n_cur (<= 4096), cur_u_right_host, cur_occupied_host, th, nnratio (>= 0.4): as for
 * vslam_search_by_projection_mappoints.  n_mp == 0 or n_cur == 0: an empty result, nothing is launched.
 * _wait: match_cur[idx] = index INTO THE CALLER'S points ARRAY of the MapPoint written to F.mvpMapPoints[idx], or -1;
 * *nmatches as the reference counts it; *n_to_match = nToMatch (points in view, before the far test); *n_matched_against =
 * points handed to the matcher; track_out (may be NULL): the n_mp records.  More than 4096 points handed on:
 * VSLAM_ERR_UNSUPPORTED with match_cur all -1, *nmatches = 0 and the two counts delivered.  One search per context may be
 * in flight.  An empty search computed no records: asking _wait for track_out after an enqueue with n_cur == 0 and
 * n_mp > 0 is VSLAM_ERR_INVALID (vslam_frame_in_frustum gives the records without keypoints). */
int vslam_search_local_points_async(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points,
                                    const uint8_t* mp_desc, int n_mp, int points_where, const vslam_kp* dev_cur_kps,
                                    const uint8_t* dev_cur_desc, int n_cur, const float* cur_u_right_host,
                                    const uint8_t* cur_occupied_host, float th, float nnratio);
int vslam_search_local_points_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match,
                                   int* n_matched_against, vslam_mp_track* track_out);
/* _async + _wait */
int vslam_search_local_points(vslam_fe* fe, const vslam_frustum_params* p, const vslam_map_point* points,
                              const uint8_t* mp_desc, int n_mp, int points_where, const vslam_kp* dev_cur_kps,
                              const uint8_t* dev_cur_desc, int n_cur, const float* cur_u_right_host,
                              const uint8_t* cur_occupied_host, float th, float nnratio, int32_t* match_cur, int* nmatches,
                              int* n_to_match, int* n_matched_against, vslam_mp_track* track_out);

/* With vslam_fe_set_profiling on: HIP-event time of k_frustum and of k_frustum_compact alone, summed over the local-points
 * searches waited for since profiling was switched on.  Any pointer may be NULL. */
int vslam_fe_get_local_points_profile(vslam_fe* fe, double* frustum_ms, double* compact_ms, long* passes);

/* ---------------------------------------------------------------- fisheye cameras (Camera.type: "KannalaBrandt8")
 *
 * KannalaBrandt8::project / unproject (kannalabrandt8.cpp:11-27, :82-109) and the frustum test of a fisheye Frame, by the
 * arithmetic of vi_slam_amd/csrc/vslam_kb8.h: float operations rounded one by one and the host libm's atan2f, sqrtf, cosf,
 * sinf and tanf restated bit for bit (glibc 2.35; tanf for |x| < 3*pi/4, the quiet NaN beyond).
 *
 * With a KB8 camera set:
 *   - vslam_frame_in_frustum and vslam_search_local_points[_async/_wait] run Frame::isInFrustum (frame.cpp:529-595, Nleft == -1)
 *     with KannalaBrandt8::project in place of Pinhole::project; fx, fy, cx, cy of vslam_frustum_params must equal the camera's
 *     bit for bit (VSLAM_ERR_INVALID otherwise).  Compaction, matcher and _wait do not know the camera.
 *   - the entry points that project with intrinsics of their own -- vslam_search_by_projection_frame / _keyframe / _sim3,
 *     vslam_search_by_projection_dev_async, vslam_fuse_search, vslam_search_for_triangulation -- return VSLAM_ERR_UNSUPPORTED:
 *     they hold Pinhole::project and would silently project a fisheye frame as a pinhole.
 * A KB8 camera and a distorted pinhole camera (vslam_fe_set_camera with k1 != 0) exclude each other: the reference's fisheye
 * frames have zero mDistCoef.  Setting one while the other is set is VSLAM_ERR_INVALID.
 * The rig form of SearchByProjection(F, vpMapPoints), right-camera branch included (fmatcher.cpp:321-491), is
 * vslam_search_by_projection_mappoints_rig / vslam_search_local_points_rig below; the rig form of
 * SearchByProjection(CurrentFrame, LastFrame), right-camera branch :2593-2659 included, is vslam_search_by_projection_frame_rig.
 * Fuse(pKF, vpMapPoints, th, bRight) of a fisheye KeyFrame, both cameras of a rig, is vslam_fuse_search_rig.
 * Not covered: every other matcher's fisheye or right-camera branch (SearchForTriangulation; SearchBySim3 and SearchByProjection(pKF, Scw, vpPoints, vpPointsKFs, ..) project as a pinhole whatever the camera; SearchByBoW of a rig is vslam_search_by_bow_rig, the relocalisation and loop-closing SearchByProjection vslam_search_by_projection_keyframe_kb8 / _sim3_kb8), TriangulateMatches / epipolarConstrain / matchAndtriangulate (cv::SVD), ReconstructWithTwoViews
 * (cv::fisheye::undistortPoints), projectJac, tanf beyond 3*pi/4. */
typedef struct vslam_kb8_camera {
    float fx, fy, cx, cy; /* mvParameters[0..3] */
    float k[4];           /* mvParameters[4..7] */
    float precision;      /* the Newton loop's exit of unproject; <= 0: the reference default 1e-6f */
} vslam_kb8_camera;
/* NULL = pinhole (the default).  Waits for the context's stream.  Does not touch the extraction or its captured graph. */
int vslam_fe_set_kb8_camera(vslam_fe* fe, const vslam_kb8_camera* cam);
/* n points: xyz_host 3n floats -> uv_out 2n floats, and uv_host 2n floats -> xyz_out 3n floats (x * scale, y * scale, 1).
 * Blocking, evaluated on the device.  VSLAM_ERR_INVALID without a KB8 camera. */
int vslam_kb8_project(vslam_fe* fe, const float* xyz_host, int n, float* uv_out);
int vslam_kb8_unproject(vslam_fe* fe, const float* uv_host, int n, float* xyz_out);
/* The rays of a slot's keypoints (what CreateNewMapPoints' unprojectMat_ and MLPnPsolver's bearing vectors consume): one
 * launch on the context's stream behind whatever is enqueued there; reads the slot's device keypoints and its device count
 * (vslam_fe_slot_count_ptr), writes 3 floats per keypoint to dev_rays (DEVICE memory of 3 * vslam_fe_capacity floats, entries
 * beyond the count untouched).  No host wait. */
int vslam_kb8_unproject_slot_async(vslam_fe* fe, int slot, float* dev_rays);
/* Frame::isInFrustum for a two-fisheye rig (frame.cpp:596-606, Nleft != -1; isInFrustumChecks :1191-1271): the frustum records
 * alone (vslam_search_local_points_rig consumes them on the device).  The left camera is the context's KB8 camera (its intrinsics must equal p's), the right one rig->cam2; Tlr / Trl are
 * rows [R | t] of mTlrx / mTrlx.  Restated as written: tcw = mOwx in the right branch, mRx = Rrl * Rcw and mtx = Rrl * tcw + trl,
 * twcx = Rwc * tlr + tcw, no invz (p->mbf is not read).  track_left[i] / track_right[i]: proj_x / proj_y = the camera's uv
 * (mTrackProjX/Y, mTrackProjXR/YR), view_cos, level, flags bit 0 = mbTrackInView / mbTrackInViewR, bit 1 = the input's; proj_xr
 * is 0.  Where a camera does not see the point: level -1 (frame.cpp:599-600), flags bit 0 clear, zero elsewhere (the reference
 * leaves an earlier frame's values).  depth_left / depth_right (mTrackDepth / mTrackDepthR) may be NULL.  *n_in_view counts
 * left || right.  n <= VSLAM_LOCAL_POINTS_MAX.  Blocking. */
typedef struct vslam_kb8_rig {
    vslam_kb8_camera cam2;
    float Tlr[12], Trl[12];
} vslam_kb8_rig;
int vslam_frame_in_frustum_rig(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                               const vslam_map_point* points_host, int n, vslam_mp_track* track_left,
                               vslam_mp_track* track_right, float* depth_left, float* depth_right, int* n_in_view);

/* SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) and Tracking::SearchLocalPoints for a two-fisheye rig
 * (fmatcher.cpp:321-491 with Nleft != -1; tracking.cpp:3214-3263).  F.mvpMapPoints has n_left + n_right slots: [0, n_left) the
 * left keypoints, [n_left, n_left + n_right) the right ones.  Restated as written:
 *   - the left branch (window r * scale[level] with r times th, levels [level - 1, level], NO mvuRight gate in a rig) writes
 *     its best keypoint's slot and, where mvLeftToRightMatch names one, the right slot L2R + n_left without looking at it
 *   - a left ratio failure is a `continue`: the right branch of that point is skipped (:403-404)
 *   - the right branch (r NOT times th, :425; a record with level -1 takes none, :424) writes R2L unchecked, then its own slot
 *   - a slot is occupied iff its last writer has Observations() > 0, so a cross-write by a point without observations frees it
 *   - nmatches counts writes, not slots.
 * Records: flags bit 0 = mbTrackInView / mbTrackInViewR with the far test and isBad folded in, bit 1 = Observations() > 0 (one
 * MapPoint: the bit of either record counts).  n_left, n_right <= 4096 each (0 is an ordinary input), n_mp <= 4096, nnratio >=
 * 0.4 (VSLAM_ERR_UNSUPPORTED beyond).  An L2R / R2L entry outside [-1, n_other) is VSLAM_ERR_INVALID, checked before anything is
 * enqueued.  Both grids use the context's float grid bounds, or {0, img_w, 0, img_h}.  The matcher does not project, so it
 * runs with or without a KB8 camera set. */
typedef struct vslam_rig_frame {
    const vslam_kp* dev_kps_left;  const uint8_t* dev_desc_left;  int n_left;   /* keypoints_, descriptor rows [0, Nleft)      */
    const vslam_kp* dev_kps_right; const uint8_t* dev_desc_right; int n_right;  /* keypointsRight_, rows [Nleft, Nleft+Nright) */
    const int32_t* left_to_right_host;   /* mvLeftToRightMatch: n_left entries, -1 or an index < n_right   */
    const int32_t* right_to_left_host;   /* mvRightToLeftMatch: n_right entries, -1 or an index < n_left   */
    const uint8_t* occupied_host;        /* n_left + n_right, may be NULL */
} vslam_rig_frame;
/* The matcher alone, from caller-made records (the sibling of vslam_search_by_projection_mappoints): match_cur has n_left +
 * n_right entries, each the index of the last MapPoint written to the slot or -1.  Blocking. */
int vslam_search_by_projection_mappoints_rig(vslam_fe* fe, const vslam_mp_track* track_left_host,
                                             const vslam_mp_track* track_right_host, const uint8_t* mp_desc_host, int n_mp,
                                             const vslam_rig_frame* frame, int img_w, int img_h, float th, float nnratio,
                                             int32_t* match_cur, int* nmatches);
/* upload -> k_frustum_rig -> k_rig_keep / k_rig_compact -> k_sbp_rank (two jobs) -> k_rig_resolve -> one result copy, on the
 * context's stream without a host wait in between.  p, rig: as for vslam_frame_in_frustum_rig (a KB8 camera must be set and
 * its intrinsics equal p's: VSLAM_ERR_INVALID otherwise).  points / mp_desc / points_where: as for
 * vslam_search_local_points_async.  A point goes on to the matcher when left OR right sees it and it is not far, in original
 * order, at most 4096.  The far test (fmatcher.cpp:333) reads mTrackDepth, the left depth, as vslam_frame_in_frustum_rig delivers
 * it: 0 where the left camera does not see the point (the reference reads an earlier frame's value there), so a right-only
 * point is never far.
 * _wait: match_cur (n_left + n_right entries) indexes the caller's points array; *n_to_match counts left || right before the
 * far test (tracking.cpp:3226-3230); *n_matched_against = points handed on; track_left / track_right (may be NULL): the n_mp
 * records, identical to vslam_frame_in_frustum_rig's.  More than 4096 points handed on: VSLAM_ERR_UNSUPPORTED with match_cur all
 * -1, *nmatches = 0 and the two counts delivered.  One local-points search (rig or not) per context may be in flight.  n_mp == 0
 * or n_left + n_right == 0: an empty result, nothing is launched (and no records: asking for them then is VSLAM_ERR_INVALID). */
int vslam_search_local_points_rig_async(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                        const vslam_map_point* points, const uint8_t* mp_desc, int n_mp, int points_where,
                                        const vslam_rig_frame* frame, float th, float nnratio);
int vslam_search_local_points_rig_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches, int* n_to_match,
                                       int* n_matched_against, vslam_mp_track* track_left, vslam_mp_track* track_right);
/* _async + _wait */
int vslam_search_local_points_rig(vslam_fe* fe, const vslam_frustum_params* p, const vslam_kb8_rig* rig,
                                  const vslam_map_point* points, const uint8_t* mp_desc, int n_mp, int points_where,
                                  const vslam_rig_frame* frame, float th, float nnratio, int32_t* match_cur, int* nmatches,
                                  int* n_to_match, int* n_matched_against, vslam_mp_track* track_left,
                                  vslam_mp_track* track_right);
/* With vslam_fe_set_profiling on: HIP-event time of the two-job k_sbp_rank launch and of k_rig_resolve alone, summed over the
 * rig searches waited for since profiling was switched on.  Any pointer may be NULL. */
int vslam_fe_get_local_points_rig_profile(vslam_fe* fe, double* rank_ms, double* resolve_ms, long* passes);

/* FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) for a two-fisheye rig
 * (fmatcher.cpp:2494-2684 with CurrentFrame.Nleft != -1; TrackWithMotionModel, tracking.cpp:2728 / :2736).  Restated as written:
 *   - queries are the n_last = Nleft + Nright entries of the last frame: last_kps_host is ONE array, keypoints_ followed by
 *     keypointsRight_ (octave and angle are read); a MapPoint in a left and a right slot is two independent queries
 *   - the left branch: Rcw * x3Dw + tcw as one gemm, invzc < 0 and uv outside the closed grid bounds are `continue`s,
 *     KannalaBrandt8::project, radius th * scale[octave], the forward / backward / +-1 level rule, an EMPTY WINDOW IS A `continue`
 *     (:2534-2535), no mvuRight gate, best distance <= TH_HIGH writes slot bestIdx2
 *   - the three left `continue`s skip the right branch of the query; a left window whose candidates are all occupied does not
 *   - the right branch (:2593-2658): x3Dr = Rrl * x3Dc + trl as one gemm (gemm_float as for Tcw), projected through the LEFT
 *     camera's model (mpCamera, not mpCamera2), with no depth test, no in-frame test and no empty-window `continue`; window over
 *     the right keypoints, same radius and level rule; reads and writes slot i2 + n_left
 *   - a slot is occupied iff it holds a MapPoint with Observations() > 0: a match by a point without observations leaves the
 *     slot free, a later query may overwrite it (the last writer stays, both are counted and both enter the histogram)
 *   - ONE rotation histogram over left and right entries; every entry of a rejected bin clears its slot and decrements nmatches
 *   - mvLeftToRightMatch / mvRightToLeftMatch are not read: there are no cross-writes.
 * p: as for vslam_search_by_projection_frame; a KB8 camera must be set and p->fx, fy, cx, cy equal it bit for bit
 * (VSLAM_ERR_INVALID otherwise); p->mbf is not read.  rig: only Trl is read.  cur: the keypoints, descriptors, counts and
 * occupied_host (n_left + n_right, may be NULL) are read, the match maps may be NULL.  last_flags, last_x3dw, mp_desc_host: as for
 * the pinhole form.  match_cur[slot] (n_left + n_right entries) = the index i of the last-frame entry that ends in the slot, or
 * -1; *nmatches as the reference counts it.  n_last <= 4096 (both cameras together), n_left, n_right <= 4096 each:
 * VSLAM_ERR_UNSUPPORTED beyond, nothing enqueued.  n_last == 0 or n_left + n_right == 0: an empty result, nothing is launched.
 * _async: upload -> k_sbp_rank_rig (two jobs) -> k_sbp_rig_resolve -> k_sbp_rig_replay -> one result copy on the context's
 * stream, no host wait in between; one such search per context may be in flight (a second _async is VSLAM_ERR_INVALID).
 * vslam_search_by_projection_frame keeps refusing while a KB8 camera is set. */
int vslam_search_by_projection_frame_rig_async(vslam_fe* fe, const vslam_proj_params* p, const vslam_kb8_rig* rig,
                                               const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                               const float* last_x3dw, const uint8_t* mp_desc_host, const vslam_rig_frame* cur);
int vslam_search_by_projection_frame_rig_wait(vslam_fe* fe, int32_t* match_cur, int* nmatches);
/* _async + _wait */
int vslam_search_by_projection_frame_rig(vslam_fe* fe, const vslam_proj_params* p, const vslam_kb8_rig* rig,
                                         const vslam_kp* last_kps_host, int n_last, const uint8_t* last_flags,
                                         const float* last_x3dw, const uint8_t* mp_desc_host, const vslam_rig_frame* cur,
                                         int32_t* match_cur, int* nmatches);
/* With vslam_fe_set_profiling on: HIP-event time of the two-job k_sbp_rank_rig launch and of the resolution behind it
 * (k_sbp_rig_resolve + k_sbp_rig_replay), summed over the rig frame searches waited for since.  Any pointer may be NULL. */
int vslam_fe_get_frame_rig_profile(vslam_fe* fe, double* rank_ms, double* resolve_ms, long* passes);

/* Device-resident, batched form of the same matcher: every pointer of a job is a DEVICE pointer; counts are
 * int32 in HBM (vslam_fe_slot_count_ptr); keypoint arrays hold up to the context's capacity (<= 4096).  Up to 16
 * jobs per call run in one pass of the two kernels on fe's stream.  _async returns without waiting; _wait
 * delivers n_cur[j] entries of match_cur[j] and nmatches[j]. */
typedef struct vslam_sbp_job {
    vslam_proj_params p;
    const vslam_kp* dev_last_kps;
    const int32_t* dev_n_last;
    const uint8_t* dev_last_flags;
    const float* dev_last_x3dw;
    const uint8_t* dev_mp_desc;
    const vslam_kp* dev_cur_kps;
    const uint8_t* dev_cur_desc;
    const int32_t* dev_n_cur;
    const float* dev_cur_u_right;    /* may be NULL */
    const uint8_t* dev_cur_occupied; /* may be NULL */
} vslam_sbp_job;
int vslam_search_by_projection_dev_async(vslam_fe* fe, int njobs, const vslam_sbp_job* jobs);
int vslam_search_by_projection_dev_wait(vslam_fe* fe, const int* n_cur, int32_t* const* match_cur, int* nmatches);

/* Frame::UnprojectStereo (frame.cpp:1023-1037) on the device for all left keypoints of the stereo pairs of fe's
 * last vslam_frame_stereo_batch_async / vslam_stereo_match_batch: the stereo points that UpdateLastFrame
 * (tracking.cpp) turns into MapPoints for the next frame's SearchByProjection.  Twc: npairs x 12 floats, rows
 * [mRwc | mOw] per pair.  flags[i] = 0 (no depth) or 1 | (observations ? 2 : 0).  Enqueued on fe's stream;
 * vslam_stereo_points_buffers returns the per-pair device arrays (stable for the life of the context). */
int vslam_stereo_points_dev_async(vslam_fe* fe, int npairs, const float* Twc, float cx, float cy, float invfx,
                                  float invfy, int observations, int gemm_float);
int vslam_stereo_points_buffers(vslam_fe* fe, int pair, const float** dev_x3dw, const uint8_t** dev_flags,
                                const float** dev_u_right, const float** dev_depth);

/* MapPoint::ComputeDistinctiveDescriptors (mappoint.cpp:322-390) for nsets MapPoints in one pass: set s owns the
 * descriptors desc_host[offsets[s] .. offsets[s+1]) (32 bytes each, its observations in the reference's iteration
 * order); best[s] = index inside the set of the descriptor with the least median distance to the others
 * (median = sorted[int(0.5*(N-1))], first wins), -1 for an empty set.  At most 2048 descriptors per set. */
int vslam_distinctive_descriptors(vslam_fe* fe, const uint8_t* desc_host, const int32_t* offsets, int nsets,
                                  int32_t* best);

/* Frame::ComputeBoW (frame.cpp:455-461) = DBoW3::Vocabulary::transform(features, BowVector&, FeatureVector&,
 * levelsup) (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp:754-878).
 * vslam_voc_create uploads a flat copy of DBoW3's m_nodes: node i has the children child_ids[child_start[i] ..
 * + child_count[i]) in their stored order (it decides ties), a 32-byte descriptor, and for leaves a word id and a
 * weight; depth_levels = m_L; weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; norm (the scoring object's
 * mustNormalize): 0 none, 1 L1, 2 L2.  Node ids must be larger than their parent's (DBoW3's creation order).
 * vslam_bow_transform walks the tree for n device-resident descriptors and returns per feature the word id, the
 * word weight and the node id at level depth_levels - levelsup; the _slots forms do the same for image slots of the
 * context (counts stay in HBM) in one launch.  vslam_bow_assemble (pure host) turns those into the BowVector
 * (ascending word ids / values) and the FeatureVector (ascending node ids, fv_off[n_fv+1] offsets into fv_feat)
 * exactly as DBoW3 does (std::map accumulation in feature order, double arithmetic); arrays hold n entries
 * (fv_off: n + 1). */
typedef struct vslam_voc vslam_voc;
int vslam_voc_create(int device, int depth_levels, int weighting, int norm, int n_nodes, const int32_t* child_start,
                     const int32_t* child_count, const int32_t* child_ids, int n_child_ids, const uint8_t* node_desc,
                     const double* node_weight, const int32_t* node_word_id, vslam_voc** out);
void vslam_voc_destroy(vslam_voc* voc);
/* DBoW3::Vocabulary::load(const std::string&) (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp:1084-1112), the call
 * core::System makes at start-up (src/core/system.cpp:76).  vslam_voc_load reads the file and uploads it; the
 * vslam_voc_file_* functions are its host half (no GPU needed): open parses, info / arrays expose the flat node table
 * in vslam_voc_create's layout (pointers stay valid until close).  Formats, tried in the reference's order: DBoW3's
 * binary stream (magic 88877711233; format 1 plain, 2 in QuickLZ level-1 chunks -- what Vocabulary::save writes by
 * default under any file name), then the text form for names containing ".txt" (format 3; weights keep float
 * precision as in load_fromtxt, :1372-1446).  cv::FileStorage YAML/XML vocabularies and descriptors other than
 * 1 x 32 CV_8U return VSLAM_ERR_UNSUPPORTED; a damaged file returns VSLAM_ERR_INVALID (every read is bounds-checked).
 * scoring is DBoW3's ScoringType (0 L1_NORM .. 5 DOT_PRODUCT); norm is what its scoring object's mustNormalize says,
 * in vslam_voc_create's encoding.  vslam_voc_file_last_error: message of the last failed vslam_voc_file_* call of
 * this thread (vslam_voc_load copies it into vslam_last_error). */
typedef struct vslam_voc_file vslam_voc_file;
int vslam_voc_file_open(const char* path, vslam_voc_file** out);
void vslam_voc_file_close(vslam_voc_file* f);
int vslam_voc_file_info(const vslam_voc_file* f, int* branching, int* depth_levels, int* scoring, int* weighting,
                        int* norm, int* n_nodes, int* n_words, int* n_child_ids, int* format);
int vslam_voc_file_arrays(const vslam_voc_file* f, const int32_t** child_start, const int32_t** child_count,
                          const int32_t** child_ids, const uint8_t** node_desc, const double** node_weight,
                          const int32_t** node_word_id);
const char* vslam_voc_file_last_error(void);
int vslam_voc_load(int device, const char* path, vslam_voc** out);
/* test hook of the reader: decode one QuickLZ 1.5 level-1 packet (header + payload) of at most n bytes into dst;
 * returns the decoded size and the packet's size in *used, -1 for a damaged packet or a short dst. */
long vslam_dbg_qlz_decode(const uint8_t* packet, size_t n, uint8_t* dst, size_t cap, size_t* used);
int vslam_voc_info(const vslam_voc* voc, int* depth_levels, int* weighting, int* norm, int* n_nodes);
int vslam_bow_transform(vslam_fe* fe, const vslam_voc* voc, const uint8_t* dev_desc, int n, int levelsup,
                        int32_t* word_id, double* weight, int32_t* node_id);
int vslam_bow_transform_slots_async(vslam_fe* fe, const vslam_voc* voc, int first_slot, int nslots, int levelsup);
int vslam_bow_transform_slots_wait(vslam_fe* fe, const int* n, int32_t* const* word_id, double* const* weight,
                                   int32_t* const* node_id);
int vslam_bow_assemble(int weighting, int norm, const int32_t* word_id, const double* weight, const int32_t* node_id,
                       int n, int32_t* bow_ids, double* bow_vals, int* n_bow, int32_t* fv_nodes, int32_t* fv_off,
                       int32_t* fv_feat, int* n_fv);

/* ---------------------------------------------------------------- Vocabulary::create / save (training a vocabulary)
 *
 * DBoW3::Vocabulary::create(training_features, k, L, weighting, scoring) (thirdparty/DBoW3/DBoW3/src/Vocabulary.cpp:
 * 157-571; tools/createVoc/createVoc.cpp:53-57 is its caller): hierarchical k-means over 32-byte binary descriptors
 * -- k-means++ seeding (initiateClustersKMpp, :409-491), Lloyd passes with the bitwise majority of DescManip::meanValue
 * (DescManip.cpp:25-73) until the association repeats, strict `<` so that the lowest cluster wins a tie, children in
 * cluster order, word ids in node-id order, weights log(NDocs / Ni) over the training documents -- and
 * Vocabulary::save (:1066-1079).  Everything is integer arithmetic or a libm double, so the device, the host twin
 * (vslamh_voc_train in libvslam_host.so) and the tests' numpy restatement agree bit for bit.
 *
 * ONE deviation from the reference: it draws from the process-global rand() in depth-first order, which would serialise
 * the tree.  Here a draw is a pure function of (seed, path from the root, draw counter of the node), the functions
 * below; every use is the reference's own expression with vslamvoc_draw in place of rand():
 *   first centre of a node with n features      vslamvoc_draw(key, 0, mask) % n
 *   cut_d = (double(r) / double(RAND_MAX)) * dist_sum, RAND_MAX = 2147483647, each operation rounded on its own,
 *           redrawn while r == 0 (cut_d == 0.0); after 64 zero draws in a row r = 1 (unreachable with the default mask).
 * j counts the draws of the node, redraws included. */
#if defined(__HIPCC__)
#define VSLAM_VOC_HD __host__ __device__
#else
#define VSLAM_VOC_HD
#endif
static inline VSLAM_VOC_HD uint64_t vslamvoc_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
/* key of the root: vslamvoc_mix(seed); key of child c (cluster index) of a node with key `parent` */
static inline VSLAM_VOC_HD uint64_t vslamvoc_child_key(uint64_t parent, int c) {
    return vslamvoc_mix(parent ^ ((uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull));
}
/* 31 bits in place of rand() */
static inline VSLAM_VOC_HD uint32_t vslamvoc_draw(uint64_t key, uint32_t j, uint32_t rand_mask) {
    return (uint32_t)(vslamvoc_mix(key ^ (((uint64_t)j + 1) * 0xD1B54A32D192ED03ull)) >> 33) & rand_mask;
}

#define VSLAM_VOC_MAX_FEATURES (1 << 24)
typedef struct vslam_voc_train_params {
    int32_t k;          /* branching factor, 2..64 (the reference tool uses 35) */
    int32_t L;          /* depth levels, 1..10 */
    int32_t weighting;  /* 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
    int32_t scoring;    /* 0 L1_NORM .. 5 DOT_PRODUCT; only stored in the file */
    uint64_t seed;
    uint32_t rand_mask; /* 0x7fffffff; a smaller mask is a diagnostic (mask 3: a quarter of the draws are zero).  0 is invalid */
    int32_t max_iter;   /* bound on the Lloyd passes of one node (assign passes, the first included); 0 = 10000.  Not in the
                           reference: a node that reaches it keeps the state of its last pass and is counted in the stats */
} vslam_voc_train_params;
typedef struct vslam_voc_train_stats {
    int32_t nodes, words, deepest_level; /* nodes includes the root */
    int32_t max_passes;                  /* Lloyd passes: most of any node, and the sum over the k-means nodes */
    int64_t total_passes;
    int32_t hit_max_iter;                /* nodes stopped by max_iter */
    int32_t early_stops;                 /* seedings that ended with fewer than k centres (dist_sum == 0) */
    int64_t draws, redraws;              /* vslamvoc_draw calls; those of them that were zero under cut_d */
    int32_t small_nodes;                 /* HKmeansStep calls with n <= k: one cluster per feature */
    int32_t single_leaves;               /* children with one feature above level L: leaves, no recursion */
    int64_t empty_groups;               /* meanValue calls on an empty group (the centre stays) */
    float ms_seed, ms_assign, ms_mean, ms_partition, ms_weights, ms_total; /* HIP events; the host twin fills ms_total */
} vslam_voc_train_stats;
/* desc: n_features x 32 bytes, n_features = doc_offsets[n_docs] in 1..VSLAM_VOC_MAX_FEATURES, in host memory
 * (desc_location VSLAM_IMGS_HOST) or in HBM of `device` (VSLAM_IMGS_DEVICE); document d owns the rows doc_offsets[d] ..
 * doc_offsets[d+1]) (n_docs + 1 non-decreasing entries from 0; empty documents are allowed).  *out is an in-memory
 * vslam_voc_file (format 0) for vslam_voc_file_info / _arrays / _save / _upload / _close: the flat table in
 * vslam_voc_create's layout and in DBoW3's node order (a HKmeansStep call numbers its children consecutively, then
 * descends into them in turn).  stats may be NULL.  Bad parameters or offsets return VSLAM_ERR_INVALID before anything
 * is launched.  The call is synchronous and runs on a stream of its own: a device block must be complete before it.
 * vslamh_voc_train (libvslam_host.so only) is the same on one CPU core: tests, demo, timing baseline --
 * not a fallback. */
int vslam_voc_train(int device, const vslam_voc_train_params* params, const uint8_t* desc, int desc_location,
                    const int64_t* doc_offsets, int n_docs, vslam_voc_file** out, vslam_voc_train_stats* stats);
int vslamh_voc_train(const vslam_voc_train_params* params, const uint8_t* desc, const int64_t* doc_offsets, int n_docs,
                     vslam_voc_file** out, vslam_voc_train_stats* stats);
/* Vocabulary::save(filename) for a name without ".yml": the plain binary stream (toStream(out, false), :1292-1366), which
 * Vocabulary::load and vslam_voc_load read under any name.  Works for trained and for loaded files (tools/convertVoc). */
int vslam_voc_file_save(const vslam_voc_file* f, const char* path);
/* an in-memory file (format 0) from a flat node table in vslam_voc_create's layout, with the same checks; n_words is
 * the number of leaves.  For callers that hold the arrays and want _save or _upload. */
int vslam_voc_file_from_arrays(int branching, int depth_levels, int scoring, int weighting, int n_nodes,
                               const int32_t* child_start, const int32_t* child_count, const int32_t* child_ids,
                               int n_child_ids, const uint8_t* node_desc, const double* node_weight,
                               const int32_t* node_word_id, vslam_voc_file** out);
/* the upload half of vslam_voc_load */
int vslam_voc_file_upload(int device, const vslam_voc_file* f, vslam_voc** out);

/* ---------------------------------------------------------------- KeyFrameDatabase (relocalisation / loop candidates)
 *
 * KeyFrameDatabase (src/datastructures/keyframedatabase.cpp) between Frame::ComputeBoW and SearchByBoW: the keyframes'
 * BowVectors live in HBM, and one kernel computes for every (query, keyframe) pair what the reference's walk over its
 * inverted file and DBoW3's L1Scoring::score (thirdparty/DBoW3/DBoW3/src/ScoringObject.cpp:23-68) compute: the number
 * of common words, the smallest common word and the score, whose terms are added in ascending word order into one
 * double exactly as the reference adds them.  Keyframes and maps are named by ids (KeyFrame::mnId, Map::GetId()).
 *
 * scoring is DBoW3's ScoringType as vslam_voc_file_info reports it; only 0 (L1_NORM) is implemented, anything else
 * returns VSLAM_ERR_UNSUPPORTED.  The pool holds 4096 (id, value) entries at first (vslam_kfdb_create_ex: the number
 * given, 0 = that default), doubles when an add does not fit, and is compacted -- the erased keyframes' entries and
 * slots dropped, the order of the rest kept -- whenever the erased entries exceed half of those handed out.
 *
 * add (keyframedatabase.cpp:21-27): bow_ids / bow_vals are a BowVector as vslam_bow_assemble produces it: n strictly
 * ascending word ids in [0, n_words) and their values.  n = 0 is legal; such a keyframe is never found.  A kf_id that
 * is in the database, ids out of order or out of range return VSLAM_ERR_INVALID and change nothing.  A keyframe's
 * place in `add` order is its place in every inverted list of the reference (push_back); an id erased and added again
 * goes last.  erase (:29-48; an unknown id is not an error, as there), clear (:50-54), clear_map (:56-80).
 * size: live keyframes and their entries.  stats: pool capacity and entries handed out, slots (live and erased, not
 * compacted away yet), and how often the pool grew / was compacted.  All of these wait for a query still in flight.
 * A database is not re-entrant across queries: one query (of up to 32 BowVectors) is in flight or delivered at a time.
 *
 * query_async: nq (1..32) host BowVectors, staged through pinned memory of `fe` and enqueued on its stream.  query_wait
 * delivers query q of the last query_async on (db, fe) -- any number of times, in any order, until the next
 * query_async -- as the hit list: every live keyframe sharing at least one word, in the order in which the reference's
 * walk over the query's words first meets it (smallest common word, then add order), i.e. lKFsSharingWords before any
 * exclusion; per hit the keyframe's id and map, words = mnRelocWords / mnPlaceRecognitionWords, score =
 * L1Scoring::score(query, keyframe) and si = (float)score.  Any output array may be NULL; *n_hits is always set, and
 * VSLAM_ERR_CAPACITY returned when it exceeds cap (nothing is written then).  `fe` must outlive the wait.  The hit
 * list is ordered and compacted on the host from a dense per-slot result. */
typedef struct vslam_kfdb vslam_kfdb;
int vslam_kfdb_create(int device, int n_words, int scoring, vslam_kfdb** out);
int vslam_kfdb_create_ex(int device, int n_words, int scoring, int initial_entries, vslam_kfdb** out);
void vslam_kfdb_destroy(vslam_kfdb* db);
int vslam_kfdb_add(vslam_kfdb* db, int64_t kf_id, int32_t map_id, const int32_t* bow_ids, const double* bow_vals, int n);
int vslam_kfdb_erase(vslam_kfdb* db, int64_t kf_id);
int vslam_kfdb_clear(vslam_kfdb* db);
int vslam_kfdb_clear_map(vslam_kfdb* db, int32_t map_id);
int vslam_kfdb_size(vslam_kfdb* db, int* n_keyframes, long long* n_entries);
int vslam_kfdb_stats(vslam_kfdb* db, long long* capacity, long long* used, int* n_slots, int* n_growths,
                     int* n_compactions);
int vslam_kfdb_query_async(vslam_kfdb* db, vslam_fe* fe, int nq, const int32_t* const* bow_ids,
                           const double* const* bow_vals, const int* n);
int vslam_kfdb_query_wait(vslam_kfdb* db, vslam_fe* fe, int q, int cap, int64_t* hit_kf, int32_t* hit_map,
                          int32_t* hit_words, float* hit_si, double* hit_score, int* n_hits);

/* The selection stage: KeyFrameDatabase::DetectRelocalizationCandidates (keyframedatabase.cpp:707-811) and
 * DetectNBestCandidates (:579-705) from the hit list on.  Pure host code without a database handle (libvslam_host.so
 * has them too); they return 0, -1 for invalid arguments or -4 when `cap` is too small (*n_out = the number needed).
 *   hits          hit_kf / hit_map / hit_words / hit_si of vslam_kfdb_query_wait, in its order
 *   score_io      n_hits floats: what the reference keeps in the KeyFrames (mRelocScore / mPlaceRecognitionScore).  In:
 *                 the caller's last value for each hit; out: replaced by si for the hits this query scored (words >
 *                 minCommonWords = (int)(maxCommonWords * 0.8f)).  The covisibility step reads it for neighbours that
 *                 were not scored, as the reference reads the stale member.
 *   neighbours_fn pKFi->GetBestCovisibilityKeyFrames(10): writes at most 10 ids, returns how many.  A neighbour that
 *                 is not a (non-excluded) hit is skipped, as the query stamp does in the reference.  NULL: no neighbours.
 *   relocalization: out_kf = vpRelocCandidates -- accScore > 0.75f * bestAccScore, pBestKF in map_id, first occurrence.
 *   nbest         connected_ids = pKF->GetConnectedKeyFrames(): such hits are neither listed nor seen by the
 *                 neighbour step (:597-606).  n_candidates = nNumCandidates (3 at loopclosing.cpp:415); loop_kf and
 *                 merge_kf hold n_candidates ids each; bad_maps = ids of maps with IsBad().  The fill loop is :684-704:
 *                 a keyframe enters spAlreadyAddedKF even when neither vector took it.
 * Deviations from the reference: mRelocScore is uninitialised in its constructors (keyframe.cpp:20-38) -- callers start
 * score_io at 0.0f, as mPlaceRecognitionScore starts; every query counts as carrying a fresh query id (the reference's
 * callers guarantee it; the mn*Query(0) collision of a query with id 0 is not modelled); DetectNBestCandidates never
 * ends on a bad keyframe (:687-688 `continue` without advancing) -- SetBadFlag erases bad keyframes from the database
 * (keyframe.cpp:634), so PRECONDITION: no hit is a bad keyframe, and there is no bad flag to pass. */
typedef int (*vslam_kfdb_neighbours_fn)(void* user, int64_t kf_id, int64_t* out_ids /* [10] */);
int vslam_kfdb_select_relocalization(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words,
                                     const float* hit_si, int n_hits, float* score_io, int32_t map_id,
                                     vslam_kfdb_neighbours_fn neighbours_fn, void* user, int64_t* out_kf, int cap,
                                     int* n_out);
int vslam_kfdb_select_nbest(const int64_t* hit_kf, const int32_t* hit_map, const int32_t* hit_words, const float* hit_si,
                            int n_hits, float* score_io, int32_t query_map_id, const int64_t* connected_ids,
                            int n_connected, int n_candidates, const int32_t* bad_maps, int n_bad_maps,
                            vslam_kfdb_neighbours_fn neighbours_fn, void* user, int64_t* loop_kf, int* n_loop,
                            int64_t* merge_kf, int* n_merge);

/* ---------------------------------------------------------------- Covisibility (the observation graph and its counts)
 *
 * A mirror of MapPoint::mObservations / nObs / mbBad and of the keyframes' id, map and mbBad in HBM, with a host shadow.
 * The caller calls the mirror's twin wherever the reference calls the original; the mutators change the shadow only
 * (after waiting for a query of this mirror that is still in flight), and a query uploads what changed on the
 * context's stream before its kernels.  Keyframes, MapPoints and maps are ids (KeyFrame::mnId, MapPoint::id_,
 * Map::GetId()).  Unknown ids, duplicate adds and out-of-range arguments return VSLAM_ERR_INVALID and change nothing;
 * an id that was erased may be added again.
 *
 * order_key stands for the KeyFrame* value: every std::map<KeyFrame*, ..> and every sort of pair<int, KeyFrame*> of the
 * reference orders by pointer, so the key is an input; (uintptr_t)pKF reproduces the reference's orders.  Keys are
 * unique among the live keyframes.
 *
 *   add_keyframe / add_keyframes          one keyframe / n keyframes (all or none)
 *   set_keyframe_bad                      mbBad as isBad() reads it, nothing else
 *   set_keyframe_map                      KeyFrame::UpdateMap
 *   erase_keyframe                        forgets the slot; VSLAM_ERR_INVALID while a MapPoint still observes it
 *   add_point                             a MapPoint without observations, nObs = 0, not bad
 *   add_observation (mappoint.cpp:137-162)  sets the left (is_right = 0) or right index of the keyframe's entry and that
 *                                         side's level (keypoint octave, 0..63); nObs += stereo ? 2 : 1 -- stereo is the
 *                                         caller's `!pKF->mpCamera2 && mvuRight[idx] >= 0`, kept with the left side.  A
 *                                         second call for a side overwrites it and increments nObs again, as there
 *   erase_observation (:164-197)          no entry: nothing happens.  nObs goes down per side as stored, the entry is
 *                                         dropped, and with nObs <= 2 the point becomes bad and loses every observation
 *                                         (:211-220); *became_bad (may be NULL) says so
 *   clear_point                           the first block of SetBadFlag and of Replace: bad, observations cleared; nObs
 *                                         stays as it is, as there
 *   erase_point                           forgets the MapPoint
 *   clear_map                             forgets the keyframes of the map and every MapPoint that one of them observes
 *   clear                                 forgets everything
 *   size                                  live keyframes, live points, observation entries
 *   stats                                 pool capacity and records handed out, growths, compactions
 *   get_point                             nObs, bad flag and the entries in ascending order_key; *n_records is always
 *                                         set, VSLAM_ERR_CAPACITY when it exceeds cap (nothing is written then)
 *
 * The pool holds 4096 observation records at first (initial_entries, 0 = that default).  A point's records lie in one
 * segment of 4, 8, 16, .. records; a full segment moves to one of twice the size at the pool's end, a full pool doubles,
 * and the pool is compacted when abandoned segments exceed half of what was handed out.
 *
 * Queries: up to VSLAM_COVIS_MAX_JOBS jobs per enqueue, one query per mirror in flight (a second _async returns
 * VSLAM_ERR_INVALID); results stay readable until the next enqueue on the mirror.  mp_ids is mvpMapPoints, index
 * aligned, -1 for NULL, at most VSLAM_COVIS_MAX_LIST entries; an id listed twice counts twice; a point that is bad in
 * the mirror is skipped.  result.error: bit 0 an mp_id the mirror does not know, bit 1 an unknown self_kf / kf_id
 * (CONNECTIONS and culling); the job's other outputs are zero then.
 *
 * connections, mode VSLAM_COVIS_CONNECTIONS = KeyFrame::UpdateConnections (keyframe.cpp:363-427): the counter runs over
 * every observer except self_kf, bad keyframes and keyframes of a map other than map_id.  n_counter entries (kf, count)
 * in ascending order_key = mConnectedKeyFrameWeights; kf_max / n_max by `>` along that order (:402); n_ordered entries
 * = mvpOrderedConnectedKeyFrames / mvOrderedWeights: those with count >= 15, or the single (n_max, kf_max), in
 * descending (count, order_key).  n_counter = 0: the caller returns as :385.
 * Mode VSLAM_COVIS_VOTE = Tracking::UpdateLocalKeyFrames (tracking.cpp:3309-3376): every observer counts; delivered
 * are the keyframes that are not bad, in ascending order_key, and kf_max among them; n_ordered = 0.
 * Both: n_tracked = KeyFrame::TrackedMapPoints(min_obs) (:320-339) over the list.
 * connections_lists copies the lists of job j of the query delivered last; any pointer may be NULL.
 *
 * culling = LocalMapping::KeyFrameCulling (localmapping.cpp:990-1052): mp_ids[i] = -1 for NULL and for a point the depth
 * gate :1003-1007 rejects, levels[i] = scaleLevel of :1012-1014.  n_mps = nMPs, n_redundant = nRedundantObservations
 * with thObs = th_obs (3 there).  The results of one enqueue hold up to and including the first job whose keyframe
 * the caller culls: SetBadFlag erases its observations and changes the later counts. */
#define VSLAM_COVIS_MAX_JOBS 128
#define VSLAM_COVIS_MAX_LIST 8192
#define VSLAM_COVIS_CONNECTIONS 0
#define VSLAM_COVIS_VOTE 1
typedef struct vslam_covis vslam_covis;
typedef struct vslam_covis_obs {
    int64_t kf_id;
    int32_t left_idx, right_idx;     /* -1: that side does not observe */
    int32_t left_level, right_level; /* -1 likewise */
    int32_t stereo;
    int32_t reserved;
} vslam_covis_obs;
typedef struct vslam_covis_job {
    int32_t mode;
    int32_t map_id;
    int64_t self_kf;
    int32_t min_obs;
    int32_t n;
    const int64_t* mp_ids;
} vslam_covis_job;
typedef struct vslam_covis_result {
    int32_t error;
    int32_t n_counter;
    int32_t n_ordered;
    int32_t n_max;
    int64_t kf_max; /* -1: none */
    int32_t n_tracked;
    int32_t reserved;
} vslam_covis_result;
typedef struct vslam_covis_cull_job {
    int64_t kf_id;
    int32_t n;
    int32_t reserved;
    const int64_t* mp_ids;
    const int32_t* levels;
} vslam_covis_cull_job;
typedef struct vslam_covis_cull_result {
    int32_t error;
    int32_t n_mps;
    int32_t n_redundant;
    int32_t reserved;
} vslam_covis_cull_result;
int vslam_covis_create(int device, int initial_entries, vslam_covis** out);
void vslam_covis_destroy(vslam_covis* c);
/* jobs per enqueue, list entries per job, and the number of live keyframes up to which the kernels keep the
 * histogram in LDS (above it: a global scratch array per job) */
int vslam_covis_limits(int* max_jobs, int* max_list, int* lds_slots);
int vslam_covis_add_keyframe(vslam_covis* c, int64_t kf_id, int32_t map_id, uint64_t order_key);
int vslam_covis_add_keyframes(vslam_covis* c, int n, const int64_t* kf_ids, const int32_t* map_ids, const uint64_t* order_keys);
int vslam_covis_set_keyframe_bad(vslam_covis* c, int64_t kf_id);
int vslam_covis_set_keyframe_map(vslam_covis* c, int64_t kf_id, int32_t map_id);
int vslam_covis_erase_keyframe(vslam_covis* c, int64_t kf_id);
int vslam_covis_add_point(vslam_covis* c, int64_t mp_id);
int vslam_covis_add_observation(vslam_covis* c, int64_t mp_id, int64_t kf_id, int32_t idx, int is_right, int level, int stereo);
int vslam_covis_erase_observation(vslam_covis* c, int64_t mp_id, int64_t kf_id, int* became_bad);
int vslam_covis_clear_point(vslam_covis* c, int64_t mp_id);
int vslam_covis_erase_point(vslam_covis* c, int64_t mp_id);
int vslam_covis_clear_map(vslam_covis* c, int32_t map_id);
int vslam_covis_clear(vslam_covis* c);
int vslam_covis_size(vslam_covis* c, int* n_keyframes, int* n_points, long long* n_observations);
int vslam_covis_stats(vslam_covis* c, long long* capacity, long long* used, int* n_growths, int* n_compactions);
int vslam_covis_get_point(vslam_covis* c, int64_t mp_id, int cap, int* n_obs, int* bad, vslam_covis_obs* obs, int* n_records);
int vslam_covis_connections_async(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_job* jobs);
int vslam_covis_connections_wait(vslam_covis* c, vslam_fe* fe, vslam_covis_result* results /* [n_jobs] */);
int vslam_covis_connections(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_job* jobs, vslam_covis_result* results);
int vslam_covis_connections_lists(vslam_covis* c, int job, int64_t* counter_kf, int32_t* counter_n /* [n_counter] */,
                                  int64_t* ordered_kf, int32_t* ordered_w /* [n_ordered] */);
int vslam_covis_culling_async(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_cull_job* jobs, int th_obs);
int vslam_covis_culling_wait(vslam_covis* c, vslam_fe* fe, vslam_covis_cull_result* results /* [n_jobs] */);
int vslam_covis_culling(vslam_covis* c, vslam_fe* fe, int n_jobs, const vslam_covis_cull_job* jobs, int th_obs,
                        vslam_covis_cull_result* results);
/* HIP-event spans summed over the queries waited for while vslam_fe_set_profiling is on: the upload's scatter kernel,
 * the query kernel; bytes uploaded by those queries */
int vslam_covis_get_profile(vslam_covis* c, double* apply_ms, double* query_ms, long long* upload_bytes, long* passes);

/* FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (fmatcher.cpp:546-748,
 * pinhole frames).  FeatureVectors as produced by vslam_bow_assemble (ascending node ids, offsets, feature
 * indices); kf_flags[i] != 0 iff pKF's i-th keypoint has a MapPoint that is not bad; keypoints only contribute
 * their angles; descriptors are device arrays.  match_f[iF] = KeyFrame feature index whose MapPoint is written to
 * vpMapPointMatches[iF], -1 = NULL; *nmatches as the reference counts it. */
int vslam_search_by_bow(vslam_fe* fe, const vslam_kp* kf_kps_host, const uint8_t* dev_kf_desc,
                        const uint8_t* kf_flags_host, int n_kf, const int32_t* kf_fv_nodes, const int32_t* kf_fv_off,
                        const int32_t* kf_fv_feat, int n_kf_nodes, const vslam_kp* f_kps_host,
                        const uint8_t* dev_f_desc, int n_f, const int32_t* f_fv_nodes, const int32_t* f_fv_off,
                        const int32_t* f_fv_feat, int n_f_nodes, float nnratio, int check_orientation,
                        int32_t* match_f, int* nmatches);

/* FMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (fmatcher.cpp:1100-1240):
 * both sides carry MapPoint flags (exists and not bad), the threshold is bestDist1 < TH_LOW, and the result is
 * indexed by the first KeyFrame: match12[idx1] = idx2 (vpMatches12[idx1] = vpMapPoints2[idx2]) or -1. */
int vslam_search_by_bow_keyframes(vslam_fe* fe, const vslam_kp* kps1_host, const uint8_t* dev_desc1,
                                  const uint8_t* flags1_host, int n1, const int32_t* fv1_nodes, const int32_t* fv1_off,
                                  const int32_t* fv1_feat, int n1_nodes, const vslam_kp* kps2_host,
                                  const uint8_t* dev_desc2, const uint8_t* flags2_host, int n2,
                                  const int32_t* fv2_nodes, const int32_t* fv2_off, const int32_t* fv2_feat,
                                  int n2_nodes, float nnratio, int check_orientation, int32_t* match12, int* nmatches);

/* FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (fmatcher.cpp:546-748) for a two-fisheye
 * rig (F.Nleft != -1): ONE frame against 1 to 16 keyframes in one pass of the kernels (TrackReferenceKeyFrame, tracking.cpp:2578:
 * one keyframe; the Relocalization loop, tracking.cpp:3488-3509: every candidate at once).  Restated as written:
 *   - F has N = n_left + n_right features; descriptor rows and FeatureVector indices run over [0, N), left first
 *     (frame.cpp:1137).  A rig KeyFrame is indexed the same way; KeyFrame features of BOTH sides are queries
 *   - only shared vocabulary nodes are paired (the lower_bound walk)
 *   - for a KeyFrame feature with a good MapPoint ONE pass over the node's frame features skips occupied slots and keeps
 *     bestDist1 / bestDist2 / bestIdxF over realIdxF < n_left, bestDist1R / bestIdxFR over the rest; the first candidate in
 *     FeatureVector order wins a tie
 *   - the left write happens iff bestDist1 <= TH_LOW and the ratio test passes
 *   - the right branch is NESTED in `if (bestDist1 <= TH_LOW)` (:680 within :650): it runs whether or not the left ratio test
 *     passed; it does not run when the left best is above TH_LOW or no free left candidate exists.  Its own ratio test is
 *     `.. || true` (:682): bestDist1R <= TH_LOW alone writes bestIdxFR
 *   - every write counts in nmatches and enters ONE rotation histogram over both sides, with the angles of keypoints_ /
 *     keypointsRight_ by index on both the KeyFrame and the Frame side; a slot is written at most once
 *   - with n_right == 0 on both sides this is vslam_search_by_bow.
 * frame: the device keypoints (their angles) and descriptors of both extractor slots and the counts are read; the match maps and
 * occupied_host are not (the reference starts from an empty vpMapPointMatches).  f_fv_*: the frame's FeatureVector over [0, N)
 * (Vocabulary::transform of the concatenated descriptors), uploaded once for all jobs.  A keyframe job: device descriptors per
 * side (n_right may be 0 and dev_desc_right NULL), ONE host keypoint array keypoints_ then keypointsRight_ (the angle is read),
 * flags_host[i] != 0 iff the i-th feature has a MapPoint that is not bad, its FeatureVector.
 * _async: one upload -> k_sbow_nodes_rig (one wave per job and keyframe node) -> k_sbow_finish_rig (one workgroup per job) -> one
 * result copy on the context's stream, no host wait in between, in a staging block of its own: the blocking matchers may run
 * while a search is in flight.  One such search per context may be in flight (a second _async is VSLAM_ERR_INVALID).
 * _wait: match_f[j] (n_left + n_right entries) = the index of job j's KeyFrame feature whose MapPoint goes to the slot, or -1;
 * nmatches[j] as the reference counts it.
 * Limits: n_left, n_right <= 4096 on every side; at most 2048 frame features (both sides together) under a node that a keyframe
 * shares.  Beyond either _async returns VSLAM_ERR_UNSUPPORTED and nothing is enqueued or in flight; the blocking form then
 * leaves every match_f at -1 and every nmatches at 0.  A FeatureVector whose offsets do not ascend from 0 or whose indices
 * leave [0, n) is VSLAM_ERR_INVALID, checked before anything is enqueued.  Empty inputs (no features, no nodes, an empty job)
 * give an empty result of that job; when no job has anything to match nothing is launched.  The matcher does not project: it
 * runs with or without a KB8 camera set. */
typedef struct vslam_bow_rig_kf {
    const uint8_t* dev_desc_left;  int n_left;   /* descriptor rows [0, NLeft) */
    const uint8_t* dev_desc_right; int n_right;  /* rows [NLeft, NLeft + NRight); may be NULL with n_right == 0 */
    const vslam_kp* kps_host;                    /* n_left + n_right: mvKeys then mvKeysRight */
    const uint8_t* flags_host;                   /* n_left + n_right */
    const int32_t *fv_nodes, *fv_off, *fv_feat;  /* mFeatVec: n_nodes ascending node ids, n_nodes + 1 offsets, indices */
    int n_nodes;
} vslam_bow_rig_kf;
int vslam_search_by_bow_rig_async(vslam_fe* fe, const vslam_bow_rig_kf* kf_jobs, int n_kf_jobs, const vslam_rig_frame* frame,
                                  const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat, int n_f_nodes,
                                  float nnratio, int check_orientation);
int vslam_search_by_bow_rig_wait(vslam_fe* fe, int32_t* const* match_f, int* nmatches);
/* _async + _wait */
int vslam_search_by_bow_rig(vslam_fe* fe, const vslam_bow_rig_kf* kf_jobs, int n_kf_jobs, const vslam_rig_frame* frame,
                            const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat, int n_f_nodes,
                            float nnratio, int check_orientation, int32_t* const* match_f, int* nmatches);
/* With vslam_fe_set_profiling on: HIP-event time of k_sbow_nodes_rig and of k_sbow_finish_rig, summed over the rig BoW searches
 * waited for since vslam_fe_set_profiling was last called: it starts these sums anew.  Any pointer may be NULL. */
int vslam_fe_get_bow_rig_profile(vslam_fe* fe, double* nodes_ms, double* finish_ms, long* passes);

/* The KeyFrame-KeyFrame overload (fmatcher.cpp:1100-1240) for rig KeyFrames.  The reference skips idx >= mvKeysUn.size() on
 * both sides (:1135, :1155) and a rig's mvKeysUn is keypoints_ (NLeft entries): right features are neither queries nor
 * candidates.  n1 / n2 = NLeft + NRight (flags, FeatureVector indices, match12 entries), n_left1 / n_left2 = NLeft; kps*_host
 * hold n_left entries (mvKeysUn); only descriptor rows < n_left are read, so dev_desc* are the left arrays.  The flags are
 * staged with the entries >= n_left cleared and vslam_search_by_bow_keyframes' kernels run as they are. */
int vslam_search_by_bow_keyframes_rig(vslam_fe* fe, const vslam_kp* kps1_host, const uint8_t* dev_desc1,
                                      const uint8_t* flags1_host, int n1, int n_left1, const int32_t* fv1_nodes,
                                      const int32_t* fv1_off, const int32_t* fv1_feat, int n1_nodes, const vslam_kp* kps2_host,
                                      const uint8_t* dev_desc2, const uint8_t* flags2_host, int n2, int n_left2,
                                      const int32_t* fv2_nodes, const int32_t* fv2_off, const int32_t* fv2_feat, int n2_nodes,
                                      float nnratio, int check_orientation, int32_t* match12, int* nmatches);

/* FMatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (fmatcher.cpp:1242-1482)
 * and its cv::Matx twin SearchForTriangulation_ (:1484-1725, the one LocalMapping::CreateNewMapPoints calls,
 * localmapping.cpp:447) for pinhole KeyFrames without a second camera.  F12 is the matrix
 * Pinhole::epipolarConstrain builds for the pair, K1^-T [t12]x R12 K2^-1 (pinhole.cpp:121-127, row-major; it does
 * not depend on the keypoints, so the caller computes it once with its own cv::Mat algebra); (ep_x, ep_y) is the
 * epipole pKF2->mpCamera->project(R2w*Cw + t2w) (fmatcher.cpp:1249-1254).  kps*_host are mvKeysUn, has_mp*[i] != 0
 * iff GetMapPoint(i) != NULL, u_right* are mvuRight; FeatureVectors as produced by vslam_bow_assemble; the scale
 * tables of pKF2 are the context's (vslam_fe_tables).  match12[idx1] = idx2 or -1 -- vMatchedPairs is the list of
 * (idx1, match12[idx1]) with match12[idx1] >= 0 in ascending idx1; the reference never marks KeyFrame-2 features
 * as taken, so an idx2 may appear more than once.  *nmatches as the reference returns it. */
typedef struct vslam_tri_params {
    float F12[9];
    float ep_x, ep_y;
    int32_t only_stereo, coarse, check_orientation;
} vslam_tri_params;
int vslam_search_for_triangulation(vslam_fe* fe, const vslam_tri_params* p, const vslam_kp* kps1_host,
                                   const uint8_t* dev_desc1, const uint8_t* has_mp1_host, const float* u_right1_host,
                                   int n1, const int32_t* fv1_nodes, const int32_t* fv1_off, const int32_t* fv1_feat,
                                   int n1_nodes, const vslam_kp* kps2_host, const uint8_t* dev_desc2,
                                   const uint8_t* has_mp2_host, const float* u_right2_host, int n2,
                                   const int32_t* fv2_nodes, const int32_t* fv2_off, const int32_t* fv2_feat,
                                   int n2_nodes, int32_t* match12, int* nmatches);

/* The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (fmatcher.cpp:1918-2119) and of
 * Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:2121-2243; sim3 = 1, Rcw/tcw/Ow as the function derives them from
 * Scw at :2130-2134): for every MapPoint the projection gates, MapPoint::PredictScale, the window of
 * KeyFrame::GetFeaturesInArea and the keypoint with the least descriptor distance (first of the window order wins).
 * best_idx[i] = -1 (best_dist[i] = 256) when a gate rejects the point or no keypoint passes; distances above 255 are
 * reported as 255.  The caller walks the results in order and does what the reference does when
 * best_dist[i] <= TH_LOW (50): Replace / AddObservation + AddMapPoint / vpReplacePoint -- re-checking isBad() and
 * IsInKeyFrame() at that moment, because those are the only inputs an earlier iteration can change.
 * valid = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF) when the call is made. */
typedef struct vslam_fuse_point {
    float pos[3];       /* GetWorldPos() */
    float normal[3];    /* GetNormal() */
    float min_distance; /* GetMinDistanceInvariance() */
    float max_distance; /* GetMaxDistanceInvariance() */
    int32_t valid;
} vslam_fuse_point;
typedef struct vslam_fuse_params {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, bf, th;
    float log_scale_factor; /* pKF->mfLogScaleFactor */
    int32_t img_w, img_h;   /* mnMaxX, mnMaxY (mnMinX = mnMinY = 0: undistorted pinhole images); while the context holds grid
                             * bounds (vslam_fe_set_grid_bounds) those are used -- as pKF holds them, truncated to int */
    int32_t sim3;           /* 0 / 1: the two Fuse overloads; 2: one direction of SearchBySim3, see below */
    int32_t gemm_float;     /* as in vslam_proj_params */
    float Rb[9], tb[3];     /* sim3 == 2 only */
} vslam_fuse_params;
/* FMatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (fmatcher.cpp:2245-2469) is two such searches
 * (sim3 = 2) and an agreement check.  Direction 1 -> 2: Rcw | tcw = R1w | t1w, Rb | tb = sR21 | t21 (:2262-2264),
 * the points are pKF1's MapPoints that are not bad and not matched yet, the KeyFrame is pKF2; direction 2 -> 1 with
 * R2w | t2w and sR12 | t12.  A point is p2 = Rb*(Rcw*p + tcw) + tb, depth >= 0, u = fx*(x*(1.0/z)) + cx, IsInImage,
 * |p2| within the scale-invariance range, PredictScale, window, levels [l-1, l], least distance (first wins); Ow,
 * normals, bf are unused.  The caller keeps vnMatch1[i1] = best_idx where best_dist <= TH_HIGH (100), likewise
 * vnMatch2, and accepts (i1, idx2) iff vnMatch2[idx2] == i1 (:2453-2466). */
int vslam_fuse_search(vslam_fe* fe, const vslam_fuse_params* p, const vslam_fuse_point* points_host,
                      const uint8_t* mp_desc_host, int n_points, const vslam_kp* dev_kf_kps,
                      const uint8_t* dev_kf_desc, int n_kf, const float* kf_u_right_host, int32_t* best_idx,
                      int32_t* best_dist);

/* The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame (fmatcher.cpp:1918-2119 with a
 * KannalaBrandt8 camera; bRight = true and pKF->NLeft != -1: a two-fisheye rig) and of Fuse(pKF, Scw, vpPoints, th,
 * vpReplacePoint) (:2121-2243) with such a KeyFrame: ONE list of MapPoints against up to 16 (KeyFrame, camera) jobs in one
 * enqueue.  LocalMapping::SearchInNeighbors (localmapping.cpp:776-782, :809-810) calls Fuse(pKFi, ..) and Fuse(pKFi, .., true)
 * for every target KeyFrame; the search half reads of a MapPoint its position, normal, distance range, descriptor, isBad() and
 * IsInKeyFrame(pKF), and an earlier call's map mutation changes only the last two (towards "skip") and the descriptor of the
 * survivor of a Replace (mappoint.cpp:292).  So the searches of several calls can run before the first mutation; INTEGRATION.md
 * ("Fuse for a rig") states the walk that makes the caller's result equal to the sequential one.
 * Restated as written, per job and MapPoint:
 *   - p3Dc = Rcw * p3Dw + tcw as one gemm; z < 0 rejects, z == 0 goes on.  invz and ur are dead in a rig (below) and not computed
 *   - uv = pCamera->project(x, y, z): KannalaBrandt8::project with THE JOB'S OWN camera -- mpCamera2 for bRight (:1929), unlike
 *     the right branch of SearchByProjection(CurrentFrame, LastFrame), which projects through the left model
 *   - KeyFrame::IsInImage (closed below, open above) over the KeyFrame's integer copy of the grid bounds; cv::norm(p3Dw - Ow)
 *     within [min_distance, max_distance]; PO.dot(Pn) < 0.5 * dist3D rejects (both accumulated in double); PredictScale; radius
 *     th * scale[level]
 *   - KeyFrame::GetFeaturesInArea(u, v, r, bRight) over the side's own grid and keypoints (keyframe.cpp:656-699): columns outer,
 *     rows inner, ascending index within a cell; level gate [level - 1, level]
 *   - chi2: a rig's mvuRight is vector<float>(Nleft, -1) (frame.cpp:1160), and so is a monocular fisheye's: every defined entry
 *     is negative, the monocular branch e2 * invSigma2[kpLevel] > 5.99 rejects.  ODDITY, NOT reproduced: the right call reads
 *     mvuRight[idx] with the RIGHT-LOCAL index (:2053, before :2079 adds NLeft), i.e. a left feature's entry, or past the end
 *     of the vector where idx >= Nleft (undefined behaviour); the restatement reads -1 everywhere.  sim3 = 1 has no chi2 gate
 *   - least distance, `dist < bestDist` from 256: the first of the window order wins a tie and a distance of 256 never wins;
 *     sim3 = 1 starts from INT_MAX: where nothing is nearer than 256 the first candidate at 256 is reported (best_dist 256)
 *   - the reported index is the side-local index plus idx_offset (:2079); nothing passes: best_idx -1, best_dist 256.
 * sim3 = 1 reads pKF->mpCamera and the left keypoints only: camera 0, idx_offset 0, Rcw / tcw / Ow derived from Scw by the
 * caller as for vslam_fuse_search.  A monocular fisheye KeyFrame (NLeft == -1) is one job with camera 0 and idx_offset 0.
 * points[i].valid = pMP && !pMP->isBad(); a job's valid_host[i] = !pMP->IsInKeyFrame(pKF) (sim3 = 1: !spAlreadyFound.count).
 * Of p are read th, log_scale_factor, img_w, img_h and gemm_float; fx, fy, cx, cy, bf, Rcw, tcw, Ow, sim3, Rb and tb are NOT
 * read (pose and switches are the job's, the intrinsics the cameras').  A KB8 camera must be set (VSLAM_ERR_INVALID
 * otherwise); rig may be NULL when no job has camera == 1.  The window grid and IsInImage use the context's float grid bounds
 * or {0, img_w, 0, img_h}, truncated for the KeyFrame as in vslam_fuse_search.  points / mp_desc / points_where: as for
 * vslam_search_local_points_async (host or DEVICE arrays, untouched until _wait returns).
 * n_jobs outside 1..16: VSLAM_ERR_INVALID.  n_points > VSLAM_LOCAL_POINTS_MAX or a job with n_kf > 4096:
 * VSLAM_ERR_UNSUPPORTED.  Nothing is enqueued then, and the blocking form leaves -1 / 256 in every one of its n_jobs * n_points
 * outputs (for n_jobs > 16 too: the caller sized them by n_jobs; n_jobs < 1 names no outputs).  A job's dev_desc must be
 * 16-byte aligned (the rows are read 16 bytes at a time; rows [NLeft, ..) of an aligned mDescriptors are) and its dev_kps
 * 4-byte aligned: VSLAM_ERR_INVALID otherwise.  n_points == 0 and
 * jobs with n_kf == 0 are ordinary inputs with empty results.  One upload, one launch (k_fuse_rank_rig, grid (ceil(n_points /
 * 16), n_jobs)), one result copy, no host wait in between; the staging block is the entry's own, so the blocking matchers may
 * run between _async and _wait.  One search per context may be in flight: a second _async is VSLAM_ERR_INVALID.
 * _wait: best_idx / best_dist, n_jobs * n_points entries each, job-major. */
#define VSLAM_FUSE_RIG_MAX_JOBS 16
typedef struct vslam_fuse_rig_job {   /* one call of Fuse(pKF, vpMapPoints, th, bRight): one camera of one KeyFrame */
    float Rcw[9], tcw[3], Ow[3];      /* GetRotation / GetTranslation / GetCameraCenter, or the GetRight* ones for bRight */
    int32_t camera;                   /* 0 = the context's KB8 camera (mpCamera), 1 = rig->cam2 (mpCamera2) */
    int32_t sim3;                     /* 0: Fuse(pKF, vpMapPoints, th, bRight); 1: Fuse(pKF, Scw, ..) (camera must be 0) */
    const vslam_kp* dev_kps;          /* mvKeys / mvKeysRight (a rig's mvKeysUn == mvKeys): the side's own array, DEVICE */
    const uint8_t* dev_desc;          /* the side's descriptor rows, DEVICE, 16-byte aligned: mDescriptors rows [0, NLeft) or [NLeft, NLeft + NRight) */
    int32_t n_kf;                     /* keypoints of this side, <= 4096 */
    int32_t idx_offset;               /* added to a reported index: 0, or NLeft for bRight (fmatcher.cpp:2079) */
    const uint8_t* valid_host;        /* n_points bytes, 0 = IsInKeyFrame(pKF) (or spAlreadyFound); NULL = all 1 */
} vslam_fuse_rig_job;
int vslam_fuse_search_rig_async(vslam_fe* fe, const vslam_fuse_params* p, const vslam_kb8_rig* rig,
                                const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                const uint8_t* mp_desc, int n_points, int points_where);
int vslam_fuse_search_rig_wait(vslam_fe* fe, int32_t* best_idx, int32_t* best_dist);
/* _async + _wait */
int vslam_fuse_search_rig(vslam_fe* fe, const vslam_fuse_params* p, const vslam_kb8_rig* rig, const vslam_fuse_rig_job* jobs,
                          int n_jobs, const vslam_fuse_point* points, const uint8_t* mp_desc, int n_points, int points_where,
                          int32_t* best_idx, int32_t* best_dist);
/* With vslam_fe_set_profiling on: HIP-event time of k_fuse_rank_rig alone, summed over the searches waited for since
 * profiling was switched on.  Either pointer may be NULL. */
int vslam_fe_get_fuse_rig_profile(vslam_fe* fe, double* rank_ms, long* passes);

/* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (fmatcher.cpp:2689-2811) with a
 * fisheye CurrentFrame: a monocular KB8 frame (Nleft == -1) or the left camera of a two-fisheye rig -- the matcher of
 * Tracking::Relocalization (tracking.cpp:3570, :3584).  Blocking: Relocalization optimises the pose between its two calls.
 * The arguments are those of vslam_search_by_projection_keyframe; a KB8 camera must be set (VSLAM_ERR_INVALID otherwise) and
 * fx, fy, cx, cy of p must equal its intrinsics bit for bit.  Limits as there: 4096 current keypoints, 4096 KeyFrame entries.
 * Restated as written, per KeyFrame entry i with mp_flags[i] & 1:
 *   - x3Dc = Rcw * x3Dw + tcw as one gemm (gemm_float as elsewhere); uv = KannalaBrandt8::project(x3Dc)
 *   - there is NO depth test: a point behind the camera is projected like any other (theta > pi / 2) and, where it lands inside
 *     the bounds, goes on and can take a keypoint
 *   - the closed interval over the Frame's float bounds mnMinX..mnMaxY (the context's grid bounds while some are set, else
 *     {0, img_w, 0, img_h}); dist3D = cv::norm(x3Dw - Ow) within [min, max]; PredictScale; radius = th * scale[level];
 *     GetFeaturesInArea(u, v, r, level - 1, level + 1)
 *   - a rig: bRight defaults to false (frame.cpp:678-744), so only the left grid and keypoints_ are searched and only slots
 *     [0, Nleft) are read or written: n_cur = Nleft, dev_cur_kps / dev_cur_desc the left arrays, and n_kf = NLeft + NRight
 *     (GetMapPointMatches() has N entries)
 *   - occupied slots are skipped; `dist < bestDist` from 256: the first of the window order wins a tie; bestDist <= ORBdist;
 *     a written slot blocks later points; one rotation histogram, ComputeThreeMaxima, nmatches.
 * ODDITY, NOT reproduced: with mbCheckOrientation :2774 reads pKF->mvKeysUn[i].angle for every i < N, but a rig KeyFrame's
 * mvKeysUn has only NLeft entries (keyframe.cpp:40 copies F.ukeypoints_, which frame.cpp:764 set to keypoints_), so for a
 * right-camera MapPoint, i >= NLeft, the reference reads past the end of the vector (undefined behaviour); the restatement
 * reads the angle of mvKeysRight[i - NLeft].  kf_kps_host is therefore ONE array, mvKeys followed by mvKeysRight, as
 * vslam_bow_rig_kf takes it. */
int vslam_search_by_projection_keyframe_kb8(vslam_fe* fe, const vslam_proj_params* p, const float* Ow, float log_scale_factor,
                                            int orb_dist, const vslam_kp* kf_kps_host, int n_kf, const uint8_t* mp_flags,
                                            const float* mp_x3dw, const float* mp_min_dist, const float* mp_max_dist,
                                            const uint8_t* mp_desc_host, const vslam_kp* dev_cur_kps,
                                            const uint8_t* dev_cur_desc, int n_cur, const uint8_t* cur_occupied_host,
                                            int32_t* match_cur, int* nmatches);

/* FMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863) for fisheye KeyFrames:
 * ONE list of MapPoints against 1..16 (KeyFrame, Scw) jobs in one enqueue.  LoopClosing::DetectCommonRegionsFromBoW
 * (loopclosing.cpp:668-684) calls FindMatchesByProjection (:751-803) for up to five covisible KeyFrames with the same
 * pMostBoWMatchesKF, so with the same vpMapPoints, each with its own Sjw and a fresh vpMatched: jobs that do not interact.
 * points[i].valid = !pMP->isBad(); a job's valid_host[i] = !spAlreadyFound.count(pMP) (NULL = all), kf_matched_host[idx] =
 * vpMatched[idx] != NULL on entry (NULL = none); Rcw / tcw / Ow derived from Scw by the caller (:760-764) as for
 * vslam_search_by_projection_sim3; dev_kps / dev_desc the KeyFrame's LEFT keypoints and descriptor rows.  A KB8 camera must be
 * set (VSLAM_ERR_INVALID otherwise); a rig KeyFrame's mpCamera is the left one.  points / mp_desc / points_where as for
 * vslam_fuse_search_rig_async (host or DEVICE arrays), up to VSLAM_LOCAL_POINTS_MAX points.
 * Restated as written, per job and point in ascending iMP:
 *   - p3Dc = Rcw * p3Dw + tcw as one gemm; z < 0 rejects, z == 0 goes on; KannalaBrandt8::project with the context's camera
 *   - KeyFrame::IsInImage over the KeyFrame's integer bounds, closed below and open above; cv::norm(p3Dw - Ow) within the
 *     range; PO.dot(Pn) < 0.5 * dist rejects (both sides in double); PredictScale; radius = th * scale[level] (th an int)
 *   - KeyFrame::GetFeaturesInArea(u, v, r) over the left grid: columns outer, rows inner, ascending index within a cell;
 *     matched keypoints are skipped; level gate [level - 1, level]; `dist < bestDist` from 256; accepted on bestDist <=
 *     TH_LOW * ratioHamming (the float product floored, capped at 255); vpMatched[bestIdx] = pMP blocks later points; no
 *     rotation check.
 * The list is long (the MapPoints of a KeyFrame, of its covisibles and of theirs): a gate pass over (job, point) evaluates
 * everything up to the radius, an order-preserving compaction hands the 4096-wide matcher only a job's survivors, and the
 * reported match_kf[idx] is the ORIGINAL iMP.  _wait delivers per job match_kf[j] (n_kf entries), nmatches[j] and n_gated[j]
 * (the survivors).  A job with more than 4096 survivors gets nmatches -1 and -1 in every entry; the call then returns
 * VSLAM_ERR_UNSUPPORTED after the other jobs' results are delivered (run that job through the host twin).
 * n_jobs outside 1..16 or a misaligned pointer (dev_desc and device mp_desc 16 bytes, dev_kps and device points 4):
 * VSLAM_ERR_INVALID.  n_points > VSLAM_LOCAL_POINTS_MAX or a job with n_kf > 4096: VSLAM_ERR_UNSUPPORTED.  Nothing is enqueued
 * then, and the blocking form leaves -1 in every output of every job (for n_jobs > 16 too: the caller sized them by n_jobs).
 * n_points == 0 and jobs with n_kf == 0 are ordinary inputs with empty results.  One upload, no host wait between the launches
 * (k_s3k_gate, k_s3k_compact, k_sbp_rank_kb8, k_sbp_resolve, k_sbp_replay, k_s3k_finish), one result copy; the staging block
 * is the entry's own, so the blocking matchers may run between _async and _wait.  One search per context may be in flight: a
 * second _async is VSLAM_ERR_INVALID. */
#define VSLAM_SIM3_KB8_MAX_JOBS 16
typedef struct vslam_sim3_kb8_job {   /* one call of SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) */
    float Rcw[9], tcw[3], Ow[3];      /* sRcw / scw, Scw's translation / scw, -Rcw^T tcw (fmatcher.cpp:760-764) */
    const vslam_kp* dev_kps;          /* pKF's left keypoints (mvKeysUn), DEVICE, 4-byte aligned */
    const uint8_t* dev_desc;          /* mDescriptors rows [0, n_kf), DEVICE, 16-byte aligned */
    int32_t n_kf;                     /* <= 4096 */
    int32_t pad;
    const uint8_t* kf_matched_host;   /* n_kf bytes: vpMatched[idx] != NULL on entry; NULL = none */
    const uint8_t* valid_host;        /* n_points bytes: !spAlreadyFound.count(pMP); NULL = all 1 */
} vslam_sim3_kb8_job;
typedef struct vslam_sim3_kb8_params {
    int32_t th;                       /* an int in this overload */
    float ratio_hamming;
    float log_scale_factor;           /* pKF->mfLogScaleFactor */
    int32_t img_w, img_h;             /* the bounds while vslam_fe_set_grid_bounds has set none */
    int32_t gemm_float;
} vslam_sim3_kb8_params;
int vslam_search_by_projection_sim3_kb8_async(vslam_fe* fe, const vslam_sim3_kb8_params* p, const vslam_sim3_kb8_job* jobs,
                                              int n_jobs, const vslam_fuse_point* points, const uint8_t* mp_desc, int n_points,
                                              int points_where);
int vslam_search_by_projection_sim3_kb8_wait(vslam_fe* fe, int32_t* const* match_kf, int* nmatches, int* n_gated);
/* _async + _wait */
int vslam_search_by_projection_sim3_kb8(vslam_fe* fe, const vslam_sim3_kb8_params* p, const vslam_sim3_kb8_job* jobs, int n_jobs,
                                        const vslam_fuse_point* points, const uint8_t* mp_desc, int n_points, int points_where,
                                        int32_t* const* match_kf, int* nmatches, int* n_gated);
/* With vslam_fe_set_profiling on: HIP-event time of gate + compaction, of the ranking and of the resolution (k_sbp_resolve,
 * k_sbp_replay, k_s3k_finish), summed over the searches waited for since.  Any pointer may be NULL. */
int vslam_fe_get_sim3_kb8_profile(vslam_fe* fe, double* gate_ms, double* rank_ms, double* resolve_ms, long* passes);

/* Evaluate the device float helpers on host arrays (round trip through HBM): the glibc-exact sinf/cosf
 * used for the rBRIEF rotation (fextractor.cpp:103-104) and cv::fastAtan2 (fextractor.cpp:94). */
int vslam_dbg_sincos(vslam_fe* fe, const float* x, int n, float* sin_out, float* cos_out);
int vslam_dbg_fast_atan2(vslam_fe* fe, const float* y, const float* x, int n, int fma, float* deg);
/* glibc logf as MapPoint::PredictScale uses it (mappoint.cpp:514); normal positive inputs, NaN otherwise */
int vslam_dbg_logf(vslam_fe* fe, const float* x, int n, float* y);
/* Quadtree statistics of a context: how many (slot, level) DistributeOctTree problems (fextractor.cpp:530-754) ran on the
 * device so far, on how many of them nodes had to be split BELOW the kernel's fine grid (keys closer together than a fine
 * cell -- real images do that on sparse levels; resolved inside the kernel, same result, a little slower), and --
 * last_level_masks, max_batch words or NULL -- bit l of word s set if that happened on level l of slot s in the last pass.
 * Updated when a pass's results are collected. */
int vslam_fe_octree_stats(const vslam_fe* fe, unsigned long long* problems, unsigned long long* split_below_grid,
                          uint32_t* last_level_masks);
/* Result deliveries of a context so far: how many copy operations (a runtime copy or one launch of the copy kernel) the
 * extraction and SearchForInitialization paths put on the stream towards the host, and the bytes they carried.  A full
 * batch with want_host = 1 is one operation, the matcher's outputs another; with want_host = 2 the step is ONE. */
int vslam_fe_delivery_stats(const vslam_fe* fe, unsigned long long* transfers, unsigned long long* bytes);
/* In-kernel time stamps of the quadtree kernel (100 MHz ticks; out64[63] = count).  Only a library built with
 * -DVSLAM_OCT_STAMPS and a context created under VSLAM_OCT_DBG=1 records them; otherwise VSLAM_ERR_INVALID. */
int vslam_dbg_octree_stamps(vslam_fe* fe, unsigned long long* out64);
/* Number of queries for which the device SearchForInitialization had to re-scan the whole window because the
 * sorted candidate prefix (length VSLAM_INIT_TOPM, default 8) was exhausted; read-and-reset, synchronises. */
int vslam_dbg_search_init_fallbacks(vslam_fe* fe, int* count);
/* Rounds of the replay wave, queries and pairs it decided since the last call (read-and-reset, synchronises): the
 * sequential half of SearchForInitialization commits `queries / rounds` queries per round on average. */
int vslam_dbg_search_init_replay_stats(vslam_fe* fe, int* rounds, int* queries, int* pairs);
/* What this library holds right now, process-wide: bytes and blocks of device memory and of pinned host memory that its
 * objects (contexts, detectors, trackers, vocabularies, keyframe databases) own.  Any pointer may be NULL.  A create /
 * use / destroy sequence leaves all four where they were; the device's own free-memory figure cannot show that on a
 * GPU that other processes use too.  Memory handed out by vslam_host_alloc belongs to the caller and is not counted. */
int vslam_dbg_live_memory(unsigned long long* device_bytes, unsigned long long* device_blocks,
                          unsigned long long* pinned_bytes, unsigned long long* pinned_blocks);

#ifdef __cplusplus
}
#endif
#endif /* VSLAM_FE_H */
