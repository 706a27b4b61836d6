/* vslam_stereo.hip -- stereo half of the matcher ABI: Frame::ComputeStereoMatches and Frame::ComputeStereoFromRGBD on the
 * device behind the extraction of a stereo / RGB-D frame, and the stereo points (UnprojectStereo) kept in HBM for the
 * device-resident SearchByProjection. */
#include "vslam_ctx.h"

/* ------------------------------------------------------------------ stereo */
struct StereoScratch { /* carved out of fe->d_stereo */
    uint32_t* best;
    float* uRight;
    float* depth;
    int32_t* sad;
    uint8_t* rows; /* row table of the right keypoints (vk_stereo_rows_bytes) */
    int max_band;
};

static int stereo_scratch(vslam_fe* fe, int njobs, int capR, StereoScratch* s) {
    const size_t n = (size_t)njobs * fe->cap;
    /* rows of a right keypoint's band: floor(y - 2s) .. ceil(y + 2s), s <= the coarsest level's scale factor */
    s->max_band = 2 * (int)std::ceil(2.0f * fe->tab.scale[fe->p.nlevels - 1]) + 3;
    const size_t rows_bytes = vk_stereo_rows_bytes(njobs, fe->p.height, s->max_band, capR);
    int rc = fe->d_stereo.ensure(n * 16 + rows_bytes + 16);
    if (rc) return rc;
    s->best = (uint32_t*)fe->d_stereo;
    s->uRight = (float*)(s->best + n);
    s->depth = s->uRight + n;
    s->sad = (int32_t*)(s->depth + n);
    s->rows = (uint8_t*)(s->sad + n);
    return fe->h_stereo.ensure(n * 2);
}

/* mvuRight | mvDepth of npairs pairs (uRight, then depth, npairs x cap floats each) to the host, enqueued on fe's stream */
static int send_stereo_outputs(vslam_fe* fe, int npairs, const float* uRight, bool in_block) {
    const size_t n = (size_t)npairs * fe->cap;
    fe->h_stereo_cur = in_block ? (float*)(fe->h_res + fe->res_feat_bytes) : fe->h_stereo;
    if (in_block && fe->deliver_deferred) {
        /* the extraction of this call left its delivery to us (want_host = 2): counts | keypoints | descriptors | mvuRight |
         * mvDepth are contiguous -> ONE transfer for the whole stereo step */
        fe->deliver_deferred = false;
        const int rc = vslam_deliver_block(fe, n * 8);
        if (rc) return rc;
    } else {
        /* uRight | depth */
        vslam_count_delivery(fe, vslam_copy_range(fe->stream, fe->h_stereo_cur, uRight, n * 8, fe->tune), n * 8);
        HIPCHK(hipGetLastError());
    }
    fe->stereo_pairs = npairs;
    return VSLAM_OK;
}

/* enqueue the matcher kernels and the D2H of mvuRight/mvDepth (whole capacity: the keypoint counts may
 * not be known on the host yet); nothing waits */
static int enqueue_stereo(vslam_fe* feL, vslam_fe* feR, int npairs, const int* slotsL, const int* slotsR,
                          float bf, float fx, bool in_block = false) {
    if (feL->p.device != feR->p.device || feL->p.width != feR->p.width || feL->p.height != feR->p.height ||
        feL->p.nlevels != feR->p.nlevels || feL->p.scale_factor != feR->p.scale_factor) {
        g_err = "left/right extractors must share device and geometry";
        return VSLAM_ERR_INVALID;
    }
    StereoJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int j = 0; j < npairs; j++) {
        const int sL = slotsL[j], sR = slotsR[j];
        if (sL < 0 || sL >= feL->B || sR < 0 || sR >= feR->B || !feL->src.l0[sL] || !feR->src.l0[sR]) {
            g_err = "slot not extracted";
            return VSLAM_ERR_INVALID;
        }
        StereoJob& jb = jobs.job[j];
        jb.kpsL = feL->d_kps + (size_t)sL * feL->cap;
        jb.descL = feL->d_desc + (size_t)sL * feL->cap * 32;
        jb.kpsR = feR->d_kps + (size_t)sR * feR->cap;
        jb.descR = feR->d_desc + (size_t)sR * feR->cap * 32;
        jb.cntL = feL->d_counts + sL * 4;
        jb.cntR = feR->d_counts + sR * 4;
        jb.slotL = sL;
        jb.slotR = sR;
    }
    if (feL != feR) HIPCHK(vslam_stream_wait(feR->stream)); /* right results must be complete */
    feL->last_rgbd = false; /* the stereo outputs of feL are the matcher's from here on */
    StereoScratch sc;
    int rc = stereo_scratch(feL, npairs, feR->cap, &sc);
    feL->stereo_capR = feR->cap;
    if (rc) return rc;
    if (in_block) { /* mvuRight | mvDepth behind the extraction's results in the context's result block: one delivery */
        sc.uRight = (float*)(feL->d_res + feL->res_feat_bytes);
        sc.depth = sc.uRight + (size_t)npairs * feL->cap;
    }
    feL->d_stereo_u = sc.uRight; /* device-side consumers (UnprojectStereo, vslam_stereo_points_buffers) read them here */
    feL->d_stereo_depth = sc.depth;
    /* frame.cpp:853-855: mb = mbf/fx (frame.cpp:157), minZ = mb, maxD = mbf/minZ */
    const float mb = bf / fx;
    const float maxD = bf / mb;
    hipStream_t st = feL->stream;
    vk_stereo(st, jobs, npairs, feL->cap, feR->cap, feL->geom, feL->d_pyr, feL->slot_stride, feL->src, feR->d_pyr,
              feR->slot_stride, feR->src, bf, maxD, sc.best, sc.uRight, sc.depth, sc.sad, feL->cap, sc.max_band, sc.rows);
    HIPCHK(hipGetLastError());
    if ((rc = send_stereo_outputs(feL, npairs, sc.uRight, in_block))) return rc;
    for (int j = 0; j < npairs; j++) feL->stereo_slotL[j] = slotsL[j];
    return VSLAM_OK;
}

static void deliver_stereo(vslam_fe* feL, float* const* u_right, float* const* depth) {
    const size_t n = (size_t)feL->stereo_pairs * feL->cap;
    for (int j = 0; j < feL->stereo_pairs; j++) {
        const int nL = feL->n_out[feL->stereo_slotL[j]];
        if (!nL) continue;
        if (u_right && u_right[j]) memcpy(u_right[j], feL->h_stereo_cur + (size_t)j * feL->cap, (size_t)nL * 4);
        if (depth && depth[j]) memcpy(depth[j], feL->h_stereo_cur + n + (size_t)j * feL->cap, (size_t)nL * 4);
    }
}

extern "C" int vslam_stereo_match_batch(vslam_fe* feL, vslam_fe* feR, int npairs, const int* slotsL,
                                        const int* slotsR, float bf, float fx, float* const* u_right,
                                        float* const* depth) {
    if (!feL || !feR || npairs < 1 || npairs > VSLAM_MAX_STEREO_JOBS || !slotsL || !slotsR || !u_right || !depth) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(feL->p.device));
    int rc = enqueue_stereo(feL, feR, npairs, slotsL, slotsR, bf, fx);
    if (rc) return rc;
    HIPCHK(vslam_stream_wait(feL->stream));
    deliver_stereo(feL, u_right, depth);
    return VSLAM_OK;
}

extern "C" int vslam_stereo_match(vslam_fe* feL, int sL, vslam_fe* feR, int sR, float bf, float fx,
                                  float* u_right, float* depth) {
    float* u[1] = {u_right};
    float* d[1] = {depth};
    return vslam_stereo_match_batch(feL, feR, 1, &sL, &sR, bf, fx, u, d);
}

/* The extraction + stereo section of Frame::Frame(stereo) (frame.cpp:102-132) for npairs frames in one
 * enqueue: images are L0,R0,L1,R1,...; slot 2j = left, 2j+1 = right of pair j. */
extern "C" int vslam_frame_stereo_batch_async(vslam_fe* fe, int npairs, const uint8_t* const* imgs, size_t pitch,
                                              int imgs_on_device, float bf, float fx, int want_host) {
    if (!fe || npairs < 1 || npairs > VSLAM_MAX_STEREO_JOBS || 2 * npairs > fe->B ||
        (imgs_on_device != VSLAM_IMGS_STAGED && (!imgs || pitch < vslam_row_bytes(fe))) || imgs_on_device < 0 ||
        imgs_on_device > VSLAM_IMGS_STAGED) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    /* a full batch whose results go to the host: mvuRight / mvDepth live behind the extraction's results in the result
     * block (the region SearchForInitialization's outputs use in a context that runs that matcher: whoever comes first
     * in a context's life owns it) and the whole step leaves in one transfer */
    const bool blk = want_host && 2 * npairs == fe->B && fe->res_init_bytes >= (size_t)npairs * fe->cap * 8 &&
                     fe->block_region_owner != VSLAM_REGION_INIT && fe->d_res;
    if (blk) fe->block_region_owner = VSLAM_REGION_STEREO;
    /* stereo frames: the contexts of a pipelined caller are independent of each other and the step is the sum of the wide
     * kernels' single-context times; the descriptor kernel alone is 8-10 % shorter with one keypoint per wave (48 VGPRs, 8 waves
     * per SIMD) than with four (110 VGPRs, 4 waves, the trigonometry of four keypoints in one pass: fewer instructions, which
     * is what the VALU-bound mono pipeline wants): KITTI stereo +3.3 %, profiles/r04_describe_kpw_ab.txt */
    fe->desc_kpw_hint = 1;
    fe->pyr_resident_hint = true; /* and the resident pyramid tiles: see create_pyramid */
    int rc = vslam_enqueue_extract(fe, 2 * npairs, imgs, pitch, imgs_on_device, 0, 0, blk ? 2 : (want_host != 0));
    fe->desc_kpw_hint = -1;
    fe->pyr_resident_hint = false;
    if (rc == VSLAM_OK) {
        int sl[VSLAM_MAX_STEREO_JOBS], sr[VSLAM_MAX_STEREO_JOBS];
        for (int j = 0; j < npairs; j++) {
            sl[j] = 2 * j;
            sr[j] = 2 * j + 1;
        }
        rc = enqueue_stereo(fe, fe, npairs, sl, sr, bf, fx, blk);
    }
    if (rc != VSLAM_OK) hipStreamSynchronize(fe->stream);
    return rc;
}

extern "C" int vslam_frame_stereo_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                                       float* const* u_right, float* const* depth) {
    if (!fe || fe->last_nimg < 2) {
        g_err = "nothing enqueued";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_finish_extract(fe, fe->last_nimg);
    if (rc != VSLAM_OK) return rc;
    rc = vslam_deliver(fe, fe->last_nimg, kps, desc, cap, n, nullptr);
    if (rc != VSLAM_OK) return rc;
    deliver_stereo(fe, u_right, depth);
    return VSLAM_OK;
}

/* The extraction + depth section of Frame::Frame(imGray, imDepth, ...) (frame.cpp:185-257) for nframes frames in one enqueue:
 * slot j = frame j.  The extraction may replay the context's captured graph; Frame::ComputeStereoFromRGBD (k_rgbd_depth) is
 * always a plain launch behind it, with this call's depth pointers and parameters as its arguments, so a replay can never
 * read the depth images of an earlier call.  mvuRight / mvDepth take the stereo matcher's place: "pair j" = slot j. */
extern "C" int vslam_frame_rgbd_batch_async(vslam_fe* fe, int nframes, const uint8_t* const* imgs, size_t pitch, int imgs_where,
                                            const void* const* depth, size_t depth_pitch, int depth_type, int depth_where,
                                            float depth_map_factor, float bf, int want_host) {
    if (!fe || nframes < 1 || nframes > fe->B || imgs_where < 0 || imgs_where > VSLAM_IMGS_STAGED ||
        (imgs_where != VSLAM_IMGS_STAGED && (!imgs || pitch < vslam_row_bytes(fe))) || !depth ||
        (depth_type != VSLAM_DEPTH_U16 && depth_type != VSLAM_DEPTH_F32) ||
        (depth_where != VSLAM_IMGS_HOST && depth_where != VSLAM_IMGS_DEVICE && depth_where != VSLAM_IMGS_PINNED) ||
        depth_pitch < (size_t)fe->p.width * (depth_type == VSLAM_DEPTH_F32 ? 4 : 2) || depth_pitch > 0xFFFFFFFFu ||
        (depth_pitch & (depth_type == VSLAM_DEPTH_F32 ? 3 : 1)) || !std::isfinite(depth_map_factor) || !std::isfinite(bf)) {
        g_err = "invalid arguments";
        return VSLAM_ERR_INVALID;
    }
    const size_t esize = depth_type == VSLAM_DEPTH_F32 ? 4 : 2;
    for (int j = 0; j < nframes; j++)
        if (!depth[j] || ((uintptr_t)depth[j] & (esize - 1)) || (imgs_where != VSLAM_IMGS_STAGED && !imgs[j])) {
            g_err = "null or misaligned image";
            return VSLAM_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(fe->p.device));
    RgbdDepthSrc D;
    memset(&D, 0, sizeof(D));
    D.pitch = (uint32_t)depth_pitch;
    D.type = depth_type;
    D.w = fe->p.width;
    D.h = fe->p.height;
    /* the conversion rule of tracking.cpp:1305-1306: every image that is not float is converted, a float image only when the
     * factor is further than 1e-5 from 1 (a float difference, compared as a double) */
    D.scale = (std::fabs((double)(depth_map_factor - 1.0f)) > 1e-5 || depth_type != VSLAM_DEPTH_F32) ? 1 : 0;
    D.factor = depth_map_factor;
    D.bf = bf;
    if (depth_where == VSLAM_IMGS_HOST) { /* pageable: dense rows into pinned staging, which the kernel reads in place */
        const size_t rowb = (size_t)fe->p.width * esize, one = (rowb * fe->p.height + 255) & ~(size_t)255;
        HIPCHK(vslam_stream_wait(fe->stream)); /* the previous pass's gather may still read the staging */
        int rc = fe->h_depth.ensure(one * fe->B);
        if (rc) return rc;
        fe->pool->parallel_for(nframes, [&](int j) {
            uint8_t* hd = fe->h_depth + one * j;
            if (depth_pitch == rowb) memcpy(hd, depth[j], rowb * fe->p.height);
            else
                for (int y = 0; y < fe->p.height; y++) memcpy(hd + (size_t)y * rowb, (const uint8_t*)depth[j] + (size_t)y * depth_pitch, rowb);
        });
        for (int j = 0; j < nframes; j++) D.img[j] = fe->h_depth + one * j;
        D.pitch = (uint32_t)rowb;
    } else
        for (int j = 0; j < nframes; j++) D.img[j] = depth[j];
    /* full batches whose results go to the host: mvuRight | mvDepth behind the extraction's results, one transfer (as the
     * stereo frame entry does it) */
    const bool blk = want_host && nframes == fe->B && fe->res_init_bytes >= (size_t)nframes * fe->cap * 8 &&
                     fe->block_region_owner != VSLAM_REGION_INIT && fe->d_res;
    if (blk) fe->block_region_owner = VSLAM_REGION_STEREO;
    /* the stereo matcher's scratch, row table included although no RGB-D pass reads it: vslam_stereo_points_* carve the
     * buffer again with (stereo_pairs, stereo_capR) and must find it large enough, or they would move it.  Outside any capture. */
    StereoScratch sc;
    int rc = stereo_scratch(fe, nframes, fe->cap, &sc);
    if (rc) return rc;
    fe->stereo_capR = fe->cap;
    rc = vslam_enqueue_extract(fe, nframes, imgs, pitch, imgs_where, 0, 0, blk ? 2 : (want_host != 0));
    if (rc == VSLAM_OK) rc = fe->t_rgbd.arm(fe->profiling);
    if (rc == VSLAM_OK) {
        if (blk) {
            sc.uRight = (float*)(fe->d_res + fe->res_feat_bytes);
            sc.depth = sc.uRight + (size_t)nframes * fe->cap;
        }
        fe->d_stereo_u = sc.uRight;
        fe->d_stereo_depth = sc.depth;
        const vslam_kp* ukps = fe->d_kps; /* ukeypoints_ = keypoints_ without a camera or with k1 == 0 */
        if (fe->has_cam && vslam_fe_slot_ukps(fe, 0, &ukps) != VSLAM_OK) ukps = fe->d_kps;
        fe->t_rgbd.mark(0, fe->stream);
        vk_rgbd_depth(fe->stream, fe->d_kps, ukps, fe->d_counts, fe->cap, nframes, D, sc.uRight, sc.depth);
        fe->t_rgbd.mark(1, fe->stream);
        if (hipGetLastError() != hipSuccess) {
            g_err = "k_rgbd_depth launch failed";
            rc = VSLAM_ERR_HIP;
        }
    }
    if (rc == VSLAM_OK) rc = send_stereo_outputs(fe, nframes, sc.uRight, blk);
    if (rc == VSLAM_OK)
        for (int j = 0; j < nframes; j++) fe->stereo_slotL[j] = j;
    fe->last_rgbd = rc == VSLAM_OK; /* vslam_enqueue_extract cleared it */
    if (rc != VSLAM_OK) hipStreamSynchronize(fe->stream);
    return rc;
}

extern "C" int vslam_frame_rgbd_wait(vslam_fe* fe, vslam_kp* const* kps, uint8_t* const* desc, int cap, int* n,
                                     float* const* u_right, float* const* depth) {
    if (!fe || !fe->last_rgbd || fe->last_nimg < 1) {
        g_err = "no RGB-D pass enqueued";
        return VSLAM_ERR_INVALID;
    }
    int rc = vslam_finish_extract(fe, fe->last_nimg);
    if (rc != VSLAM_OK) return rc;
    if ((rc = fe->t_rgbd.collect())) return rc; /* vslam_fe_set_profiling: the depth gather's own span */
    rc = vslam_deliver(fe, fe->last_nimg, kps, desc, cap, n, nullptr);
    if (rc != VSLAM_OK) return rc;
    deliver_stereo(fe, u_right, depth);
    return VSLAM_OK;
}

/* with vslam_fe_set_profiling on: HIP-event time of k_rgbd_depth alone, summed over the RGB-D passes waited for since */
extern "C" int vslam_fe_get_rgbd_profile(vslam_fe* fe, double* depth_ms, long* passes) {
    if (!fe) return VSLAM_ERR_INVALID;
    fe->t_rgbd.read({depth_ms}, passes);
    return VSLAM_OK;
}

/* ------------------------------------------------------------------ stereo points on the device */
/* the stereo points of every pair, allocated by the first call that hands them out or fills them */
static int stereo_points_alloc(vslam_fe* fe) {
    const int rc = fe->d_x3dw.ensure((size_t)fe->B * fe->cap * 3);
    return rc ? rc : fe->d_mpflags.ensure((size_t)fe->B * fe->cap);
}

extern "C" int vslam_stereo_points_dev_async(vslam_fe* fe, int npairs, const float* Twc, float cx, float cy,
                                             float invfx, float invfy, int observations, int gemm_float) {
    if (!fe || npairs < 1 || npairs > VSLAM_MAX_SBP_JOBS || npairs > fe->stereo_pairs || !Twc) {
        g_err = "invalid arguments (npairs must not exceed the pairs of the last stereo enqueue, <= 16)";
        return VSLAM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(fe->p.device));
    int rc = stereo_points_alloc(fe);
    if (rc) return rc;
    StereoScratch sc;
    if ((rc = stereo_scratch(fe, fe->stereo_pairs, fe->stereo_capR, &sc))) return rc; /* same carving as the enqueue that filled it */
    UnprojJobs U;
    memset(&U, 0, sizeof(U));
    U.cx = cx; U.cy = cy; U.invfx = invfx; U.invfy = invfy;
    U.cap = fe->cap; U.observations = observations; U.gemmFloat = gemm_float;
    for (int j = 0; j < npairs; j++) {
        UnprojJob& J = U.job[j];
        memcpy(J.Twc, Twc + 12 * j, sizeof(J.Twc));
        const int sl = fe->stereo_slotL[j];
        J.kps = fe->d_kps + (size_t)sl * fe->cap;
        J.nPtr = fe->d_counts + sl * 4;
        J.depth = fe->d_stereo_depth + (size_t)j * fe->cap;
        J.x3Dw = fe->d_x3dw + (size_t)j * fe->cap * 3;
        J.flags = fe->d_mpflags + (size_t)j * fe->cap;
    }
    vk_unproject_stereo(fe->stream, U, npairs);
    HIPCHK(hipGetLastError());
    return VSLAM_OK;
}

extern "C" int vslam_stereo_points_buffers(vslam_fe* fe, int pair, const float** dev_x3dw, const uint8_t** dev_flags,
                                           const float** dev_u_right, const float** dev_depth) {
    if (!fe || pair < 0 || pair >= fe->B || pair >= VSLAM_MAX_SBP_JOBS) return VSLAM_ERR_INVALID;
    HIPCHK(hipSetDevice(fe->p.device));
    int rc = stereo_points_alloc(fe);
    if (rc) return rc;
    if (dev_x3dw) *dev_x3dw = fe->d_x3dw + (size_t)pair * fe->cap * 3;
    if (dev_flags) *dev_flags = fe->d_mpflags + (size_t)pair * fe->cap;
    if (dev_u_right || dev_depth) {
        if (fe->stereo_pairs < 1 || pair >= fe->stereo_pairs) {
            g_err = "no stereo result for this pair yet";
            return VSLAM_ERR_INVALID;
        }
        StereoScratch sc;
        if ((rc = stereo_scratch(fe, fe->stereo_pairs, fe->stereo_capR, &sc))) return rc;
        if (dev_u_right) *dev_u_right = fe->d_stereo_u + (size_t)pair * fe->cap;
        if (dev_depth) *dev_depth = fe->d_stereo_depth + (size_t)pair * fe->cap;
    }
    return VSLAM_OK;
}
