/* vslam_featuretracker.h -- C ABI of the pyramidal Lucas-Kanade feature tracker, vilib::FeatureTrackerGPU.
 *
 * Replaces, on MI355X (gfx950), vilib::FeatureTrackerGPU over vilib::FeatureTrackerBase
 *   thirdparty/vilib/visual_lib/include/vilib/feature_tracker/feature_tracker_gpu.h, feature_tracker_options.h
 *   thirdparty/vilib/visual_lib/src/feature_tracker/feature_tracker_gpu.cpp, feature_tracker_base.cpp,
 *   feature_tracker_cuda_tools.cu
 * the one consumer of the grid detectors (vslam_fastgrid.h, vslam_harrisgrid.h).  Each call, vslam_ft_track_bundle takes
 * one frame per camera of a FrameBundle, builds their half-sampled pyramids once, runs the inverse-compositional
 * Lucas-Kanade tracker over them for every live track of every camera, drops the tracks that did not converge, calls the
 * bound detector on the same pyramids for the cameras where too few are left (cells that hold a surviving track stay
 * empty-handed) and precomputes the new tracks' templates and inverse Hessians.  Every step is enqueued once for the whole
 * bundle; vslam_ft_create / vslam_ft_track are the bundle of one camera.
 * Every float operation is rounded on its own, in the order in which the reference's source text reads; DESIGN.md
 * section 8 lists what the reference leaves undefined and what is chosen (lane order of the two reductions, saturating
 * float-to-int conversion, IEEE division, best-N ties by cell index, track ids from 0 per tracker).
 * The cameras of an object share one detector object -- and with it one image size, one grid and one stream -- and one
 * vslam_ft_params; 1 <= cameras <= the detector's max_batch (<= 64).  A rig whose cameras differ in image size is
 * several trackers.  A camera shares nothing else with its neighbours but the track-id counter, so a bundle serves C
 * independent sequences as well as the C cameras of a rig.
 * Error codes and vslam_last_error() are those of vslam_fe.h.
 */
#ifndef VSLAM_FEATURETRACKER_H
#define VSLAM_FEATURETRACKER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_FT_MAX_LEVELS 8
#define VSLAM_FT_MAX_ITER 30 /* FEATURE_TRACKER_MAX_ITERATION_COUNT (feature_tracker/config.h), compile-time there too */
#define VSLAM_FT_DETECTOR_FAST 0   /* the handle is a vslam_fg* */
#define VSLAM_FT_DETECTOR_HARRIS 1 /* the handle is a vslam_hg* */

/* vilib::FeatureTrackerOptions (feature_tracker_options.h:50-98) field for field, then vilib::Frame's n_pyr_levels. */
typedef struct vslam_ft_params {
    int32_t klt_min_level, klt_max_level;             /* levels klt_max_level .. klt_min_level are optimised, coarsest first */
    int32_t klt_patch_sizes[VSLAM_FT_MAX_LEVELS];     /* per level: 8, 16 or 32 */
    float klt_min_update_squared;
    int32_t min_tracks_to_detect_new_features;
    int32_t reset_before_detection;
    int32_t use_best_n_features;                      /* -1: every detected feature */
    int32_t klt_template_is_first_observation;
    int32_t affine_est_offset, affine_est_gain;
    int32_t pyramid_levels;                           /* >= klt_max_level + 1 and >= the detector's max_level; <= 8 */
} vslam_ft_params;

typedef struct vslam_ft vslam_ft;
typedef struct vslam_ftbook vslam_ftbook;

/* One feature of the current frame, in addFeature order (feature_tracker_base.cpp:91-98): px, score, level, track id */
typedef struct vslam_ft_feature {
    float x, y, score;
    int32_t level, track_id;
} vslam_ft_feature;
/* One live track (feature_tracker_base.h:69-112) */
typedef struct vslam_ft_track_info {
    float first_pos[2], cur_pos[2], cur_disparity;
    int32_t life, track_id, buffer_id;
} vslam_ft_track_info;

/* FeatureTrackerGPU(options, 1) + setDetectorGPU(detector, 0).  The tracker works on the detector's stream and image
 * size and must be destroyed before it.  VSLAM_ERR_INVALID: level counts, patch sizes, or an image size that is no
 * multiple of 2^(pyramid_levels-1) (pyramid_pool.cpp:58-59). */
int vslam_ft_create(const vslam_ft_params* p, int detector_kind, void* detector, vslam_ft** out);
/* FeatureTrackerGPU(options, n_cameras) + setDetectorGPU(detector, c) for every camera c.  VSLAM_ERR_INVALID also for
 * n_cameras < 1 and n_cameras above the detector's max_batch.  vslam_ft_create is n_cameras = 1. */
int vslam_ft_create_bundle(const vslam_ft_params* p, int detector_kind, void* detector, int n_cameras, vslam_ft** out);
int vslam_ft_cameras(const vslam_ft* ft);
void vslam_ft_destroy(vslam_ft* ft);
/* max_ftr_count_ (feature_tracker_gpu.cpp:404-411), per camera */
int vslam_ft_capacity(const vslam_ft* ft);

/* FeatureTrackerGPU::track for one frame (feature_tracker_gpu.cpp:85-288).  img: host memory, or device memory when
 * on_device != 0. */
int vslam_ft_track(vslam_ft* ft, const uint8_t* img, size_t pitch, int on_device, int32_t* n_tracked, int32_t* n_detected);
/* FeatureTrackerGPU::track for a FrameBundle: imgs[c] is camera c's frame, all of one pitch and all in host or all in
 * device memory; n_tracked[c], n_detected[c] (arrays of vslam_ft_cameras, or NULL) are camera c's counts, their sums
 * the reference's two totals.  Within a call new track ids go to camera 0's new tracks first, then camera 1's, ...
 * vslam_ft_track is this for an object of one camera and VSLAM_ERR_INVALID for any other. */
int vslam_ft_track_bundle(vslam_ft* ft, const uint8_t* const* imgs, size_t pitch, int on_device, int32_t* n_tracked,
                          int32_t* n_detected);

/* Read side.  The lists are copied up to `cap` entries; *n is how many there are.  The forms without a camera read
 * camera 0; a camera outside [0, vslam_ft_cameras) is VSLAM_ERR_INVALID. */
int vslam_ft_features(const vslam_ft* ft, vslam_ft_feature* out, int cap, int* n);
int vslam_ft_features_cam(const vslam_ft* ft, int camera, vslam_ft_feature* out, int cap, int* n);
int vslam_ft_tracks(const vslam_ft* ft, vslam_ft_track_info* out, int cap, int* n);
int vslam_ft_tracks_cam(const vslam_ft* ft, int camera, vslam_ft_track_info* out, int cap, int* n);
/* FeatureTrackerBase::getDisparity (feature_tracker_base.cpp:137-171) over one camera's tracks */
int vslam_ft_disparity(const vslam_ft* ft, double pivot_ratio, double* out);
int vslam_ft_disparity_cam(const vslam_ft* ft, int camera, double pivot_ratio, double* out);
/* The next three apply to every camera of the object, as the options they change are shared in the reference. */
int vslam_ft_reset(vslam_ft* ft);                /* FeatureTrackerGPU::reset */
int vslam_ft_set_best_n(vslam_ft* ft, int n);    /* setBestNFeatures; the buffers keep the capacity they were created with */
int vslam_ft_set_min_tracks(vslam_ft* ft, int n); /* setMinTracksToDetect */
/* Diagnostic: the template of live track `track` (index into the track list) on pyramid level `level`: the
 * (ps+2) x (ps+2) int32 patch and the 10 words of the inverse Hessian as they lie in device memory.  Where the patch
 * did not fit the level, invH[0] is the word 0x7fffffff and the rest is what the buffer held before. */
int vslam_ft_template_copy(vslam_ft* ft, int track, int level, int32_t* patch, float* invH);
int vslam_ft_template_copy_cam(vslam_ft* ft, int camera, int track, int level, int32_t* patch, float* invH);

/* Diagnostic for tests/tools/time_featuretracker*.py: with enable != 0, a track call brackets its two kernels with HIP
 * events; vslam_ft_kernel_ms then waits for them and returns the last call's k_ft_track and k_ft_update times in
 * milliseconds (0 where the kernel did not run).  A bundle has one launch of each for all its cameras. */
int vslam_ft_profile(vslam_ft* ft, int enable);
int vslam_ft_kernel_ms(vslam_ft* ft, float* track_ms, float* update_ms);

/* The bookkeeping alone -- track list, buffer-id LIFO, feature list, occupancy, best-N selection -- as vslam_ft_track
 * runs it around the kernels; no GPU call.  Also in libvslam_host.so.  Return values: 0, or -1 for invalid arguments. */
int vslam_ftbook_create(const vslam_ft_params* p, int n_cols, int n_rows, int cell_w, int cell_h, vslam_ftbook** out);
void vslam_ftbook_destroy(vslam_ftbook* b);
int vslam_ftbook_capacity(const vslam_ftbook* b);
/* step 02: res[4*i] = (x, y, disparity, unused) of track i; a NaN x ends the track */
int vslam_ftbook_results(vslam_ftbook* b, const float* res, int n);
int vslam_ftbook_need_detect(const vslam_ftbook* b);
/* step 03 on a detector's grid; the tracks it adds are the last *n_detected of the list */
int vslam_ftbook_detect(vslam_ftbook* b, const float* pos, const float* score, const int32_t* level, int* n_detected);
int vslam_ftbook_update_count(const vslam_ftbook* b); /* step 04: how many tracks at the end of the list get templates */
int vslam_ftbook_features(const vslam_ftbook* b, vslam_ft_feature* out, int cap, int* n);
int vslam_ftbook_tracks(const vslam_ftbook* b, vslam_ft_track_info* out, int cap, int* n);
int vslam_ftbook_disparity(const vslam_ftbook* b, double pivot_ratio, double* out);
int vslam_ftbook_reset(vslam_ftbook* b);
int vslam_ftbook_set_best_n(vslam_ftbook* b, int n);
int vslam_ftbook_set_min_tracks(vslam_ftbook* b, int n);
/* The id the next new track gets (from 0).  A tracker over several cameras keeps one counter, as Point::getNewId is one:
 * it sets it before a camera's step 03 and reads it back afterwards.  vslam_ftbook_next_id: -1 for a null book. */
int vslam_ftbook_next_id(const vslam_ftbook* b);
int vslam_ftbook_set_next_id(vslam_ftbook* b, int id);

#ifdef __cplusplus
}
#endif
#endif
