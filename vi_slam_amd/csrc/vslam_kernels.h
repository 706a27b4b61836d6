/* vslam_kernels.h -- launch wrappers implemented in the kernel files (vslam_image_kernels.hip, vslam_kernels.hip,
 * vslam_octree_kernel.hip, vslam_match_kernels.hip, vslam_init_kernel.hip, vslam_projection_kernels.hip).  T: the context's resolved switches
 * (vslam_tuning.h); the launchers read their A/B knobs from it, never from the environment. */
#ifndef VSLAM_KERNELS_H
#define VSLAM_KERNELS_H

#include "vslam_tuning.h"
#include "vslam_device.h"

void vk_upload_disc(const int umax[16]); /* IC_Angle disc -> packed dword weights of the descriptor kernel */

void vk_resize_level(hipStream_t st, uint8_t* pyr, size_t slot_stride, const BatchSrc& src,
                     const LevelGeom& sg, const LevelGeom& dg, int src_level, const uint16_t* xtab,
                     const int16_t* xa, const uint16_t* ytab, const int16_t* yb, int nslots);

void vk_hamming_matrix(hipStream_t st, const uint8_t* q, int nq, const uint8_t* t, int nt, uint8_t* out);
/* nprob problems in one launch: part holds nrows * nsplit * 2 words (nrows = queries of all problems back to back,
 * Top2Job::row0), idx2 / dist2 nrows * 2; nsplit from vk_hamming_top2_batch_split */
int vk_hamming_top2_batch_split(int nprob, int max_nq, int max_nt);
void vk_hamming_top2_batch(hipStream_t st, const Top2Jobs& jobs, int nprob, int max_nq, int nrows, int nsplit, uint32_t* part,
                           int32_t* idx2, int32_t* dist2);

void vk_blur7_v2(hipStream_t st, const uint8_t* pyr, size_t slot_stride, const BatchSrc& src, const PyramidGeom& g,
                 uint8_t* blur, const uint32_t* tasks, int ntasks, const int32_t taps[7], int rows_per_task,
                 int nslots);
void vk_pyramid_group(hipStream_t st, uint8_t* pyr, size_t slot_stride, const BatchSrc& src, const PyrGroupDev& G,
                      size_t lds_bytes, bool fit /* a ping-pong plan: the kernel that sits where a FAST workgroup sat */, int nslots,
                      uint8_t* reset_cand = nullptr, size_t cand_stride = 0,
                      int32_t* reset_err = nullptr);
void vk_fast_cells_v3(hipStream_t st, const uint8_t* pyr, size_t slot_stride, const BatchSrc& src,
                      const PyramidGeom& g, const CellDesc* cells, int ncells, uint8_t* cand_region,
                      size_t cand_stride, int iniTh, int minTh, int tile_rows, int max_window_w, int max_px, int nslots);
/* k_fast_bands: one workgroup per band of cells (vslam::build_bands); max_wh = tallest band window.  _check: the
 * kernel's limits (0 = a band list it can run) */
int vk_fast_bands_check(int max_wh, int max_iw, int max_cells_per_band);
void vk_fast_bands(hipStream_t st, const uint8_t* pyr, size_t slot_stride, const BatchSrc& src, const PyramidGeom& g,
                   const BandDesc* bands, int nbands, const uint8_t* classes, const CellDesc* cells, int ncells, uint8_t* cand_region,
                   size_t cand_stride, int iniTh, int minTh, int max_wh, int max_iw, int nslots);
void vk_resize_level_v2(hipStream_t st, uint8_t* pyr, size_t slot_stride, const BatchSrc& src, const LevelGeom& sg,
                        const LevelGeom& dg, int src_level, const uint16_t* qbase, const ResizeQuad* quads,
                        const uint16_t* ytab, const int16_t* yb, int nslots);
size_t vk_octree_lds_bytes(int maxNodes);
int vk_octree_set_max_lds(size_t bytes);
void vk_octree(hipStream_t st, const uint8_t* cand_region, size_t cand_stride, int ncells, const OctParams& P,
               uint32_t* keys_a, void* sorted_a, size_t pts_stride,
               uint32_t* sel_xyr, int32_t* sel_cnt, int32_t* err_flag, int nlevels, int nslots, int32_t* deep_flags,
               int regkeys, int threads = 1024);
void vk_assign_out(hipStream_t st, const OctParams& P, const PyramidGeom& g, uint32_t* sel_xyr, int32_t* sel_cnt, int lap0,
                   int lap1, SelKp* sel, int32_t* slot_counts, int cap, int32_t* err_flag, int nslots,
                   const int32_t* deep_flags);
void vk_orient_describe_dev(hipStream_t st, const uint8_t* pyr, const uint8_t* blur, size_t slot_stride,
                            const BatchSrc& src, const PyramidGeom& g, const SelKp* sel,
                            const int32_t* slot_counts, const int8_t* pattern, vslam_kp* kps, uint8_t* desc,
                            int cap, int atan_fma, int nslots, int kpw_override = -1);

void vk_dbg_sincos(hipStream_t st, const float* x, int n, float* s, float* c);
void vk_dbg_logf(hipStream_t st, const float* x, int n, float* y);
void vk_dbg_atan2(hipStream_t st, const float* y, const float* x, int n, int fma, float* a);

void vk_stereo(hipStream_t st, const StereoJobs& jobs, int njobs, int maxNL, int maxNR, const PyramidGeom& g,
               const uint8_t* pyrL, size_t strideL, const BatchSrc& srcL, const uint8_t* pyrR, size_t strideR,
               const BatchSrc& srcR, float mbf, float maxD, uint32_t* best, float* uRight, float* depth,
               int32_t* sad, int cap, int max_band, uint8_t* rows_scratch);
/* bytes of rows_scratch: row table, bucket items and {uR, octave} records of njobs stereo pairs */
size_t vk_stereo_rows_bytes(int njobs, int nrows, int max_band, int cap);
void vk_hamming_matrix_batch(hipStream_t st, const MatJobs& jobs, int njobs, int maxr, int maxc, const int32_t* idx,
                             uint8_t* tmp, uint8_t* out);
size_t vk_search_init_lds(int cap, int max_c2);
size_t vk_search_init_scratch_bytes(int npairs, int max_c2, int M);
int vk_search_init_set_max_lds(size_t bytes);
/* k_si_topm + k_si_replay; scratch = vk_search_init_scratch_bytes(); fallbacks (nullable) counts full re-scans */
void vk_search_init(hipStream_t st, const InitJobs& jobs, int npairs, int cap, const SiBounds& bounds, int window,
                    float nnratio, int checkOri, int32_t* matches_out, float* prev_out, int32_t* nmatch_out,
                    int max_c2, int M, uint8_t* scratch, int* fallbacks, const vslam_tuning& T);
/* FMatcher::SearchByProjection(CurrentFrame, LastFrame): k_sbp_rank + k_sbp_replay over up to
 * VSLAM_MAX_SBP_JOBS problems; maxLast / maxCur size the grid and the LDS (capacities) */
size_t vk_sbp_rank_lds(int nCur);
size_t vk_sbp_replay_lds(int nCur, int nLast);
size_t vk_sbp_scratch_bytes(int nLast, int M);
size_t vk_sbp_proj_bytes(int nLast);
int vk_sbp_set_max_lds(size_t bytes);
struct RigResolveDev;
/* the rig form of SearchByProjection(F, vpMapPoints): k_sbp_rank over JS.job[0] (left) and JS.job[1] (right) in one launch, then
 * k_rig_resolve; maxMp sizes the grid (capacity of the MapPoint list); `between` (may be null) is recorded between the two */
size_t vk_rig_resolve_lds(int nSlots);
void vk_search_rig(hipStream_t st, const SbpJobs& JS, const RigResolveDev& A, int maxMp, hipEvent_t between = nullptr);
struct RigFrameDev;
/* the rig form of SearchByProjection(CurrentFrame, LastFrame): k_sbp_rank_rig over JS.job[0] (left) and JS.job[1] (right) in one
 * launch, then k_sbp_rig_resolve and k_sbp_rig_replay; nLast sizes the grid; `between` (may be null) is recorded behind the ranking */
size_t vk_sbp_rig_resolve_lds(int nSlots);
size_t vk_sbp_rig_replay_lds(int nSlots, int nLast);
void vk_search_frame_rig(hipStream_t st, const SbpJobs& JS, const RigFrameDev& R, int nLast, hipEvent_t between = nullptr);
void vk_search_by_projection(hipStream_t st, const SbpJobs& JS, int njobs, int maxLast, int maxCur, int* fallbacks,
                             int forceSeq);
/* the same behind k_sbp_rank_kb8: modes 2 and 3 of a fisheye frame / KeyFrame; `between` (may be null) is recorded behind the
 * ranking */
void vk_search_by_projection_kb8(hipStream_t st, const SbpJobs& JS, int njobs, int maxLast, int maxCur, int* fallbacks,
                                 int forceSeq, const vslam_kb8_camera& cam, hipEvent_t between = nullptr);
/* SearchByProjection(pKF, Scw, ..) for fisheye KeyFrames: k_s3k_gate, k_s3k_compact, then the above over every job's
 * survivors (A.cap sizes the ranking grid, maxKF the LDS), then k_s3k_finish; the events (may be null) are recorded behind the
 * compaction and behind the ranking */
struct Sim3Kb8Args;
void vk_search_sim3_kb8(hipStream_t st, const Sim3Kb8Args& A, const SbpJobs& JS, int njobs, int maxKF, int* fallbacks,
                        int forceSeq, hipEvent_t after_compact = nullptr, hipEvent_t after_rank = nullptr);
int vk_distinctive_set_max_lds(size_t bytes);
void vk_distinctive(hipStream_t st, const uint8_t* desc, const int32_t* offsets, int nsets, int maxN, int32_t* best);
void vk_unproject_stereo(hipStream_t st, const UnprojJobs& U, int njobs);
void vk_fuse_search(hipStream_t st, const FuseArgsDev& A);
/* k_fuse_rank_rig: A.nPoints MapPoints against A.job[0 .. njobs); maxKF (the largest job's keypoint count) sizes the LDS */
void vk_fuse_search_rig(hipStream_t st, const FuseRigArgs& A, int njobs, int maxKF);
void vk_reset_headers(hipStream_t st, uint8_t* d_cand, size_t cand_stride_bytes, int nimg, int32_t* d_err);
/* device -> pinned host (or device) range copies / zero fills in one launch; see k_copy_ranges */
/* returns the number of copy operations put on the stream (runtime copies or one kernel launch) */
int vk_copy_ranges(hipStream_t st, const CopyRanges& R, const vslam_tuning& T = vslam_process_tuning());
/* cv::undistortPoints of every keypoint of slots 0..nimg-1 (counts[s*4] keypoints each, cap apart): full vslam_kp copies
 * with x, y replaced (vslam_undistort.hip) */
void vk_undistort_kps(hipStream_t st, const vslam_kp* kps, const int32_t* counts, vslam_kp* ukps, int cap, int nimg,
                      const UdCam& cam);
/* the same arithmetic on n loose points (x, y interleaved) */
void vk_undistort_xy(hipStream_t st, const float* xy, int n, float* out, const UdCam& cam);
/* host (pinned) images -> level 0 of the slots, one launch; src.l0 / src.pitch0 describe the host rows */
void vk_pull_images(hipStream_t st, const BatchSrc& src, uint8_t* pyr, size_t slot_stride, uint32_t off0, int dpitch,
                    int w, int h, int nimg, int from_host, const vslam_tuning& T);
/* interleaved colour rows (fmt = VSLAM_PIX_*, not GRAY8; shift 14 | 15) -> gray level 0 of the slots, in vk_pull_images' place */
void vk_gray_images(hipStream_t st, const BatchSrc& src, uint8_t* pyr, size_t slot_stride, uint32_t off0, int dpitch, int w,
                    int h, int nimg, int from_host, int fmt, int shift, const vslam_tuning& T);
/* Frame::ComputeStereoFromRGBD for every keypoint of slots 0..nimg-1: u_right / depth are nimg x cap floats */
void vk_rgbd_depth(hipStream_t st, const vslam_kp* kps, const vslam_kp* ukps, const int32_t* counts, int cap, int nimg,
                   const RgbdDepthSrc& D, float* u_right, float* depth);
/* Frame::isInFrustum over a local map, and the ordered compaction of the points that go on to the matcher (vslam_frustum.hip) */
struct FrustumArgsDev;
struct FrustumCompactDev;
void vk_frustum(hipStream_t st, const FrustumArgsDev& A);
void vk_frustum_compact(hipStream_t st, const FrustumCompactDev& A);
struct FrustumRigCompactDev;
void vk_rig_compact(hipStream_t st, const FrustumRigCompactDev& A);
/* the same records with KannalaBrandt8::project, and isInFrustumChecks for both cameras of a fisheye rig (vslam_kb8.hip) */
struct FrustumRigDev;
void vk_frustum_kb8(hipStream_t st, const FrustumArgsDev& A, const vslam_kb8_camera& cam);
void vk_frustum_rig(hipStream_t st, const FrustumRigDev& A);
/* the pair list, every hypothesis' score and flags, the selection (vslam_two_view.hip): njobs TvJobDev in HBM, max_groups =
 * the most 64-hypothesis groups (H and F together) of any job, ev = four events around the three launches or NULL */
struct TvJobDev;
void vk_two_view(hipStream_t st, const TvJobDev* jobs, int njobs, int max_groups, hipEvent_t* ev);
void vk_pack_slots(hipStream_t st, const vslam_kp* kps, const uint8_t* desc, const int32_t* counts, int cap, int first,
                   int nslots, uint8_t* dst, size_t slot_bytes);
void vk_gather_rows32(hipStream_t st, const uint8_t* src, const int32_t* idx, int n, uint8_t* dst);

#endif
