/* vslam_host.h -- host-side logic of the front-end that involves no GPU call: constructor tables,
 * resize coefficient tables, the FAST cell list, the sequential quadtree distribution and the
 * order-dependent matcher replays.  Plain C++17; built into libvslam_fe.so (with the kernels) and into
 * libvslam_host.so (g++, no HIP) so the CPU test-suite can exercise it without a GPU.
 * namespace vslam is vslam_host.cpp; the C declarations at the end are grouped by the file that defines them
 * (vslam_match_host.cpp, vslam_camera_host.cpp).  vslam_kfdb_host.cpp and vslam_ftbook.cpp define what include/vslam_fe.h and
 * include/vslam_featuretracker.h declare.
 */
#ifndef VSLAM_HOST_H
#define VSLAM_HOST_H

#include <array>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/vslam_fe.h"

/* EDGE_THRESHOLD-3: the FAST cell grid starts 16 px inside the level (fextractor.cpp:764-767) */
#define VSLAM_FAST_BORDER 16

/* shared between the host files of one library, not exported from it */
#define VSLAM_HOST_INTERNAL __attribute__((visibility("hidden")))

namespace vslam {

/* FExtractor constructor tables (fextractor.cpp:401-461). */
struct ExtractorTables {
    int nlevels = 0;
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> quota; /* mnFeaturesPerLevel */
    int umax[16];
    std::vector<int8_t> disc_u, disc_v; /* flattened radius-15 disc of IC_Angle (fextractor.cpp:75-92) */
};
void build_tables(int nfeatures, float scaleFactor, int nlevels, ExtractorTables& t);

/* level sizes (fextractor.cpp:1139-1140) */
void level_size(const ExtractorTables& t, int w, int h, int level, int* lw, int* lh);

/* cv::resize INTER_LINEAR 8u coefficient tables for one (src -> dst) level pair, in the layout
 * k_resize_level reads: xtab = {sx, min(sx+1, sw-1)} per dx, xa = {alpha0, alpha1}; ytab = clipped
 * {sy, sy+1}, yb = {beta0, beta1}. */
struct ResizeTables {
    std::vector<uint16_t> xtab, ytab;
    std::vector<int16_t> xa, yb;
};
void build_resize_tables(int sw, int sh, int dw, int dh, ResizeTables& r);
/* Quad form of the column table for k_resize_level_v2 (see ResizeQuad in vslam_device.h): qbase[q], and per
 * quad 4 selectors + 4 packed coefficient pairs (8 uint32).  Returns false when some quad's taps do not fit an
 * 8-byte window (scale factor > 2) or the source is narrower than 8 px -- the caller keeps the v1 kernel. */
bool build_resize_quads(const ResizeTables& r, int sw, int dw, std::vector<uint16_t>& qbase,
                        std::vector<uint32_t>& quads);

/* ---- fused pyramid (k_pyramid_group): one workgroup computes a spatial tile of SEVERAL consecutive levels in LDS.
 * Level l is resized from level l-1 (a cascade, fextractor.cpp:1148), so a tile of level l needs a slightly larger
 * tile of level l-1: every (tile, level) gets a COMPUTE range (own range + what the deeper levels of the same tile
 * need, recomputed instead of exchanged between workgroups) and a STORE range (a partition of the level: every
 * pixel of a level is stored by exactly one tile).  Columns are counted in quads (4 output pixels, the unit of
 * k_resize_level_v2's column table). */
struct PyrTileLevel {     /* entry j of a tile: j = 0 is the group's source level (staged from HBM), j >= 1 computed */
    int16_t c0, nc;       /* first column (multiple of 4) and number of columns (multiple of 4) held in LDS */
    int16_t r0, nr;       /* first row, number of rows held in LDS */
    int16_t sq0, sq1;     /* quads stored to HBM: [sq0, sq1) */
    int16_t sr0, sr1;     /* rows stored to HBM: [sr0, sr1) */
    uint32_t lds_off;     /* byte offset of this level's tile in the workgroup's LDS (multiple of 16) */
    uint32_t pitch;       /* LDS row pitch in bytes: nc + 8 (the 8-byte tap window of the last quad may overrun nc)
                             rounded up to a multiple of 16 (rows are staged with 16-byte stores) */
    uint32_t rt_off;      /* j >= 1: byte offset of the level's row table in LDS (nr entries of 8 bytes) */
};
struct PyrGroupPlan {
    int l0 = 0, nl = 0;        /* source level, number of computed levels (l0+1 .. l0+nl) */
    int ntx = 0, nty = 0;      /* tiles per image */
    size_t lds_bytes = 0;      /* dynamic LDS per workgroup */
    std::vector<PyrTileLevel> tiles; /* [ntx*nty][nl+1] */
};
struct PyrLevelTables {   /* tables of destination level l (source l-1), as the per-level kernels use them */
    int sw, sh, dw, dh;
    ResizeTables r;
    std::vector<uint16_t> qbase;
    std::vector<uint32_t> quads;
};
/* Plan for levels l0+1 .. l0+nl (tabs[j-1] = tables of level l0+j).  Returns false if a tile would need more than 64
 * quads per row (lane = quad) or more LDS than max_lds -- the caller then keeps the per-level launches.
 * pingpong = false: every level of the group has LDS of its own.  pingpong = true: two regions, the even entries of a
 * tile (source, level 2, level 4) in the first and the odd ones in the second -- level j is computed from level j-1 alone,
 * so it may overwrite level j-2; the planner checks that a level's tile never touches the one it is computed from. */
bool build_pyramid_group(const std::vector<const PyrLevelTables*>& tabs, int l0, size_t max_lds, PyrGroupPlan& plan,
                         int rows_override = -1 /* vslam_tuning.pyr_rows */, bool pingpong = false);
#ifndef VSLAM_PYR_LDS_KB
#define VSLAM_PYR_LDS_KB 64 /* LDS a pyramid tile's cascade may take with every level resident (32 / 48 / 96 measured) */
#endif
/* LDS of a ping-pong tile, row tables included: what one k_fast_bands workgroup holds (8 of them fill a CU's 160 KB), so a
 * pyramid workgroup fits where a FAST workgroup retired */
#define VSLAM_PYR_PINGPONG_LDS (20 * 1024)
/* The tile shape vslam_fe_create plans with: rows of the first computed level per tile, the LDS layout and its limit, from
 * the frame size, the context's batch and vslam_tuning.pyr_rows / pyr_pingpong (-1: default). */
void pyramid_tile_shape(int width, int height, int batch, int tune_rows, int tune_pingpong, int* rows, bool* pingpong,
                        size_t* max_lds);
/* CPU emulation of k_pyramid_group with the SAME plan and indexing (LDS tiles as arrays); used by the CPU tests to
 * validate a plan before it ever runs on the GPU.  levels[j] = image of level l0+j (j = 0 input, j >= 1 output,
 * pitch = stride[j]).  Returns 0, or a negative code if an access leaves a tile (the GPU would read garbage). */
int emulate_pyramid_group(const PyrGroupPlan& plan, const std::vector<const PyrLevelTables*>& tabs,
                          const uint8_t* src, int sstride, int readable_w, std::vector<uint8_t*>& dst,
                          const std::vector<int>& dstride);

/* FAST cell grid of one level (fextractor.cpp:764-797).  Cells are listed in the reference's visiting
 * order (row-major, skipped cells omitted). */
struct HostCell {
    uint16_t level, x0, y0, x1, y1;
};
void build_cells(int level, int lw, int lh, std::vector<HostCell>& out);

/* Bands of k_fast_bands: up to max_cells CONSECUTIVE cells of one cell row (same level, same y0) whose interiors together
 * are at most max_width px wide; the cells of a row are visited left to right with a constant pitch `wcell` (the last
 * one may be clipped, fextractor.cpp:791-795), so cell k of a band has the interior columns [k * wcell, min((k + 1) * wcell,
 * ww - 6)) of the band's interior.  Bands are listed in cell order (cell0 ascending) and cover every cell exactly once. */
struct HostBand {
    uint32_t cell0;                  /* index of the band's first cell in the cell list */
    uint16_t level, ncell, wcell;
    uint16_t x0, y0, ww, wh;         /* shared window: [x0, x0 + ww) x [y0, y0 + wh) in level coordinates */
};
void build_bands(const std::vector<HostCell>& cells, int max_cells, int max_width, std::vector<HostBand>& out);

/* The band list in the words k_fast_bands reads (BandDesc in vslam_device.h has the same 16 bytes) and its column tables,
 * one 272-byte record per (cell pitch, interior width) class: cellbit[136] = 1 << (cell of interior column x), 0 past the
 * interior; cellfl[136] = bit 0 first / bit 1 last column of its cell. */
struct BandWords {
    uint32_t cell0; /* first cell of the band in the cell list */
    uint32_t lnw;   /* level | ncell << 4 | wcell << 8 | column-table class << 16 */
    uint32_t xy;    /* x0 | y0 << 16 */
    uint32_t wh;    /* window width | height << 16 */
};
struct BandTables {
    std::vector<BandWords> bands;
    std::vector<uint8_t> classes;
    int max_wh = 0, max_iw = 0, max_cells = 0; /* tallest window, widest interior, most cells of a band */
    bool ok = false; /* the words can hold the list: a band exists, level < 16, wcell < 256, class < 65536 */
};
void pack_bands(const std::vector<HostBand>& hb, int nlevels, BandTables& out);

/* Slots of a context's keypoint arrays: nfeatures + 4 * nlevels + 8, or the exact bound of what DistributeOctTree can
 * return if that is more (only for very small nfeatures); a multiple of 4, so packed descriptors stay 16-byte aligned.
 * quota: mnFeaturesPerLevel; lw / lh: level sizes. */
int keypoint_capacity(const int* quota, const int* lw, const int* lh, int nlevels, int nfeatures);

/* Plan of the device quadtree (k_octree_v4): the per-level fields of OctParams (vslam_device.h), the list capacities and the
 * fine grid.  selOff: the level's result list (max(N + 3, 4 * nIni) + 1 entries) in a slot's lists; lut: build_oct_lut of
 * every level at its fineD, x table (lutW entries) then y table, from lutOff. */
struct OctPlan {
    int32_t N[VSLAM_MAX_LEVELS], H[VSLAM_MAX_LEVELS], nIni[VSLAM_MAX_LEVELS], selOff[VSLAM_MAX_LEVELS];
    int32_t fineD[VSLAM_MAX_LEVELS], lutOff[VSLAM_MAX_LEVELS], lutW[VSLAM_MAX_LEVELS];
    float hX[VSLAM_MAX_LEVELS];
    int32_t selStride = 0, maxNodes = 0, fineLdsOff = 0, fineLdsBytes = 0;
    std::vector<uint32_t> lut;
    bool fits = false; /* the device kernel can run this plan; otherwise the quadtree stays on the host */
};
/* cell_first[l]: index of the level's first FAST cell (nlevels + 1 entries); forced_depth: vslam_tuning.oct_fine_depth (-1:
 * by the level's quota); budget: LDS bytes a workgroup should take in all -- it steers the depths, whose floor is 1, while
 * `fits` is judged against the CU's 160 KB and the 150 KB the node arrays may have of it; node_bytes(maxNodes): size of
 * the kernel's node arrays (vk_octree_lds_bytes, which belongs to the kernel file). */
void plan_octree(const int* quota, const int* lw, const int* lh, const int* cell_first, int nlevels, int forced_depth,
                 size_t budget, const std::function<size_t(int)>& node_bytes, OctPlan& P);

/* A FAST candidate / selected keypoint in level coordinates relative to the 16-px border. */
struct Cand {
    int16_t x, y;
    uint8_t response;
};

/* FExtractor::DistributeOctTree (fextractor.cpp:530-754) on integer candidates.
 * W = maxBorderX - minBorderX, H = maxBorderY - minBorderY, N = mnFeaturesPerLevel[level].
 * Result order = the reference's lNodes order (front to back).  Tie-break of equal-size nodes in the
 * "largest first" phase: the node created later is split first (the reference sorts by heap address,
 * which is not reproducible).  Returns false when nIni < 1 (reference UB). */
bool distribute_octree(const Cand* cands, int n, int W, int H, int N, std::vector<Cand>& out);

/* The implicit quadtree under DistributeOctTree's initial nodes (fextractor.cpp:534-561 for the roots, DivideNode
 * :472-517 for the halving): a key's root b = min((int)(x / hX), nIni - 1) and its quadrant at every depth depend on x and y
 * SEPARATELY (midpoints mx = x0 + ceil((x1 - x0) / 2), kp.x < mx; the same in y), so the path to depth D is
 *     path = xs[x] | ys[y],   xs[x] = b << 2D | (x's D decisions on the even bits), ys[y] = (y's on the odd bits),
 * most significant decision first -- two table look-ups instead of D dependent halvings per key (k_octree_v4).
 * W = maxBorderX - minBorderX, H = maxBorderY - minBorderY; xs gets W + 1 entries, ys H + 1.
 * oct_key_path: the same path by walking the halvings, any depth (the kernel uses it below the tables' depth). */
void build_oct_lut(int W, int H, int D, std::vector<uint32_t>& xs, std::vector<uint32_t>& ys);
uint32_t oct_key_path(int x, int y, int W, int H, int depth);

/* Frame::AssignFeaturesToGrid + GetFeaturesInArea (frame.cpp:386-414, 678-756), undistorted image. */
struct FrameGrid {
    static const int COLS = 64, ROWS = 48; /* frame.h:42-43 */
    float minX, maxX, minY, maxY, invW, invH;
    std::vector<int> cell_start; /* COLS*ROWS+1, cells indexed ix*ROWS+iy */
    std::vector<int> cell_items;
    const vslam_kp* kps;
    int n;
    void build(const vslam_kp* k, int n_, int imgW, int imgH); /* bounds {0, imgW, 0, imgH} */
    void build(const vslam_kp* k, int n_, const float bounds[4]); /* minX, maxX, minY, maxY (ComputeImageBounds) */
    /* A KeyFrame's grid: the cells and inverses are the Frame's, made from its float bounds (keyframe.cpp:36, :58-67), while
     * KeyFrame::GetFeaturesInArea (:663-675) places its window from the integer mnMinX / mnMinY the KeyFrame truncated them to */
    VSLAM_HOST_INTERNAL void build_keyframe(const vslam_kp* k, int n_, const float bounds[4]);
    void query(float x, float y, float r, int minLevel, int maxLevel, std::vector<int>& out) const;
};

/* FMatcher::SearchForInitialization (fmatcher.cpp:983-1098) sequential replay over frame 2's grid with the float
 * bounds minX, maxX, minY, maxY (vslam_bounds order).  dist(i1,i2) is read
 * from a dense matrix over the octave-0 keypoints of both frames: row r of `dmat` belongs to l0_1[r],
 * column c to l0_2[c] (map2[i2] = column or -1). */
int search_for_initialization_replay(const vslam_kp* kps1, int n1, const vslam_kp* kps2, int n2,
                                     const uint8_t* dmat, const int* row_of_i1, const int* col_of_i2,
                                     int ncols, const float bounds[4], float* prevMatched, int32_t* matches12,
                                     int windowSize, float nnratio, bool checkOri);

/* The end of every matcher's orientation check: the three fullest bins of the rotation histogram stay
 * (vslam_md::three_maxima / keeps_bin, the kernels' text), the entries of every other bin are returned, bin after bin in the
 * order they were pushed.  The caller clears them by its own rule: SearchForInitialization counts a loser only if it still
 * holds a match (fmatcher.cpp:1082-1086), the other matchers count every one. */
VSLAM_HOST_INTERNAL std::vector<int> rotation_losers(const std::vector<int>* rotHist /* 30 = FMatcher::HISTO_LENGTH bins */);

/* Carving of one staging block (vslam_staging.h): part 0 starts at 0 and part i at the end of part i - 1 rounded up to
 * `align` (a power of two), so a part of no bytes takes no room.  off[0 .. n) receives the starts; returns the rounded
 * end of the last part, the block's size. */
size_t layout_parts(size_t align, const size_t* sizes, int n, size_t* off);
/* the same for a braced list of sizes: {off[0], .., off[N - 1], total}, made for structured bindings */
template <size_t N>
std::array<size_t, N + 1> layout(size_t align, const size_t (&sizes)[N]) {
    std::array<size_t, N + 1> o;
    o[N] = layout_parts(align, sizes, (int)N, o.data());
    return o;
}

} // namespace vslam

/* ---- vslam_host.cpp (its other vslamh_* hooks serve the CPU suite alone, which declares them where it calls them) */
/* layout_parts for the CPU suite (off: n entries); returns the total */
extern "C" uint64_t vslamh_layout(uint64_t align, const uint64_t* sizes, int n, uint64_t* off);

/* ---- vslam_match_host.cpp: the matchers on the host */
/* index map-back and over-capacity decision of vslam_search_local_points_wait */
extern "C" int vslamh_local_points_finish(const int32_t* match_compact, int n_cur, const int32_t* orig_index, int n_kept,
                                          int capacity, int32_t* match_cur);
/* the range check of a rig frame's mvLeftToRightMatch / mvRightToLeftMatch (each entry -1 or an index of the
 * other side), as vslam_search_by_projection_mappoints_rig makes it before anything is enqueued */
extern "C" int vslamh_rig_maps_check(const int32_t* left_to_right, int n_left, const int32_t* right_to_left, int n_right);
/* vslam_two_view_score over host arrays by the shared vslam_two_view.h code (CPU tests, the demo) */
extern "C" int vslamh_two_view_score(const vslam_two_view_job* job, vslam_two_view_result* result);
/* vslam_search_by_projection_frame_rig's intrinsics test (p's fx, fy, cx, cy against the KB8 camera, bit for
 * bit), and the function itself over host arrays, sequential as the reference writes it (CPU tests, the shim's fallback) */
extern "C" int vslamh_frame_rig_camera_check(const vslam_proj_params* p, const vslam_kb8_camera* cam);
extern "C" int vslamh_search_by_projection_frame_rig(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Trl,
                                                     const vslam_kp* last_kps, int n_last, const uint8_t* last_flags,
                                                     const float* last_x3dw, const uint8_t* mp_desc, const vslam_kp* kps_left,
                                                     const uint8_t* desc_left, int n_left, const vslam_kp* kps_right,
                                                     const uint8_t* desc_right, int n_right, const uint8_t* occupied,
                                                     const float* scale_factors, int nlevels, const float* bounds,
                                                     int32_t* match_cur, int* nmatches);
/* SearchByBoW(KeyFrame, Frame) of a rig (fmatcher.cpp:546-748, F.Nleft != -1) over host arrays for one keyframe,
 * sequential as the reference writes it (CPU tests, the shim's fallback beyond the device limits) */
extern "C" int vslamh_search_by_bow_rig(const vslam_kp* kf_kps, const uint8_t* kf_desc_left, int kf_n_left,
                                        const uint8_t* kf_desc_right, int kf_n_right, const uint8_t* kf_flags,
                                        const int32_t* kf_fv_nodes, const int32_t* kf_fv_off, const int32_t* kf_fv_feat,
                                        int n_kf_nodes, const vslam_kp* f_kps_left, const uint8_t* f_desc_left, int n_left,
                                        const vslam_kp* f_kps_right, const uint8_t* f_desc_right, int n_right,
                                        const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat,
                                        int n_f_nodes, float nnratio, int check_orientation, int32_t* match_f, int* nmatches);
/* the search half of Fuse for a fisheye KeyFrame / a rig (vslam_fuse_search_rig) over host arrays, a job's
 * dev_kps / dev_desc included, sequential as the reference writes it; any number of jobs and points (CPU tests, and the shim's
 * walk for the one-point searches of a MapPoint whose descriptor was recomputed) */
extern "C" int vslamh_fuse_search_rig(const vslam_fuse_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                                      const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                      const uint8_t* mp_desc, int n_points, const float* scale_factors, const float* inv_sigma2,
                                      int nlevels, const float* bounds, int32_t* best_idx, int32_t* best_dist);
/* the relocalisation and loop-closing SearchByProjection for fisheye cameras
 * (vslam_search_by_projection_keyframe_kb8, vslam_search_by_projection_sim3_kb8) over host arrays, sequential as the reference
 * writes them; the second takes any number of jobs, points and survivors (CPU tests, the shim's fallback for a refused job) */
extern "C" int vslamh_search_by_projection_keyframe_kb8(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Ow,
                                                        float log_scale_factor, int orb_dist, const vslam_kp* kf_kps, int n_kf,
                                                        const uint8_t* mp_flags, const float* mp_x3dw, const float* mp_min_dist,
                                                        const float* mp_max_dist, const uint8_t* mp_desc, const vslam_kp* cur_kps,
                                                        const uint8_t* cur_desc, int n_cur, const uint8_t* cur_occupied,
                                                        const float* scale_factors, int nlevels, const float* bounds,
                                                        int32_t* match_cur, int* nmatches);
extern "C" int vslamh_search_by_projection_sim3_kb8(const vslam_sim3_kb8_params* p, const vslam_kb8_camera* cam,
                                                    const vslam_sim3_kb8_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                                    const uint8_t* mp_desc, int n_points, const float* scale_factors, int nlevels,
                                                    const float* bounds, int32_t* const* match_kf, int* nmatches, int* n_gated);

/* ---- vslam_camera_host.cpp: the camera models on the host */
/* the decisions around a KB8 camera, as the entry points take them (each returns a VSLAM_* code):
 * _exclusive: setting a KB8 camera beside a pinhole camera with that k1, or a pinhole camera with that k1 beside a KB8 camera
 * (other_set: the other kind is set); _frustum_check: the frustum parameters against the camera (NULL: pinhole, nothing to check); _projecting_entry:
 * an entry point that projects with intrinsics of its own */
extern "C" int vslamh_kb8_exclusive(int other_set, float k1);
extern "C" int vslamh_kb8_frustum_check(const vslam_frustum_params* p, const vslam_kb8_camera* cam);
extern "C" int vslamh_kb8_projecting_entry(int has_kb8);
#endif
