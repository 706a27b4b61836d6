/* vslam_shim.hpp -- header-only C++ face of libvslam_fe.so with the reference's class names and signatures.
 *
 * What a maintainer of KMS-TEAM/vi_slam includes instead of (the bodies of)
 *   include/vi_slam/geometry/fextractor.h:26-91   -> FExtractor
 *   include/vi_slam/geometry/fmatcher.h:70-147    -> FMatcher (hot-path subset + the two pinhole SearchByProjection
 *                                                     overloads used by tracking)
 *   src/datastructures/frame.cpp:823-997          -> ComputeStereoMatches
 * Everything forwards to the C ABI in vslam_fe.h; nothing is computed here.
 *
 * cv:: types: with -DVSLAM_SHIM_WITH_OPENCV the signatures take cv::Mat / cv::KeyPoint / cv::Point2f exactly as
 * the reference does.  Without OpenCV (this repository's test build) POD stand-ins with the same layout are
 * used: KeyPoint == cv::KeyPoint (28 bytes), Point2f == cv::Point2f, Mat8u == a CV_8UC1 cv::Mat
 * (rows, cols, step, data).
 *
 * Error behaviour follows the reference where it has one (compute() returns -1 on an empty image,
 * fextractor.cpp:1037-1038); failures of the library surface as std::runtime_error(vslam_last_error()).
 */
#ifndef VSLAM_SHIM_HPP
#define VSLAM_SHIM_HPP

#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <memory>
#include <vector>

#include "vslam_fe.h"
#include "vslam_fastgrid.h"
#include "vslam_harrisgrid.h"
#include "vslam_featuretracker.h"

#ifdef VSLAM_SHIM_WITH_OPENCV
#include <opencv2/core/core.hpp>
#endif

#ifndef VSLAM_SHIM_NAMESPACE
#define VSLAM_SHIM_NAMESPACE vi_slam_amd
#endif

/* libvslam_fe.so, the host side (declared in vi_slam_amd/csrc/vslam_host.h, defined in vslam_match_host.cpp):
 * SearchByProjection(CurrentFrame, LastFrame) of a two-fisheye rig as the reference's sequential loop over host arrays -- what
 * FMatcher::SearchByProjection(RigFrameView, ..) falls back on beyond the device's limits */
extern "C" int vslamh_search_by_projection_frame_rig(const vslam_proj_params* p, const vslam_kb8_camera* cam, const float* Trl,
                                                     const vslam_kp* last_kps, int n_last, const uint8_t* last_flags,
                                                     const float* last_x3dw, const uint8_t* mp_desc, const vslam_kp* kps_left,
                                                     const uint8_t* desc_left, int n_left, const vslam_kp* kps_right,
                                                     const uint8_t* desc_right, int n_right, const uint8_t* occupied,
                                                     const float* scale_factors, int nlevels, const float* bounds,
                                                     int32_t* match_cur, int* nmatches);

/* the same for SearchByBoW(KeyFrame, Frame) of a rig, one keyframe: FMatcher::SearchByBoW(.., RigFrameView, ..)'s fallback */
extern "C" int vslamh_search_by_bow_rig(const vslam_kp* kf_kps, const uint8_t* kf_desc_left, int kf_n_left,
                                        const uint8_t* kf_desc_right, int kf_n_right, const uint8_t* kf_flags,
                                        const int32_t* kf_fv_nodes, const int32_t* kf_fv_off, const int32_t* kf_fv_feat,
                                        int n_kf_nodes, const vslam_kp* f_kps_left, const uint8_t* f_desc_left, int n_left,
                                        const vslam_kp* f_kps_right, const uint8_t* f_desc_right, int n_right,
                                        const int32_t* f_fv_nodes, const int32_t* f_fv_off, const int32_t* f_fv_feat,
                                        int n_f_nodes, float nnratio, int check_orientation, int32_t* match_f, int* nmatches);

/* the search half of Fuse for a fisheye KeyFrame / a rig over host arrays (a job's dev_kps / dev_desc are HOST pointers here):
 * the one-point searches that FMatcher::FuseWalk's caller redoes for a MapPoint whose descriptor was recomputed */
extern "C" int vslamh_fuse_search_rig(const vslam_fuse_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                                      const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                      const uint8_t* mp_desc, int n_points, const float* scale_factors, const float* inv_sigma2,
                                      int nlevels, const float* bounds, int32_t* best_idx, int32_t* best_dist);

/* the loop-closing SearchByProjection for fisheye KeyFrames over host arrays (a job's dev_kps / dev_desc are HOST pointers here):
 * what FMatcher::FindMatchesByProjectionKB8 runs for a job whose survivors exceed the device's 4096 */
extern "C" int vslamh_search_by_projection_sim3_kb8(const vslam_sim3_kb8_params* p, const vslam_kb8_camera* cam,
                                                    const vslam_sim3_kb8_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                                    const uint8_t* mp_desc, int n_points, const float* scale_factors, int nlevels,
                                                    const float* bounds, int32_t* const* match_kf, int* nmatches, int* n_gated);

namespace VSLAM_SHIM_NAMESPACE {
namespace geometry {

#ifdef VSLAM_SHIM_WITH_OPENCV
typedef cv::KeyPoint KeyPoint;
typedef cv::Point2f Point2f;
#else
struct Point2f {
    float x, y;
};
struct KeyPoint { /* field order of cv::KeyPoint */
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};
/* CV_8UC1 (or, for colour input, CV_8UC3 / CV_8UC4) matrix stand-in: non-owning view or owning buffer */
struct Mat8u {
    int rows = 0, cols = 0;
    size_t step = 0;
    uint8_t* data = nullptr;
    std::vector<uint8_t> own;
    int nchannels = 1;
    Mat8u() {}
    Mat8u(int r, int c, uint8_t* d, size_t s, int ch = 1) : rows(r), cols(c), step(s), data(d), nchannels(ch) {}
    void create(int r, int c, int ch = 1) {
        rows = r;
        cols = c;
        nchannels = ch;
        step = (size_t)c * ch;
        own.assign((size_t)r * c * ch, 0);
        data = own.data();
    }
    int channels() const { return nchannels; }
    void release() {
        rows = cols = 0;
        step = 0;
        own.clear();
        data = nullptr;
    }
    bool empty() const { return !data || rows == 0 || cols == 0; }
    uint8_t* ptr(int r) { return data + (size_t)r * step; }
    const uint8_t* ptr(int r) const { return data + (size_t)r * step; }
};
#endif
static_assert(sizeof(KeyPoint) == sizeof(vslam_kp), "KeyPoint must be layout-compatible with vslam_kp");
static_assert(sizeof(Point2f) == 8, "Point2f is two packed floats");

inline void check(int rc) {
    if (rc != VSLAM_OK) throw std::runtime_error(std::string("libvslam_fe: ") + vslam_last_error());
}

/* ---------------------------------------------------------------------------------------------------
 * FExtractor (fextractor.h:26-91).  The image size becomes known at the first compute(), as in the
 * reference (mvImagePyramid is sized there, fextractor.cpp:1135-1160); the device context is created then
 * and re-created if the size changes.  One instance per concurrent stream, like the reference
 * (tracking.cpp:1087-1093 allocates Left / Right / Ini extractors).
 * ------------------------------------------------------------------------------------------------- */
class FExtractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    FExtractor(int nfeatures_, float scaleFactor_, int nlevels_, int iniThFAST_, int minThFAST_, int device_ = 0,
               int max_batch_ = 1)
        : nfeatures(nfeatures_), scaleFactor(scaleFactor_), nlevels(nlevels_), iniThFAST(iniThFAST_),
          minThFAST(minThFAST_), device(device_), max_batch(max_batch_) {
        /* scale tables exactly as fextractor.cpp:406-422 (float products, scaleFactor held as double) */
        mvScaleFactor.resize(nlevels);
        mvLevelSigma2.resize(nlevels);
        mvScaleFactor[0] = 1.0f;
        mvLevelSigma2[0] = 1.0f;
        for (int i = 1; i < nlevels; i++) {
            mvScaleFactor[i] = (float)(mvScaleFactor[i - 1] * scaleFactor);
            mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i];
        }
        mvInvScaleFactor.resize(nlevels);
        mvInvLevelSigma2.resize(nlevels);
        for (int i = 0; i < nlevels; i++) {
            mvInvScaleFactor[i] = 1.0f / mvScaleFactor[i];
            mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i];
        }
    }
    ~FExtractor() {
        if (fe_) vslam_fe_destroy(fe_);
    }
    FExtractor(const FExtractor&) = delete;
    FExtractor& operator=(const FExtractor&) = delete;

#ifdef VSLAM_SHIM_WITH_OPENCV
    int compute(cv::InputArray image, cv::InputArray /*mask*/, std::vector<cv::KeyPoint>& keypoints,
                cv::OutputArray descriptors, std::vector<int>& vLappingArea) {
        if (image.empty()) return -1;
        cv::Mat im = image.getMat();
        CV_Assert(im.depth() == CV_8U);
        std::vector<uint8_t> d;
        int n = 0;
        const int mono = run(im.data, im.cols, im.rows, im.step, im.channels(), keypoints, d, vLappingArea, &n);
        if (n == 0) descriptors.release();
        else cv::Mat(n, 32, CV_8U, d.data()).copyTo(descriptors);
        return mono;
    }
#else
    /* mask is ignored, as in the reference ("Mask is ignored in the current implementation") */
    int compute(const Mat8u& image, const Mat8u& /*mask*/, std::vector<KeyPoint>& keypoints, Mat8u& descriptors,
                std::vector<int>& vLappingArea) {
        if (image.empty()) return -1; /* fextractor.cpp:1037-1038 */
        std::vector<uint8_t> d;
        int n = 0;
        const int mono = run(image.data, image.cols, image.rows, image.step, image.channels(), keypoints, d, vLappingArea, &n);
        if (n == 0) descriptors.release();
        else {
            descriptors.create(n, 32);
            std::memcpy(descriptors.data, d.data(), (size_t)n * 32);
        }
        return mono;
    }
#endif

    int GetLevels() { return nlevels; }
    float GetScaleFactor() { return (float)scaleFactor; }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    /* mvImagePyramid[level] (fextractor.h:64), fetched from HBM on demand; borderless w x h, tight rows */
    std::vector<uint8_t> ImagePyramidLevel(int level, int* w, int* h) const {
        if (!fe_) throw std::runtime_error("FExtractor: no image has been processed yet");
        check(vslam_fe_level_size(fe_, level, w, h));
        std::vector<uint8_t> out((size_t)*w * *h);
        check(vslam_fe_level_copy(fe_, 0, level, 0, out.data(), (size_t)*w));
        return out;
    }

    /* the device context (NULL before the first compute): device-side consumers -- FMatcher, stereo -- use it */
    vslam_fe* context() const { return fe_; }

    /* The Frame's camera (Pinhole::toK, mDistCoef: 4 or 5 coefficients).  Set it BEFORE compute(): every later pass then
     * also writes the undistorted keypoints on the device (UndistortKeyPoints below reads them).  Kept across the
     * re-creation of the context when the image size changes.  An empty dist removes the camera. */
    void SetCamera(float fx, float fy, float cx, float cy, const std::vector<float>& dist) {
        has_cam_ = !dist.empty();
        if (has_cam_) {
            if (dist.size() != 4 && dist.size() != 5) throw std::invalid_argument("mDistCoef needs 4 or 5 coefficients");
            std::memset(&cam_, 0, sizeof(cam_));
            cam_.fx = fx;
            cam_.fy = fy;
            cam_.cx = cx;
            cam_.cy = cy;
            for (size_t i = 0; i < dist.size(); i++) cam_.dist[i] = dist[i];
            cam_.ndist = (int32_t)dist.size();
        }
        if (fe_) check(vslam_fe_set_camera(fe_, has_cam_ ? &cam_ : nullptr));
    }
    bool HasCamera() const { return has_cam_; }
    float DistortionK1() const { return has_cam_ ? cam_.dist[0] : 0.0f; }

    /* The cvtColor calls of Tracking::GrabImageMonocular / GrabImageStereo / GrabImageRGBD (tracking.cpp:1235-1336):
     * channels = mImGray.channels() (1, 3 or 4), mbRGB = Tracking::mbRGB (Camera.RGB).  Later compute() calls take images of
     * that many channels and the device converts them (COLOR_RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY).  gray_shift: 0 =
     * OpenCV 4.x coefficients, 14 = OpenCV 3.x.  Kept across the re-creation of the context. */
    void SetPixelFormat(int channels, bool mbRGB, int gray_shift = 0) {
        if (channels != 1 && channels != 3 && channels != 4) throw std::invalid_argument("images have 1, 3 or 4 channels");
        const int fmt = channels == 1 ? VSLAM_PIX_GRAY8
                        : channels == 3 ? (mbRGB ? VSLAM_PIX_RGB8 : VSLAM_PIX_BGR8) : (mbRGB ? VSLAM_PIX_RGBA8 : VSLAM_PIX_BGRA8);
        if (fe_) check(vslam_fe_set_pixel_format(fe_, fmt, gray_shift));
        pix_fmt_ = fmt;
        gray_shift_ = gray_shift;
    }
    int Channels() const { return pix_fmt_ == VSLAM_PIX_GRAY8 ? 1 : pix_fmt_ <= VSLAM_PIX_BGR8 ? 3 : 4; }

    /* The extraction + depth section of Frame::Frame(imGray, imDepth, ...) (frame.cpp:185-257): ExtractORB(0, imGray, 0, 0),
     * UndistortKeyPoints, ComputeStereoFromRGBD in one pass of the device.  imRGB: the image as GrabImageRGBD receives it (the
     * extractor's pixel format); imDepth / depth_step / depth_type: the caller's CV_16UC1 (VSLAM_DEPTH_U16) or CV_32FC1
     * (VSLAM_DEPTH_F32) depth image BEFORE convertTo; mDepthMapFactor as Tracking holds it (1 / DepthMapFactor). */
    void computeRGBD(const uint8_t* imRGB, int cols, int rows, size_t step, const void* imDepth, size_t depth_step,
                     int depth_type, float mDepthMapFactor, float mbf, std::vector<KeyPoint>& keypoints,
                     std::vector<KeyPoint>& ukeypoints, std::vector<uint8_t>& descriptors, std::vector<float>& mvuRight,
                     std::vector<float>& mvDepth) {
        ensure(cols, rows);
        const int cap = vslam_fe_capacity(fe_);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        mvuRight.assign(cap, -1.0f);
        mvDepth.assign(cap, -1.0f);
        vslam_kp* kp = reinterpret_cast<vslam_kp*>(keypoints.data());
        uint8_t* dp = descriptors.data();
        float *up = mvuRight.data(), *zp = mvDepth.data();
        int n = 0;
        check(vslam_frame_rgbd_batch_async(fe_, 1, &imRGB, step, VSLAM_IMGS_HOST, &imDepth, depth_step, depth_type,
                                           VSLAM_IMGS_HOST, mDepthMapFactor, mbf, 1));
        check(vslam_frame_rgbd_wait(fe_, &kp, &dp, cap, &n, &up, &zp));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
        mvuRight.resize(n);
        mvDepth.resize(n);
        ukeypoints = keypoints;
        if (has_cam_ && cam_.dist[0] != 0.0f && n) {
            int nu = 0;
            check(vslam_fe_ukps_copy(fe_, 0, reinterpret_cast<vslam_kp*>(ukeypoints.data()), n, &nu));
        }
    }

protected:
    void ensure(int cols, int rows) {
        if (!fe_ || cols != w_ || rows != h_) {
            if (fe_) vslam_fe_destroy(fe_);
            fe_ = nullptr;
            vslam_fe_params p;
            std::memset(&p, 0, sizeof(p));
            p.width = cols;
            p.height = rows;
            p.nfeatures = nfeatures;
            p.scale_factor = (float)scaleFactor;
            p.nlevels = nlevels;
            p.ini_th_fast = iniThFAST;
            p.min_th_fast = minThFAST;
            p.device = device;
            p.max_batch = max_batch;
            check(vslam_fe_create(&p, &fe_));
            w_ = cols;
            h_ = rows;
            if (has_cam_) check(vslam_fe_set_camera(fe_, &cam_));
            if (pix_fmt_ != VSLAM_PIX_GRAY8) check(vslam_fe_set_pixel_format(fe_, pix_fmt_, gray_shift_));
        }
    }

    int run(const uint8_t* data, int cols, int rows, size_t step, int channels, std::vector<KeyPoint>& keypoints,
            std::vector<uint8_t>& desc, std::vector<int>& vLappingArea, int* n_out) {
        if (channels != Channels()) throw std::invalid_argument("FExtractor: image channels differ from SetPixelFormat");
        ensure(cols, rows);
        const int cap = vslam_fe_capacity(fe_); /* quota + the quadtree's overshoot, see vslam_fe.h */
        keypoints.resize(cap);
        desc.resize((size_t)cap * 32);
        int n = 0, mono = 0;
        const int lap0 = vLappingArea.size() > 0 ? vLappingArea[0] : 0, lap1 = vLappingArea.size() > 1 ? vLappingArea[1] : 0;
        check(vslam_fe_extract(fe_, data, step, lap0, lap1, reinterpret_cast<vslam_kp*>(keypoints.data()), desc.data(),
                               cap, &n, &mono));
        keypoints.resize(n);
        *n_out = n;
        return mono;
    }

    int nfeatures;
    double scaleFactor;
    int nlevels;
    int iniThFAST;
    int minThFAST;
    int device, max_batch;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
    vslam_fe* fe_ = nullptr;
    int w_ = 0, h_ = 0;
    bool has_cam_ = false;
    vslam_camera cam_;
    int pix_fmt_ = VSLAM_PIX_GRAY8, gray_shift_ = 0;
};

/* Frame::UndistortKeyPoints (frame.cpp:758-790) for the keypoints the extractor's last compute() returned: with
 * mDistCoef.at<float>(0) == 0 (or no camera) ukeypoints_ = keypoints_, otherwise the device's cv::undistortPoints of
 * them (vslam_fe_ukps_copy). */
inline void UndistortKeyPoints(const FExtractor& extractor, const std::vector<KeyPoint>& keypoints,
                               std::vector<KeyPoint>& ukeypoints) {
    if (!extractor.HasCamera() || extractor.DistortionK1() == 0.0f || keypoints.empty()) {
        ukeypoints = keypoints;
        return;
    }
    if (!extractor.context()) throw std::runtime_error("UndistortKeyPoints: no image has been processed yet");
    ukeypoints.resize(keypoints.size());
    int n = 0;
    const int rc = vslam_fe_ukps_copy(extractor.context(), 0, reinterpret_cast<vslam_kp*>(ukeypoints.data()),
                                      (int)ukeypoints.size(), &n);
    if (rc != VSLAM_OK || n != (int)keypoints.size())
        throw std::runtime_error(rc != VSLAM_OK ? vslam_last_error()
                                                : "UndistortKeyPoints: the extractor's slot no longer holds these keypoints");
}

/* Frame::ComputeImageBounds (frame.cpp:793-821): {0, cols, 0, rows} without distortion (k1 == 0), else the undistorted
 * corners.  Needs the extractor's context (after its first compute()). */
inline void ComputeImageBounds(const FExtractor& extractor, float& mnMinX, float& mnMaxX, float& mnMinY, float& mnMaxY) {
    if (!extractor.context()) throw std::runtime_error("ComputeImageBounds: no image has been processed yet");
    float b[4];
    if (vslam_fe_image_bounds(extractor.context(), b) != VSLAM_OK) throw std::runtime_error(vslam_last_error());
    mnMinX = b[0];
    mnMaxX = b[1];
    mnMinY = b[2];
    mnMaxY = b[3];
}

/* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY for the matchers that run on the extractor's context after initialisation (every
 * SearchByProjection form, Fuse, SearchBySim3): call it once ComputeImageBounds has run, and again after the extractor
 * re-created its context for another image size.  ClearGridBounds returns to {0, cols, 0, rows}.  While bounds are set
 * FMatcher's two SearchByProjection wrappers below hand the device the slot's ukeypoints_ instead of keypoints_.  Always
 * pass the Frame's floats: the KeyFrame-side matchers truncate them to int themselves, as KeyFrame does. */
inline void SetGridBounds(const FExtractor& extractor, float mnMinX, float mnMaxX, float mnMinY, float mnMaxY) {
    if (!extractor.context()) throw std::runtime_error("SetGridBounds: no image has been processed yet");
    const vslam_bounds b = {mnMinX, mnMaxX, mnMinY, mnMaxY};
    if (vslam_fe_set_grid_bounds(extractor.context(), &b) != VSLAM_OK) throw std::runtime_error(vslam_last_error());
}
inline void ClearGridBounds(const FExtractor& extractor) {
    if (extractor.context() && vslam_fe_set_grid_bounds(extractor.context(), nullptr) != VSLAM_OK)
        throw std::runtime_error(vslam_last_error());
}

/* What the matchers read of a Frame (frame.h:71-91): undistorted keypoints, the image bounds of its grid,
 * and where its descriptors are in HBM (the extractor that produced them still holds them). */
struct FrameView {
    const std::vector<KeyPoint>* ukeypoints = nullptr; /* Frame::ukeypoints_ */
    const FExtractor* extractor = nullptr;             /* descriptors_ live in its slot 0 */
    int mnMaxX = 0, mnMaxY = 0;                        /* image bounds (no distortion: cols, rows) */
    /* float grid bounds of a distorted camera (ComputeImageBounds); unset = {0, mnMaxX, 0, mnMaxY}.  Used by
     * SearchForInitialization only (the matchers after initialisation read the context's: SetGridBounds above). */
    bool has_bounds = false;
    vslam_bounds bounds = {0.0f, 0.0f, 0.0f, 0.0f};
};

/* Frame::Frame(imGray, imDepth, timeStamp, extractor, voc, K, distCoef, bf, thDepth, pCamera) (frame.cpp:185-257), the part
 * that runs on the device: the members a Frame keeps of it, over a FrameView for the matchers.  imGray is the image as
 * Tracking::GrabImageRGBD receives it (the extractor converts colour input: FExtractor::SetPixelFormat), imDepth the depth
 * image before GrabImageRGBD's convertTo, which the device applies with mDepthMapFactor.  K and distCoef go to the
 * extractor once (FExtractor::SetCamera), as they are the same for every Frame.  The vocabulary, the time stamp and thDepth
 * are not read by anything computed here. */
struct DepthImage {
    const void* data = nullptr;
    size_t step = 0;
    int type = VSLAM_DEPTH_U16; /* VSLAM_DEPTH_U16 (CV_16UC1) or VSLAM_DEPTH_F32 (CV_32FC1) */
};
struct FrameRGBD : FrameView {
    std::vector<KeyPoint> keypoints_, ukeypoints_;
    std::vector<uint8_t> descriptors_; /* N x 32 */
    std::vector<float> mvuRight, mvDepth;
    int N = 0;
    float mbf = 0.0f, mThDepth = 0.0f;
    double mTimeStamp = 0.0;

    FrameRGBD(const uint8_t* imGray, int cols, int rows, size_t step, const DepthImage& imDepth, float mDepthMapFactor,
              double timeStamp, FExtractor* pExtractor, float bf, float thDepth)
        : mbf(bf), mThDepth(thDepth), mTimeStamp(timeStamp) {
        pExtractor->computeRGBD(imGray, cols, rows, step, imDepth.data, imDepth.step, imDepth.type, mDepthMapFactor, bf,
                                keypoints_, ukeypoints_, descriptors_, mvuRight, mvDepth);
        N = (int)keypoints_.size();
        ukeypoints = &ukeypoints_;
        extractor = pExtractor;
        mnMaxX = cols;
        mnMaxY = rows;
        if (pExtractor->HasCamera()) {
            ComputeImageBounds(*pExtractor, bounds.min_x, bounds.max_x, bounds.min_y, bounds.max_y);
            has_bounds = true;
        }
    }
    FrameRGBD(const FrameRGBD&) = delete; /* FrameView::ukeypoints points into this object */
    FrameRGBD& operator=(const FrameRGBD&) = delete;
};

/* DBoW3::FeatureVector (a std::map in the reference) as the flat arrays the library takes: ascending node ids, nodes.size() + 1
 * offsets into feat, the feature indices of each node in order.  (BowVector, its sibling, stands before KeyFrameDatabase.) */
struct FeatureVector {
    std::vector<int> nodes, off, feat;
};

/* ---------------------------------------------------------------------------------------------------
 * FMatcher (fmatcher.h:70-147), hot-path subset
 * ------------------------------------------------------------------------------------------------- */
class FMatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30; /* fmatcher.cpp:313-315 */

    FMatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    /* fmatcher.cpp:2859-2875: 256-bit Hamming distance of two descriptor rows */
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
        int dist = 0;
        for (int i = 0; i < 8; i++) {
            uint32_t pa, pb;
            std::memcpy(&pa, a + 4 * i, 4);
            std::memcpy(&pb, b + 4 * i, 4);
            dist += __builtin_popcount(pa ^ pb);
        }
        return dist;
    }

    /* fmatcher.cpp:983-1098 */
    int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<Point2f>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10) {
        const std::vector<KeyPoint>& k1 = *F1.ukeypoints;
        const std::vector<KeyPoint>& k2 = *F2.ukeypoints;
        vnMatches12.assign(k1.size(), -1);
        if (k1.empty()) return 0;
        if (vbPrevMatched.size() != k1.size()) throw std::invalid_argument("vbPrevMatched.size() != F1 keypoints");
        const uint8_t *d1 = nullptr, *d2 = nullptr;
        int n1 = 0, n2 = 0, nm = 0;
        check(vslam_fe_slot_buffers(F1.extractor->context(), 0, nullptr, &d1, &n1));
        check(vslam_fe_slot_buffers(F2.extractor->context(), 0, nullptr, &d2, &n2));
        if (n1 != (int)k1.size() || n2 != (int)k2.size())
            throw std::runtime_error("FMatcher: the extractor's slot no longer holds this frame's descriptors");
        if (F2.has_bounds) {
            check(vslam_search_for_initialization_ex(F2.extractor->context(), reinterpret_cast<const vslam_kp*>(k1.data()),
                                                     d1, n1, reinterpret_cast<const vslam_kp*>(k2.data()), d2, n2,
                                                     &F2.bounds, reinterpret_cast<float*>(vbPrevMatched.data()),
                                                     vnMatches12.data(), windowSize, mfNNratio, mbCheckOrientation ? 1 : 0,
                                                     &nm));
            return nm;
        }
        check(vslam_search_for_initialization(F2.extractor->context(), reinterpret_cast<const vslam_kp*>(k1.data()), d1,
                                              n1, reinterpret_cast<const vslam_kp*>(k2.data()), d2, n2, F2.mnMaxX,
                                              F2.mnMaxY, reinterpret_cast<float*>(vbPrevMatched.data()),
                                              vnMatches12.data(), windowSize, mfNNratio, mbCheckOrientation ? 1 : 0,
                                              &nm));
        return nm;
    }

    /* fmatcher.cpp:2471-2687 (pinhole frames).  What the function reads of the two Frames:
     *   cur : pose rows [Rcw | tcw] (T_w_c_ as the reference uses it), intrinsics, mbf, mb, mvuRight, grid bounds,
     *         and the extractor slot that still holds its keypoints/descriptors in HBM
     *   last: ukeypoints_ (octave, angle), pose, and per keypoint its MapPoint (flags bit0 = present and not an
     *         outlier, bit1 = Observations() > 0, world position, descriptor)
     * mvpMapPointIndex[i2] = index into the last frame whose MapPoint ends up in CurrentFrame.mvpMapPoints[i2]. */
    struct CurrentFrameView {
        FrameView frame;
        float Tcw[12];
        float fx, fy, cx, cy, mbf, mb;
        const std::vector<float>* mvuRight = nullptr; /* NULL: monocular */
    };
    struct LastFrameView {
        const std::vector<KeyPoint>* ukeypoints = nullptr;
        float Tlw[12];
        const std::vector<uint8_t>* mapPointFlags = nullptr;
        const std::vector<float>* mapPointWorldPos = nullptr;    /* 3 per keypoint */
        const std::vector<uint8_t>* mapPointDescriptors = nullptr; /* 32 per keypoint */
    };
    int SearchByProjection(const CurrentFrameView& cur, const LastFrameView& last, const float th, const bool bMono,
                           std::vector<int>& mvpMapPointIndex) {
        vslam_proj_params p;
        std::memset(&p, 0, sizeof(p));
        std::memcpy(p.Tcw, cur.Tcw, sizeof(p.Tcw));
        p.fx = cur.fx; p.fy = cur.fy; p.cx = cur.cx; p.cy = cur.cy; p.mbf = cur.mbf; p.th = th;
        p.check_orientation = mbCheckOrientation ? 1 : 0;
        p.img_w = cur.frame.mnMaxX;
        p.img_h = cur.frame.mnMaxY;
        check(vslam_projection_direction(cur.Tcw, last.Tlw, cur.mb, bMono ? 1 : 0, 0, &p.forward, &p.backward));
        const vslam_kp* dk = nullptr;
        const uint8_t* dd = nullptr;
        int n2 = 0, nm = 0;
        slot_keypoints(*cur.frame.extractor, &dk, &dd, &n2);
        mvpMapPointIndex.assign(n2, -1);
        const int n = (int)last.ukeypoints->size();
        check(vslam_search_by_projection_frame(cur.frame.extractor->context(), &p,
                                               reinterpret_cast<const vslam_kp*>(last.ukeypoints->data()), n,
                                               last.mapPointFlags->data(), last.mapPointWorldPos->data(),
                                               last.mapPointDescriptors->data(), dk, dd, n2,
                                               cur.mvuRight ? cur.mvuRight->data() : nullptr, nullptr,
                                               mvpMapPointIndex.data(), &nm));
        return nm;
    }

    /* fmatcher.cpp:321-411 (pinhole frames): vpMapPoints as vslam_mp_track records + descriptors; occupied marks
     * keypoints of F whose mvpMapPoints entry already holds a MapPoint with observations */
    int SearchByProjection(const FrameView& F, const std::vector<float>* mvuRight, const std::vector<vslam_mp_track>& vpMapPoints,
                           const std::vector<uint8_t>& mapPointDescriptors, const std::vector<uint8_t>* occupied,
                           const float th, std::vector<int>& mvpMapPointIndex) {
        const vslam_kp* dk = nullptr;
        const uint8_t* dd = nullptr;
        int n2 = 0, nm = 0;
        slot_keypoints(*F.extractor, &dk, &dd, &n2);
        mvpMapPointIndex.assign(n2, -1);
        check(vslam_search_by_projection_mappoints(F.extractor->context(), vpMapPoints.data(), mapPointDescriptors.data(),
                                                   (int)vpMapPoints.size(), dk, dd, n2,
                                                   mvuRight ? mvuRight->data() : nullptr,
                                                   occupied ? occupied->data() : nullptr, F.mnMaxX, F.mnMaxY, th,
                                                   mfNNratio, mvpMapPointIndex.data(), &nm));
        return nm;
    }

    /* Tracking::SearchLocalPoints from its second loop on (tracking.cpp:3214-3263): Frame::isInFrustum(pMP, 0.5) over
     * mvpLocalMapPoints and matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, mbFarPoints, mThFarPoints) in
     * one enqueue.  What the two functions read of the Frame and of the MapPoints:
     *   cur               pose rows [mRcwx | mtcwx], mOwx, intrinsics, mbf, mfLogScaleFactor, mvuRight, and the extractor slot
     *   mvpLocalMapPoints vslam_map_point per MapPoint (GetWorldPos2, GetNormal2, Get{Min,Max}DistanceInvariance, flags bit0 =
     *                     mnLastFrameSeen != mCurrentFrame.id_ && !isBad(), bit1 = Observations() > 0) + descriptors
     * mvpMapPointIndex[i2] = index into mvpLocalMapPoints of the point written to mCurrentFrame.mvpMapPoints[i2], or -1;
     * nToMatch as the reference counts it; mTrack (may be NULL) receives what isInFrustum left in every MapPoint
     * (mbTrackInView = flags & 1, mTrackProjX / Y for mmProjectPoints).  The loop over mCurrentFrame.mvpMapPoints
     * (:3195-3212), IncreaseVisible and the choice of th stay with the caller.  Returns the matches. */
    struct LocalFrameView {
        FrameView frame;
        float Tcw[12], Ow[3];
        float fx, fy, cx, cy, mbf, mfLogScaleFactor;
        const std::vector<float>* mvuRight = nullptr; /* NULL: monocular */
    };
    int SearchLocalPoints(const LocalFrameView& cur, const std::vector<vslam_map_point>& mvpLocalMapPoints,
                          const std::vector<uint8_t>& mapPointDescriptors, const std::vector<uint8_t>* occupied,
                          const float th, const bool bFarPoints, const float thFarPoints,
                          std::vector<int>& mvpMapPointIndex, int& nToMatch, std::vector<vslam_mp_track>* mTrack = nullptr,
                          const float viewingCosLimit = 0.5f) {
        vslam_frustum_params p;
        std::memset(&p, 0, sizeof(p));
        std::memcpy(p.Tcw, cur.Tcw, sizeof(p.Tcw));
        std::memcpy(p.Ow, cur.Ow, sizeof(p.Ow));
        p.fx = cur.fx; p.fy = cur.fy; p.cx = cur.cx; p.cy = cur.cy; p.mbf = cur.mbf;
        p.viewing_cos_limit = viewingCosLimit;
        p.log_scale_factor = cur.mfLogScaleFactor;
        p.img_w = cur.frame.mnMaxX;
        p.img_h = cur.frame.mnMaxY;
        p.far_points = bFarPoints ? 1 : 0;
        p.th_far_points = thFarPoints;
        const vslam_kp* dk = nullptr;
        const uint8_t* dd = nullptr;
        int n2 = 0, nm = 0, against = 0;
        slot_keypoints(*cur.frame.extractor, &dk, &dd, &n2);
        mvpMapPointIndex.assign(n2, -1);
        nToMatch = 0;
        if (mTrack) mTrack->resize(mvpLocalMapPoints.size());
        check(vslam_search_local_points(cur.frame.extractor->context(), &p, mvpLocalMapPoints.data(),
                                        mapPointDescriptors.data(), (int)mvpLocalMapPoints.size(), VSLAM_IMGS_HOST, dk, dd, n2,
                                        cur.mvuRight ? cur.mvuRight->data() : nullptr,
                                        occupied ? occupied->data() : nullptr, th, mfNNratio, mvpMapPointIndex.data(), &nm,
                                        &nToMatch, &against, (mTrack && n2 > 0 && !mTrack->empty()) ? mTrack->data() : nullptr));
        return nm;
    }

    /* The same for a two-fisheye rig (Frame::Nleft != -1; isInFrustumChecks frame.cpp:1191-1271 and both branches of
     * SearchByProjection(F, vpMapPoints), fmatcher.cpp:321-491).  cur.left is the left camera: its pose, its intrinsics (those
     * of the KannalaBrandt8 attached to its extractor) and keypoints_ in its extractor's slot 0; `right` is the extractor that
     * holds keypointsRight_ (mpORBextractorRight), rig the right camera with mTlr / mTrl.  F.mvpMapPoints has Nleft + Nright
     * slots, left first: mvpMapPointIndex and `occupied` are laid out that way.  mTrack / mTrackR (may be NULL) receive
     * the records of the left and of the right camera; nToMatch counts left || right (tracking.cpp:3226-3230). */
    struct RigFrameView {
        LocalFrameView left;
        const FExtractor* right = nullptr;
        vslam_kb8_rig rig;
        const std::vector<int>* mvLeftToRightMatch = nullptr;
        const std::vector<int>* mvRightToLeftMatch = nullptr;
        /* read by SearchByProjection(rig frame, last frame) alone: the stereo baseline of bForward / bBackward, and -- optional,
         * for the host fallback beyond the device's limits -- keypointsRight_ and both cameras' descriptor rows on the host
         * (keypoints_ is left.frame.ukeypoints) */
        float mb = 0.0f;
        const vslam_kb8_camera* camera = nullptr; /* the left camera's mvParameters, as attached to the left extractor */
        const std::vector<KeyPoint>* keypointsRight = nullptr;
        const std::vector<uint8_t>* descriptorsLeft = nullptr;  /* 32 per keypoint */
        const std::vector<uint8_t>* descriptorsRight = nullptr;
        /* read by SearchByBoW alone: mFeatVec over the Nleft + Nright features, left first (DBoW3::Vocabulary::transform of a
         * RigFrameView) */
        const FeatureVector* mFeatVec = nullptr;
    };
    int SearchLocalPoints(const RigFrameView& cur, const std::vector<vslam_map_point>& mvpLocalMapPoints,
                          const std::vector<uint8_t>& mapPointDescriptors, const std::vector<uint8_t>* occupied,
                          const float th, const bool bFarPoints, const float thFarPoints,
                          std::vector<int>& mvpMapPointIndex, int& nToMatch, std::vector<vslam_mp_track>* mTrack = nullptr,
                          std::vector<vslam_mp_track>* mTrackR = nullptr, const float viewingCosLimit = 0.5f) {
        static_assert(sizeof(int) == sizeof(int32_t), "mvLeftToRightMatch is handed over as int32");
        if (!cur.right || !cur.mvLeftToRightMatch || !cur.mvRightToLeftMatch)
            throw std::invalid_argument("SearchLocalPoints: a rig frame needs its right extractor and both match maps");
        const LocalFrameView& L = cur.left;
        vslam_frustum_params p;
        std::memset(&p, 0, sizeof(p));
        std::memcpy(p.Tcw, L.Tcw, sizeof(p.Tcw));
        std::memcpy(p.Ow, L.Ow, sizeof(p.Ow));
        p.fx = L.fx; p.fy = L.fy; p.cx = L.cx; p.cy = L.cy; p.mbf = L.mbf;
        p.viewing_cos_limit = viewingCosLimit;
        p.log_scale_factor = L.mfLogScaleFactor;
        p.img_w = L.frame.mnMaxX;
        p.img_h = L.frame.mnMaxY;
        p.far_points = bFarPoints ? 1 : 0;
        p.th_far_points = thFarPoints;
        vslam_rig_frame f;
        std::memset(&f, 0, sizeof(f));
        check(vslam_fe_slot_buffers(L.frame.extractor->context(), 0, &f.dev_kps_left, &f.dev_desc_left, &f.n_left));
        check(vslam_fe_slot_buffers(cur.right->context(), 0, &f.dev_kps_right, &f.dev_desc_right, &f.n_right));
        if ((int)cur.mvLeftToRightMatch->size() != f.n_left || (int)cur.mvRightToLeftMatch->size() != f.n_right ||
            (occupied && (int)occupied->size() != f.n_left + f.n_right))
            throw std::invalid_argument("SearchLocalPoints: match maps / occupancy do not fit the rig's keypoints");
        f.left_to_right_host = cur.mvLeftToRightMatch->data();
        f.right_to_left_host = cur.mvRightToLeftMatch->data();
        f.occupied_host = occupied ? occupied->data() : nullptr;
        const int N = f.n_left + f.n_right;
        int nm = 0, against = 0;
        mvpMapPointIndex.assign(N, -1);
        nToMatch = 0;
        if (mTrack) mTrack->resize(mvpLocalMapPoints.size());
        if (mTrackR) mTrackR->resize(mvpLocalMapPoints.size());
        const bool records = N > 0 && !mvpLocalMapPoints.empty();
        check(vslam_search_local_points_rig(L.frame.extractor->context(), &p, &cur.rig, mvpLocalMapPoints.data(),
                                            mapPointDescriptors.data(), (int)mvpLocalMapPoints.size(), VSLAM_IMGS_HOST, &f, th,
                                            mfNNratio, mvpMapPointIndex.data(), &nm, &nToMatch, &against,
                                            (mTrack && records) ? mTrack->data() : nullptr,
                                            (mTrackR && records) ? mTrackR->data() : nullptr));
        return nm;
    }

    /* FMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) for a two-fisheye rig
     * (fmatcher.cpp:2494-2684 with Nleft != -1; TrackWithMotionModel, tracking.cpp:2728 / :2736).  cur: as for the rig
     * SearchLocalPoints (pose, the intrinsics of the KannalaBrandt8 attached to the left extractor, both extractors' slot 0,
     * rig.Trl) plus mb; the match maps are not read.  last: as for the pinhole form, with ukeypoints = the last frame's
     * keypoints_ followed by its keypointsRight_ (Nleft + Nright entries, octave and angle are read) and one flag byte, world
     * position and descriptor per entry.  CurrentFrame.mvpMapPoints has Nleft + Nright slots, left first: mvpMapPointIndex[slot]
     * = index into the last frame of the MapPoint that ends in the slot, or -1; `occupied` (may be NULL) is laid out that way.
     * Beyond the device's limits (4096 last-frame entries, 4096 keypoints per camera) the call runs the sequential host form,
     * if cur carries camera, keypointsRight and both descriptor arrays; otherwise it throws.  Returns the matches. */
    int SearchByProjection(const RigFrameView& cur, const LastFrameView& last, const float th, const bool bMono,
                           std::vector<int>& mvpMapPointIndex, const std::vector<uint8_t>* occupied = nullptr) {
        static_assert(sizeof(KeyPoint) == sizeof(vslam_kp), "KeyPoint arrays are handed over as vslam_kp");
        if (!cur.right || !last.ukeypoints || !last.mapPointFlags || !last.mapPointWorldPos || !last.mapPointDescriptors)
            throw std::invalid_argument("SearchByProjection: a rig frame needs its right extractor, the last frame its arrays");
        const LocalFrameView& L = cur.left;
        const size_t n = last.ukeypoints->size();
        if (last.mapPointFlags->size() != n || last.mapPointWorldPos->size() != 3 * n || last.mapPointDescriptors->size() != 32 * n)
            throw std::invalid_argument("SearchByProjection: one flag, position and descriptor per last-frame keypoint");
        vslam_proj_params p;
        std::memset(&p, 0, sizeof(p));
        std::memcpy(p.Tcw, L.Tcw, sizeof(p.Tcw));
        p.fx = L.fx; p.fy = L.fy; p.cx = L.cx; p.cy = L.cy; p.mbf = L.mbf; p.th = th;
        p.check_orientation = mbCheckOrientation ? 1 : 0;
        p.img_w = L.frame.mnMaxX;
        p.img_h = L.frame.mnMaxY;
        check(vslam_projection_direction(L.Tcw, last.Tlw, cur.mb, bMono ? 1 : 0, 0, &p.forward, &p.backward));
        vslam_rig_frame f;
        std::memset(&f, 0, sizeof(f));
        check(vslam_fe_slot_buffers(L.frame.extractor->context(), 0, &f.dev_kps_left, &f.dev_desc_left, &f.n_left));
        check(vslam_fe_slot_buffers(cur.right->context(), 0, &f.dev_kps_right, &f.dev_desc_right, &f.n_right));
        const int N = f.n_left + f.n_right;
        if (occupied && (int)occupied->size() != N)
            throw std::invalid_argument("SearchByProjection: occupancy does not fit the rig's keypoints");
        f.occupied_host = occupied ? occupied->data() : nullptr;
        mvpMapPointIndex.assign(N, -1);
        int nm = 0;
        const vslam_kp* lk = reinterpret_cast<const vslam_kp*>(last.ukeypoints->data());
        const int rc = vslam_search_by_projection_frame_rig(L.frame.extractor->context(), &p, &cur.rig, lk, (int)n,
                                                            last.mapPointFlags->data(), last.mapPointWorldPos->data(),
                                                            last.mapPointDescriptors->data(), &f, mvpMapPointIndex.data(), &nm);
        if (rc != VSLAM_ERR_UNSUPPORTED) {
            check(rc);
            return nm;
        }
        /* over the device's limits: the reference loop on the host */
        if (!cur.camera || !L.frame.ukeypoints || !cur.keypointsRight || !cur.descriptorsLeft || !cur.descriptorsRight ||
            (int)L.frame.ukeypoints->size() != f.n_left || (int)cur.keypointsRight->size() != f.n_right ||
            cur.descriptorsLeft->size() != 32 * (size_t)f.n_left || cur.descriptorsRight->size() != 32 * (size_t)f.n_right)
            check(rc);
        const vslam_kb8_camera& cam = *cur.camera;
        const std::vector<float> sf = const_cast<FExtractor*>(L.frame.extractor)->GetScaleFactors();
        vslam_bounds b;
        int is_set = 0;
        check(vslam_fe_get_grid_bounds(L.frame.extractor->context(), &b, &is_set));
        const float bounds[4] = {is_set ? b.min_x : 0.0f, is_set ? b.max_x : (float)p.img_w, is_set ? b.min_y : 0.0f,
                                 is_set ? b.max_y : (float)p.img_h};
        check(vslamh_search_by_projection_frame_rig(&p, &cam, cur.rig.Trl, lk, (int)n, last.mapPointFlags->data(),
                                                    last.mapPointWorldPos->data(), last.mapPointDescriptors->data(),
                                                    reinterpret_cast<const vslam_kp*>(L.frame.ukeypoints->data()),
                                                    cur.descriptorsLeft->data(), f.n_left,
                                                    reinterpret_cast<const vslam_kp*>(cur.keypointsRight->data()),
                                                    cur.descriptorsRight->data(), f.n_right, f.occupied_host, sf.data(),
                                                    (int)sf.size(), bounds, mvpMapPointIndex.data(), &nm));
        return nm;
    }

    /* FMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (fmatcher.cpp:546-748) for a
     * two-fisheye rig (F.Nleft != -1).  A rig KeyFrame: its descriptor rows in HBM per camera (a KeyFrame made from a frame keeps
     * the addresses of the slots it was extracted into, or of its own copies), ONE keypoint array mvKeys followed by mvKeysRight
     * (the angle is read), one flag per feature (has a MapPoint that is not bad) and mFeatVec over NLeft + NRight features.
     * `descriptors` (optional, (NLeft + NRight) x 32 bytes on the host) is read by the host fallback alone; `extractor` by the
     * KeyFrame-KeyFrame overload alone (the context to run on).
     * The vector form is the relocalisation loop (tracking.cpp:3488-3509): every candidate KeyFrame against the one frame in one
     * enqueue, up to 16 per call (more are served in groups of 16).  vvpMapPointIndex[k][slot] = index of KeyFrame k's feature
     * whose MapPoint goes to vpMapPointMatches[slot] (Nleft + Nright slots, left first), or -1; the returned vector holds the
     * nmatches of each KeyFrame.  cur: both extractors' slot 0 and mFeatVec are read; no pose, no camera.
     * Beyond the device's limits (4096 features per camera, 2048 frame features under one node) the call runs the sequential
     * host form, if cur carries ukeypoints, keypointsRight and both descriptor arrays and every KeyFrame its descriptors;
     * otherwise it throws. */
    struct RigKeyFrameView {
        const uint8_t* dev_desc_left = nullptr;
        const uint8_t* dev_desc_right = nullptr;
        int NLeft = 0, NRight = 0;
        const std::vector<KeyPoint>* keys = nullptr;          /* mvKeys then mvKeysRight */
        const std::vector<uint8_t>* mapPointFlags = nullptr;  /* NLeft + NRight */
        const FeatureVector* mFeatVec = nullptr;
        const std::vector<uint8_t>* descriptors = nullptr;
        const FExtractor* extractor = nullptr;
    };
    std::vector<int> SearchByBoW(const std::vector<RigKeyFrameView>& vpKFs, const RigFrameView& cur,
                                 std::vector<std::vector<int> >& vvpMapPointIndex) {
        static_assert(sizeof(KeyPoint) == sizeof(vslam_kp) && sizeof(int) == sizeof(int32_t), "arrays are handed over as they are");
        if (!cur.right || !cur.left.frame.extractor || !cur.mFeatVec)
            throw std::invalid_argument("SearchByBoW: a rig frame needs both extractors and its FeatureVector");
        const FeatureVector& ffv = *cur.mFeatVec;
        if (ffv.off.size() != ffv.nodes.size() + 1) throw std::invalid_argument("SearchByBoW: FeatureVector offsets");
        vslam_fe* fe = cur.left.frame.extractor->context();
        vslam_rig_frame f;
        std::memset(&f, 0, sizeof(f));
        check(vslam_fe_slot_buffers(fe, 0, &f.dev_kps_left, &f.dev_desc_left, &f.n_left));
        check(vslam_fe_slot_buffers(cur.right->context(), 0, &f.dev_kps_right, &f.dev_desc_right, &f.n_right));
        const int N = f.n_left + f.n_right;
        std::vector<int> nmatches(vpKFs.size(), 0);
        vvpMapPointIndex.assign(vpKFs.size(), std::vector<int>((size_t)N, -1));
        for (size_t first = 0; first < vpKFs.size(); first += 16) {
            const int K = (int)std::min<size_t>(16, vpKFs.size() - first);
            vslam_bow_rig_kf jobs[16];
            int32_t* out[16];
            std::memset(jobs, 0, sizeof(jobs));
            for (int j = 0; j < K; j++) {
                const RigKeyFrameView& k = vpKFs[first + j];
                const size_t n = (size_t)k.NLeft + (size_t)k.NRight;
                if (k.NLeft < 0 || k.NRight < 0 || !k.keys || !k.mapPointFlags || !k.mFeatVec || k.keys->size() != n ||
                    k.mapPointFlags->size() != n || k.mFeatVec->off.size() != k.mFeatVec->nodes.size() + 1)
                    throw std::invalid_argument("SearchByBoW: a rig KeyFrame holds NLeft + NRight keypoints and flags and a FeatureVector");
                jobs[j].dev_desc_left = k.dev_desc_left;
                jobs[j].n_left = k.NLeft;
                jobs[j].dev_desc_right = k.dev_desc_right;
                jobs[j].n_right = k.NRight;
                jobs[j].kps_host = reinterpret_cast<const vslam_kp*>(k.keys->data());
                jobs[j].flags_host = k.mapPointFlags->data();
                jobs[j].fv_nodes = k.mFeatVec->nodes.data();
                jobs[j].fv_off = k.mFeatVec->off.data();
                jobs[j].fv_feat = k.mFeatVec->feat.data();
                jobs[j].n_nodes = (int)k.mFeatVec->nodes.size();
                out[j] = vvpMapPointIndex[first + j].data();
            }
            const int rc = vslam_search_by_bow_rig(fe, jobs, K, &f, ffv.nodes.data(), ffv.off.data(), ffv.feat.data(),
                                                   (int)ffv.nodes.size(), mfNNratio, mbCheckOrientation ? 1 : 0, out,
                                                   nmatches.data() + first);
            if (rc != VSLAM_ERR_UNSUPPORTED) {
                check(rc);
                continue;
            }
            /* over the device's limits: the reference loop on the host, one KeyFrame after the other */
            const std::vector<KeyPoint>* kl = cur.left.frame.ukeypoints;
            if (!kl || !cur.keypointsRight || !cur.descriptorsLeft || !cur.descriptorsRight || (int)kl->size() != f.n_left ||
                (int)cur.keypointsRight->size() != f.n_right || cur.descriptorsLeft->size() != 32 * (size_t)f.n_left ||
                cur.descriptorsRight->size() != 32 * (size_t)f.n_right)
                check(rc);
            for (int j = 0; j < K; j++) {
                const RigKeyFrameView& k = vpKFs[first + j];
                if (!k.descriptors || k.descriptors->size() != 32 * ((size_t)k.NLeft + (size_t)k.NRight)) check(rc);
                check(vslamh_search_by_bow_rig(jobs[j].kps_host, k.descriptors->data(), k.NLeft,
                                               k.descriptors->data() + 32 * (size_t)k.NLeft, k.NRight, jobs[j].flags_host,
                                               jobs[j].fv_nodes, jobs[j].fv_off, jobs[j].fv_feat, jobs[j].n_nodes,
                                               reinterpret_cast<const vslam_kp*>(kl->data()), cur.descriptorsLeft->data(), f.n_left,
                                               reinterpret_cast<const vslam_kp*>(cur.keypointsRight->data()),
                                               cur.descriptorsRight->data(), f.n_right, ffv.nodes.data(), ffv.off.data(),
                                               ffv.feat.data(), (int)ffv.nodes.size(), mfNNratio, mbCheckOrientation ? 1 : 0,
                                               out[j], &nmatches[first + j]));
            }
        }
        return nmatches;
    }
    /* one KeyFrame: TrackReferenceKeyFrame's call (tracking.cpp:2578).  Returns nmatches. */
    int SearchByBoW(const RigKeyFrameView& pKF, const RigFrameView& cur, std::vector<int>& vpMapPointIndex) {
        std::vector<std::vector<int> > all;
        const std::vector<int> nm = SearchByBoW(std::vector<RigKeyFrameView>(1, pKF), cur, all);
        vpMapPointIndex.swap(all[0]);
        return nm[0];
    }
    /* FMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (fmatcher.cpp:1100-1240) for rig
     * KeyFrames: idx >= mvKeysUn.size() is skipped on both sides and a rig's mvKeysUn has NLeft entries, so right features are
     * neither queries nor candidates.  vpMatches12[idx1] = idx2 or -1, NLeft + NRight entries.  Runs on pKF1.extractor's
     * context.  Returns nmatches. */
    int SearchByBoW(const RigKeyFrameView& pKF1, const RigKeyFrameView& pKF2, std::vector<int>& vpMatches12) {
        const RigKeyFrameView* k[2] = {&pKF1, &pKF2};
        for (int i = 0; i < 2; i++)
            if (!k[i]->keys || !k[i]->mapPointFlags || !k[i]->mFeatVec || k[i]->NLeft < 0 || k[i]->NRight < 0 ||
                (int)k[i]->keys->size() < k[i]->NLeft || (int)k[i]->mapPointFlags->size() != k[i]->NLeft + k[i]->NRight ||
                k[i]->mFeatVec->off.size() != k[i]->mFeatVec->nodes.size() + 1)
                throw std::invalid_argument("SearchByBoW: a rig KeyFrame holds its keypoints, NLeft + NRight flags and a FeatureVector");
        if (!pKF1.extractor) throw std::invalid_argument("SearchByBoW: the first KeyFrame names the extractor to run on");
        const int n1 = pKF1.NLeft + pKF1.NRight, n2 = pKF2.NLeft + pKF2.NRight;
        vpMatches12.assign((size_t)n1, -1);
        int nm = 0;
        check(vslam_search_by_bow_keyframes_rig(
            pKF1.extractor->context(), reinterpret_cast<const vslam_kp*>(pKF1.keys->data()), pKF1.dev_desc_left,
            pKF1.mapPointFlags->data(), n1, pKF1.NLeft, pKF1.mFeatVec->nodes.data(), pKF1.mFeatVec->off.data(),
            pKF1.mFeatVec->feat.data(), (int)pKF1.mFeatVec->nodes.size(), reinterpret_cast<const vslam_kp*>(pKF2.keys->data()),
            pKF2.dev_desc_left, pKF2.mapPointFlags->data(), n2, pKF2.NLeft, pKF2.mFeatVec->nodes.data(), pKF2.mFeatVec->off.data(),
            pKF2.mFeatVec->feat.data(), (int)pKF2.mFeatVec->nodes.size(), mfNNratio, mbCheckOrientation ? 1 : 0,
            vpMatches12.data(), &nm));
        return nm;
    }

    /* The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) (fmatcher.cpp:1918-2119) for a fisheye KeyFrame / both
     * cameras of a two-fisheye rig: ONE list of candidate MapPoints against any number of (KeyFrame, camera) jobs, 16 per
     * enqueue (more are served in groups of 16).  A job is one call of Fuse -- vslam_fuse_rig_job (include/vslam_fe.h): the
     * camera's own pose, camera 0 / 1, the side's keypoints and descriptor rows in HBM, idx_offset 0 or NLeft, and one byte per
     * MapPoint that is 0 where IsInKeyFrame(pKF) holds.  LocalMapping::SearchInNeighbors lists, for every target KeyFrame, its
     * left job and then its right one.  points[i].valid = pMP && !pMP->isBad().  extractor: the context to run on, with the
     * KannalaBrandt8 of mpCamera attached; rig (may be NULL when no job has camera 1) carries mpCamera2.
     * gemmFloat: as vslam_fuse_params::gemm_float (a reference build whose cv::gemm stays in float).  The window grid and IsInImage
     * use the context's grid bounds while it holds any (SetGridBounds), else {0, imgW, 0, imgH}.
     * bestIdx / bestDist: jobs.size() * points.size() entries each, job-major; -1 / 256 where nothing passes.  What the
     * reference does with a result -- Replace / AddObservation + AddMapPoint where bestDist <= TH_LOW -- stays with the caller:
     * FuseWalk below. */
    void FuseSearchRig(const FExtractor& extractor, const vslam_kb8_rig* rig, const std::vector<vslam_fuse_rig_job>& jobs,
                       const std::vector<vslam_fuse_point>& points, const std::vector<uint8_t>& mapPointDescriptors, const float th,
                       const float logScaleFactor, const int imgW, const int imgH, std::vector<int>& bestIdx,
                       std::vector<int>& bestDist, const bool gemmFloat = false) {
        static_assert(sizeof(int) == sizeof(int32_t), "the results are handed over as int32");
        if (mapPointDescriptors.size() != 32 * points.size())
            throw std::invalid_argument("FuseSearchRig: one descriptor per MapPoint");
        const size_t n = points.size();
        bestIdx.assign(jobs.size() * n, -1);
        bestDist.assign(jobs.size() * n, 256);
        vslam_fuse_params p;
        std::memset(&p, 0, sizeof(p));
        p.th = th;
        p.log_scale_factor = logScaleFactor;
        p.img_w = imgW;
        p.img_h = imgH;
        p.gemm_float = gemmFloat ? 1 : 0;
        for (size_t first = 0; first < jobs.size() && n; first += VSLAM_FUSE_RIG_MAX_JOBS) {
            const int K = (int)std::min<size_t>(VSLAM_FUSE_RIG_MAX_JOBS, jobs.size() - first);
            check(vslam_fuse_search_rig(extractor.context(), &p, rig, jobs.data() + first, K, points.data(),
                                        mapPointDescriptors.data(), (int)n, VSLAM_IMGS_HOST, bestIdx.data() + first * n,
                                        bestDist.data() + first * n));
        }
    }

    /* FMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (fmatcher.cpp:2689-2811) with
     * a fisheye CurrentFrame -- Tracking::Relocalization's matcher for a monocular KB8 frame or the left camera of a two-fisheye
     * rig.  extractor: the context that extracted the frame (of a rig the LEFT camera's: only keypoints_ and slots [0, Nleft) take
     * part), with the KannalaBrandt8 of mpCamera attached; camera: its parameters (fx .. cy travel in the projection record).
     * Tcw: rows [Rcw | tcw] of CurrentFrame.T_w_c_, Ow = -Rcw^T tcw.  Per entry i of pKF->GetMapPointMatches() (N = NLeft +
     * NRight entries for a rig KeyFrame): keyFrameKeys[i] = mvKeys followed by mvKeysRight (the reference reads mvKeysUn[i].angle
     * past its end for i >= NLeft; the right keypoint's angle is read instead), mapPointFlags[i] & 1 = pMP && !isBad() &&
     * !sAlreadyFound.count(pMP), position (3 floats), Get{Min,Max}DistanceInvariance(), descriptor.  occupied (may be NULL): one
     * byte per current keypoint, CurrentFrame.mvpMapPoints[i2] != NULL.  matchCur[i2] = i or -1; returns nmatches. */
    int SearchByProjectionKeyFrameKB8(const FExtractor& extractor, const vslam_kb8_camera& camera, const float* Tcw,
                                      const float* Ow, const float th, const int ORBdist, const float logScaleFactor,
                                      const int imgW, const int imgH, const std::vector<KeyPoint>& keyFrameKeys,
                                      const std::vector<uint8_t>& mapPointFlags, const std::vector<float>& x3Dw,
                                      const std::vector<float>& minDistance, const std::vector<float>& maxDistance,
                                      const std::vector<uint8_t>& mapPointDescriptors, const std::vector<uint8_t>* occupied,
                                      std::vector<int>& matchCur, const bool gemmFloat = false) {
        static_assert(sizeof(int) == sizeof(int32_t), "the results are handed over as int32");
        const size_t n = keyFrameKeys.size();
        if (mapPointFlags.size() != n || x3Dw.size() != 3 * n || minDistance.size() != n || maxDistance.size() != n ||
            mapPointDescriptors.size() != 32 * n)
            throw std::invalid_argument("SearchByProjectionKeyFrameKB8: one flag, position, range and descriptor per entry");
        vslam_proj_params p;
        std::memset(&p, 0, sizeof(p));
        std::memcpy(p.Tcw, Tcw, sizeof(p.Tcw));
        p.fx = camera.fx; p.fy = camera.fy; p.cx = camera.cx; p.cy = camera.cy;
        p.th = th;
        p.check_orientation = mbCheckOrientation ? 1 : 0;
        p.img_w = imgW;
        p.img_h = imgH;
        p.gemm_float = gemmFloat ? 1 : 0;
        const vslam_kp* dk = nullptr;
        const uint8_t* dd = nullptr;
        int nCur = 0;
        check(vslam_fe_slot_buffers(extractor.context(), 0, &dk, &dd, &nCur));
        if (occupied && occupied->size() != (size_t)nCur)
            throw std::invalid_argument("SearchByProjectionKeyFrameKB8: one occupancy byte per current keypoint");
        matchCur.assign((size_t)nCur, -1);
        int nm = 0;
        check(vslam_search_by_projection_keyframe_kb8(extractor.context(), &p, Ow, logScaleFactor, ORBdist,
                                                      reinterpret_cast<const vslam_kp*>(keyFrameKeys.data()), (int)n,
                                                      mapPointFlags.data(), x3Dw.data(), minDistance.data(), maxDistance.data(),
                                                      mapPointDescriptors.data(), dk, dd, nCur, occupied ? occupied->data() : nullptr,
                                                      matchCur.data(), &nm));
        return nm;
    }

    /* LoopClosing::FindMatchesByProjection's batch (loopclosing.cpp:668-684, :751-803) for fisheye KeyFrames: ONE list of
     * MapPoints -- those of pMostBoWMatchesKF, of its covisibles and of theirs -- against the covisible KeyFrames as jobs, each
     * one call of SearchByProjection(pKFj, Sjw, vpMapPoints, vpMatched, th, ratioHamming) (fmatcher.cpp:750-863).  A job is a
     * vslam_sim3_kb8_job (include/vslam_fe.h): Rcw / tcw / Ow derived from Sjw, pKFj's left keypoints and descriptor rows in HBM,
     * vpMatched != NULL bytes, !spAlreadyFound bytes.  Any number of jobs: 16 per enqueue.  hostJobs (may be NULL): the same jobs
     * with dev_kps / dev_desc pointing at HOST copies; a job whose survivors exceed the device's 4096 (nmatches -1) is then run by
     * the host twin, and without them the refusal is thrown.  camera: mpCamera's parameters, for the twin.
     * matchKf[j][idx] = iMP (vpMatched[idx] = vpMapPoints[iMP]) or -1; nmatches[j]; nGated[j] = points behind the gates. */
    void FindMatchesByProjectionKB8(FExtractor& extractor, const vslam_kb8_camera& camera,
                                    const std::vector<vslam_sim3_kb8_job>& jobs, const std::vector<vslam_sim3_kb8_job>* hostJobs,
                                    const std::vector<vslam_fuse_point>& points, const std::vector<uint8_t>& mapPointDescriptors,
                                    const int th, const float ratioHamming, const float logScaleFactor, const int imgW,
                                    const int imgH, std::vector<std::vector<int>>& matchKf, std::vector<int>& nmatches,
                                    std::vector<int>& nGated, const bool gemmFloat = false) {
        static_assert(sizeof(int) == sizeof(int32_t), "the results are handed over as int32");
        if (mapPointDescriptors.size() != 32 * points.size())
            throw std::invalid_argument("FindMatchesByProjectionKB8: one descriptor per MapPoint");
        if (hostJobs && hostJobs->size() != jobs.size())
            throw std::invalid_argument("FindMatchesByProjectionKB8: one host job per job");
        vslam_sim3_kb8_params p;
        std::memset(&p, 0, sizeof(p));
        p.th = th;
        p.ratio_hamming = ratioHamming;
        p.log_scale_factor = logScaleFactor;
        p.img_w = imgW;
        p.img_h = imgH;
        p.gemm_float = gemmFloat ? 1 : 0;
        matchKf.assign(jobs.size(), std::vector<int>());
        nmatches.assign(jobs.size(), 0);
        nGated.assign(jobs.size(), 0);
        std::vector<int32_t*> out(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) {
            matchKf[j].assign((size_t)std::max(jobs[j].n_kf, 0), -1);
            out[j] = matchKf[j].data();
        }
        for (size_t first = 0; first < jobs.size(); first += VSLAM_SIM3_KB8_MAX_JOBS) {
            const int K = (int)std::min<size_t>(VSLAM_SIM3_KB8_MAX_JOBS, jobs.size() - first);
            const int rc = vslam_search_by_projection_sim3_kb8(extractor.context(), &p, jobs.data() + first, K, points.data(),
                                                               mapPointDescriptors.data(), (int)points.size(), VSLAM_IMGS_HOST,
                                                               out.data() + first, nmatches.data() + first, nGated.data() + first);
            if (rc != VSLAM_ERR_UNSUPPORTED || !hostJobs) check(rc);
            if (rc != VSLAM_ERR_UNSUPPORTED) continue;
            const std::vector<float> sf = extractor.GetScaleFactors();
            vslam_bounds b;
            int is_set = 0;
            check(vslam_fe_get_grid_bounds(extractor.context(), &b, &is_set));
            const float bounds[4] = {is_set ? b.min_x : 0.0f, is_set ? b.max_x : (float)imgW, is_set ? b.min_y : 0.0f,
                                     is_set ? b.max_y : (float)imgH};
            bool any = false;
            for (size_t j = first; j < first + (size_t)K; j++) {
                if (nmatches[j] != -1) continue; /* delivered */
                any = true;
                check(vslamh_search_by_projection_sim3_kb8(&p, &camera, hostJobs->data() + j, 1, points.data(),
                                                           mapPointDescriptors.data(), (int)points.size(), sf.data(),
                                                           (int)sf.size(), bounds, out.data() + j, nmatches.data() + j,
                                                           nGated.data() + j));
            }
            if (!any) check(rc); /* refused as a whole: a KeyFrame or a list beyond the limits */
        }
    }

    /* ONE (job, point) search on the host with the same parameters as FuseSearchRig: what FuseWalk's searchOne calls for a
     * MapPoint whose descriptor was recomputed.  hostJob: the job with dev_kps / dev_desc pointing at HOST copies of the side's
     * keypoints and descriptor rows (valid_host is not read: one point, asked about by the walk already); camera: mpCamera's
     * parameters; descriptor: the MapPoint's 32 bytes of now.  Scale tables and grid bounds come from the extractor's context. */
    static void FuseSearchOneHost(FExtractor& extractor, const vslam_kb8_camera& camera, const vslam_kb8_rig* rig,
                                  const vslam_fuse_rig_job& hostJob, const vslam_fuse_point& point, const uint8_t* descriptor,
                                  const float th, const float logScaleFactor, const int imgW, const int imgH, int& bestIdx,
                                  int& bestDist, const bool gemmFloat = false) {
        vslam_fuse_params p;
        std::memset(&p, 0, sizeof(p));
        p.th = th;
        p.log_scale_factor = logScaleFactor;
        p.img_w = imgW;
        p.img_h = imgH;
        p.gemm_float = gemmFloat ? 1 : 0;
        vslam_fuse_rig_job job = hostJob;
        job.valid_host = nullptr;
        const std::vector<float> sf = extractor.GetScaleFactors(), is2 = extractor.GetInverseScaleSigmaSquares();
        vslam_bounds b;
        int is_set = 0;
        check(vslam_fe_get_grid_bounds(extractor.context(), &b, &is_set));
        const float bounds[4] = {is_set ? b.min_x : 0.0f, is_set ? b.max_x : (float)imgW, is_set ? b.min_y : 0.0f,
                                 is_set ? b.max_y : (float)imgH};
        int32_t oi = -1, od = 256;
        check(vslamh_fuse_search_rig(&p, &camera, rig, &job, 1, &point, descriptor, 1, sf.data(), is2.data(), (int)sf.size(), bounds,
                                     &oi, &od));
        bestIdx = oi;
        bestDist = od;
    }

    /* The walk over the results of FuseSearchRig that makes the caller's map equal to the one the reference's sequential calls
     * leave ("Fuse for a rig").  Jobs in the reference's call order (the left job of a KeyFrame before its right
     * job), points in order.  At each (job, point):
     *   - isBad(point) or isInKeyFrame(job, point) holds NOW: skip (both only ever flip towards "skip")
     *   - descriptorRecomputed(point) -- the point survived a Replace earlier in this walk, so ComputeDistinctiveDescriptors ran
     *     (mappoint.cpp:292): the batch result is stale; searchOne(job, point, idx, dist) redoes this one search with the
     *     descriptor of now (vslamh_fuse_search_rig with one job and one point, or a one-job device call)
     *   - bestDist <= TH_LOW: fuse(job, point, bestIdx), the reference's :2093-2112; it may Replace either way
     * A point that fused in the left job is in the KeyFrame or bad, so the right job of the same KeyFrame skips it: a stale
     * descriptor only ever matters across KeyFrames.  Returns nFused summed over the jobs. */
    template <class IsBad, class IsInKeyFrame, class DescriptorRecomputed, class SearchOne, class Fuse>
    static int FuseWalk(const size_t nJobs, const size_t nPoints, const std::vector<int>& bestIdx, const std::vector<int>& bestDist,
                        IsBad isBad, IsInKeyFrame isInKeyFrame, DescriptorRecomputed descriptorRecomputed, SearchOne searchOne,
                        Fuse fuse) {
        if (bestIdx.size() != nJobs * nPoints || bestDist.size() != nJobs * nPoints)
            throw std::invalid_argument("FuseWalk: nJobs * nPoints results");
        const int TH_LOW = 50;
        int nFused = 0;
        for (size_t j = 0; j < nJobs; j++)
            for (size_t i = 0; i < nPoints; i++) {
                if (isBad(i) || isInKeyFrame(j, i)) continue;
                int idx = bestIdx[j * nPoints + i], dist = bestDist[j * nPoints + i];
                if (descriptorRecomputed(i)) searchOne(j, i, idx, dist);
                if (idx < 0 || dist > TH_LOW) continue;
                fuse(j, i, idx);
                nFused++;
            }
        return nFused;
    }

protected:
    /* the current frame's keypoints for the projection matchers: keypoints_ of slot 0 as before, ukeypoints_ once the
     * context holds grid bounds (SetGridBounds) -- the undistorted grid bins undistorted keypoints */
    static void slot_keypoints(const FExtractor& e, const vslam_kp** dk, const uint8_t** dd, int* n) {
        check(vslam_fe_slot_buffers(e.context(), 0, dk, dd, n));
        vslam_bounds b;
        int is_set = 0;
        check(vslam_fe_get_grid_bounds(e.context(), &b, &is_set));
        if (is_set && e.HasCamera()) check(vslam_fe_slot_ukps(e.context(), 0, dk));
    }

    float mfNNratio;
    bool mbCheckOrientation;
};

/* Frame::ComputeStereoMatches (frame.cpp:823-997): fills mvuRight / mvDepth (size N = left keypoints) from the
 * last frames processed by the two extractors (the reference's mpORBextractorLeft / Right). */
inline void ComputeStereoMatches(const FExtractor& left, const FExtractor& right, float mbf, float fx, int N,
                                 std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    mvuRight.assign(N, -1.0f);
    mvDepth.assign(N, -1.0f);
    if (N == 0) return;
    check(vslam_stereo_match(left.context(), 0, right.context(), 0, mbf, fx, mvuRight.data(), mvDepth.data()));
}

/* ---------------------------------------------------------------------------------------------------
 * geometry::KannalaBrandt8 (cameramodels/kannalabrandt8.h): the fisheye camera of a Frame whose extractor is `extractor`.
 * Constructed from the reference's mvParameters (fx, fy, cx, cy, k0..k3) it becomes the context's camera: project /
 * unproject run on the device with the host libm's results bit for bit, and FMatcher::SearchLocalPoints on that extractor
 * tests the frustum with this projection (its LocalFrameView carries the same fx, fy, cx, cy).  The matchers that project
 * with intrinsics of their own throw while it is attached (VSLAM_ERR_UNSUPPORTED).  Detach() or the destructor returns the
 * context to pinhole.  The extractor must have processed an image (the context is created by the first one).
 *     KannalaBrandt8 cam(extractor, vParameters);
 *     cv::Point2f uv = cam.project(p3D);   cam.unproject(keys, rays);   cam.unprojectSlotAsync(dev_rays);
 * Not here: projectJac, TriangulateMatches / epipolarConstrain (cv::SVD), ReconstructWithTwoViews
 * (cv::fisheye::undistortPoints).
 * ------------------------------------------------------------------------------------------------- */
#ifdef VSLAM_SHIM_WITH_OPENCV
typedef cv::Point3f Point3f;
#else
struct Point3f {
    float x, y, z;
};
#endif
static_assert(sizeof(Point3f) == 12 && sizeof(Point2f) == 8, "vectors of points are packed floats");

class KannalaBrandt8 {
public:
    KannalaBrandt8(const FExtractor& extractor, const std::vector<float>& vParameters, float precision = 1e-6f)
        : extractor_(&extractor) {
        if (vParameters.size() != 8) throw std::invalid_argument("KannalaBrandt8: 8 parameters (fx, fy, cx, cy, k0..k3)");
        if (!extractor.context()) throw std::runtime_error("KannalaBrandt8: the extractor has not processed an image yet");
        cam_.fx = vParameters[0]; cam_.fy = vParameters[1]; cam_.cx = vParameters[2]; cam_.cy = vParameters[3];
        for (int i = 0; i < 4; i++) cam_.k[i] = vParameters[4 + i];
        cam_.precision = precision;
        check(vslam_fe_set_kb8_camera(extractor.context(), &cam_));
        attached_ = true;
    }
    ~KannalaBrandt8() {
        if (attached_) (void)vslam_fe_set_kb8_camera(extractor_->context(), nullptr);
    }
    KannalaBrandt8(const KannalaBrandt8&) = delete;
    KannalaBrandt8& operator=(const KannalaBrandt8&) = delete;
    void Detach() {
        if (attached_) check(vslam_fe_set_kb8_camera(extractor_->context(), nullptr));
        attached_ = false;
    }
    const vslam_kb8_camera& parameters() const { return cam_; }

    void project(const std::vector<Point3f>& p3D, std::vector<Point2f>& uv) const {
        uv.resize(p3D.size());
        check(vslam_kb8_project(extractor_->context(), reinterpret_cast<const float*>(p3D.data()), (int)p3D.size(),
                                reinterpret_cast<float*>(uv.data())));
    }
    Point2f project(const Point3f& p3D) const {
        Point2f uv;
        check(vslam_kb8_project(extractor_->context(), &p3D.x, 1, &uv.x));
        return uv;
    }
    void unproject(const std::vector<Point2f>& p2D, std::vector<Point3f>& rays) const {
        rays.resize(p2D.size());
        check(vslam_kb8_unproject(extractor_->context(), reinterpret_cast<const float*>(p2D.data()), (int)p2D.size(),
                                  reinterpret_cast<float*>(rays.data())));
    }
    Point3f unproject(const Point2f& p2D) const {
        Point3f r;
        check(vslam_kb8_unproject(extractor_->context(), &p2D.x, 1, &r.x));
        return r;
    }
    /* the rays of the keypoints of the extractor's last image into DEVICE memory of 3 * vslam_fe_capacity floats; enqueued,
     * not waited for */
    void unprojectSlotAsync(float* dev_rays) const { check(vslam_kb8_unproject_slot_async(extractor_->context(), 0, dev_rays)); }
    /* Frame::isInFrustum of a two-fisheye rig (Nleft != -1) over a local map: this camera is the left one.  Returns the number
     * of points either camera sees. */
    int isInFrustumRig(const vslam_frustum_params& p, const vslam_kb8_rig& rig, const std::vector<vslam_map_point>& points,
                       std::vector<vslam_mp_track>& left, std::vector<vslam_mp_track>& right) const {
        left.resize(points.size());
        right.resize(points.size());
        int n = 0;
        check(vslam_frame_in_frustum_rig(extractor_->context(), &p, &rig, points.data(), (int)points.size(), left.data(),
                                         right.data(), nullptr, nullptr, &n));
        return n;
    }

private:
    const FExtractor* extractor_;
    vslam_kb8_camera cam_;
    bool attached_ = false;
};

/* ---------------------------------------------------------------------------------------------------
 * The scoring half of MotionEstimator::Reconstruct (motion_estimation.cpp:2006-2094).  FindHomography and FindFundamental
 * (:2096-2195) split in two: loop one stays in the caller and computes every H21i = T2inv*Hn*T1, H12i = H21i.inv() and
 * F21i = T2t*Fn*T1 (ComputeH21 / ComputeF21 run cv::SVDecomp, which this library does not restate); then ONE call scores
 * all of them over all matches and selects, as loop two and the two threads of the reference do:
 *
 *     MotionEstimator me(extractor, mSigma);
 *     me.Check(vKeys1, vKeys2, vMatches12, vH21, vH12, vF21, out);       // CheckHomographies + CheckFundamentals
 *     if (out.SH + out.SF == 0.f) return false;
 *     float RH = out.SH / (out.SH + out.SF);                             // :2078-2093 as before, with
 *     ... ReconstructH(out.vbMatchesInliersH, vH21[out.bestH], ...)  or  ReconstructF(out.vbMatchesInliersF, vF21[out.bestF], ...)
 *
 * A model is 9 floats row-major (Mat3f); with VSLAM_SHIM_WITH_OPENCV the overloads take std::vector<cv::Mat> of 3 x 3
 * CV_32F.  The extractor only lends its device context and stream; it must have processed an image.
 * ------------------------------------------------------------------------------------------------- */
struct Mat3f {
    float v[9];
};
static_assert(sizeof(Mat3f) == 36, "a vector of Mat3f is n x 9 packed floats");

class MotionEstimator {
public:
    struct Consensus {
        float SH = 0.0f, SF = 0.0f;                                /* score of FindHomography / FindFundamental */
        int bestH = -1, bestF = -1;                                /* index of H21 / F21 among the hypotheses, -1: none */
        std::vector<std::pair<int, int>> mvMatches12;              /* (index in frame 1, index in frame 2) */
        std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;    /* over mvMatches12; all false without a winner */
        std::vector<float> vScoresH, vScoresF;                     /* currentScore of every iteration */
    };

    explicit MotionEstimator(const FExtractor& extractor, float sigma = 1.0f) : extractor_(&extractor), mSigma(sigma) {}

    void Check(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
               const std::vector<Mat3f>& vH21, const std::vector<Mat3f>& vH12, const std::vector<Mat3f>& vF21,
               Consensus& out) const {
        if (!extractor_->context()) throw std::runtime_error("MotionEstimator: the extractor has not processed an image yet");
        if (vH21.size() != vH12.size() || vMatches12.size() != vKeys1.size())
            throw std::runtime_error("MotionEstimator: vH21 / vH12 or vMatches12 / vKeys1 differ in length");
        vslam_two_view_job job;
        std::memset(&job, 0, sizeof(job));
        job.kps1 = reinterpret_cast<const vslam_kp*>(vKeys1.data());
        job.kps2 = reinterpret_cast<const vslam_kp*>(vKeys2.data());
        job.n1 = (int32_t)vKeys1.size();
        job.n2 = (int32_t)vKeys2.size();
        job.matches12 = vMatches12.data();
        job.H21 = vH21.empty() ? nullptr : vH21[0].v;
        job.H12 = vH12.empty() ? nullptr : vH12[0].v;
        job.nH = (int32_t)vH21.size();
        job.F21 = vF21.empty() ? nullptr : vF21[0].v;
        job.nF = (int32_t)vF21.size();
        job.sigma = mSigma;
        const size_t cap = vKeys1.size() < (size_t)VSLAM_TWO_VIEW_MAX_PAIRS ? vKeys1.size() : (size_t)VSLAM_TWO_VIEW_MAX_PAIRS;
        std::vector<int32_t> pairs(2 * cap + 2);
        std::vector<uint8_t> inH(cap + 1), inF(cap + 1);
        out.vScoresH.assign(vH21.size(), 0.0f);
        out.vScoresF.assign(vF21.size(), 0.0f);
        vslam_two_view_result res;
        std::memset(&res, 0, sizeof(res));
        res.pairs = pairs.data();
        res.scores_h = out.vScoresH.empty() ? nullptr : out.vScoresH.data();
        res.scores_f = out.vScoresF.empty() ? nullptr : out.vScoresF.data();
        res.inliers_h = inH.data();
        res.inliers_f = inF.data();
        check(vslam_two_view_score(extractor_->context(), &job, &res));
        out.SH = res.score_h;
        out.SF = res.score_f;
        out.bestH = res.best_h;
        out.bestF = res.best_f;
        out.mvMatches12.resize((size_t)res.n_pairs);
        out.vbMatchesInliersH.assign((size_t)res.n_pairs, false);
        out.vbMatchesInliersF.assign((size_t)res.n_pairs, false);
        for (int i = 0; i < res.n_pairs; i++) {
            out.mvMatches12[i] = std::make_pair((int)pairs[2 * i], (int)pairs[2 * i + 1]);
            out.vbMatchesInliersH[i] = inH[i] != 0;
            out.vbMatchesInliersF[i] = inF[i] != 0;
        }
    }

    /* one model only: the loop of FindHomography, or of FindFundamental */
    void CheckHomographies(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2,
                           const std::vector<int>& vMatches12, const std::vector<Mat3f>& vH21, const std::vector<Mat3f>& vH12,
                           Consensus& out) const {
        Check(vKeys1, vKeys2, vMatches12, vH21, vH12, std::vector<Mat3f>(), out);
    }
    void CheckFundamentals(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2,
                           const std::vector<int>& vMatches12, const std::vector<Mat3f>& vF21, Consensus& out) const {
        Check(vKeys1, vKeys2, vMatches12, std::vector<Mat3f>(), std::vector<Mat3f>(), vF21, out);
    }

#ifdef VSLAM_SHIM_WITH_OPENCV
    static std::vector<Mat3f> pack(const std::vector<cv::Mat>& v) {
        std::vector<Mat3f> out(v.size());
        for (size_t k = 0; k < v.size(); k++) {
            CV_Assert(v[k].rows == 3 && v[k].cols == 3 && v[k].type() == CV_32F);
            for (int i = 0; i < 9; i++) out[k].v[i] = v[k].at<float>(i / 3, i % 3);
        }
        return out;
    }
    void CheckHomographies(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2,
                           const std::vector<int>& vMatches12, const std::vector<cv::Mat>& vH21,
                           const std::vector<cv::Mat>& vH12, Consensus& out) const {
        CheckHomographies(vKeys1, vKeys2, vMatches12, pack(vH21), pack(vH12), out);
    }
    void CheckFundamentals(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2,
                           const std::vector<int>& vMatches12, const std::vector<cv::Mat>& vF21, Consensus& out) const {
        CheckFundamentals(vKeys1, vKeys2, vMatches12, pack(vF21), out);
    }
    void Check(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
               const std::vector<cv::Mat>& vH21, const std::vector<cv::Mat>& vH12, const std::vector<cv::Mat>& vF21,
               Consensus& out) const {
        Check(vKeys1, vKeys2, vMatches12, pack(vH21), pack(vH12), pack(vF21), out);
    }
#endif

private:
    const FExtractor* extractor_;
    float mSigma;
};

/* ---------------------------------------------------------------------------------------------------
 * The grid FAST detector of fast_cuda.h:19-25 / fast_cuda.cpp:70-132.  FASTGPU carries vilib::FASTGPU's
 * constructor (fast_gpu.h:46-56) and DetectorBase's read side (detector_base.h:48-57,75-80): detect() on an
 * 8-bit image replaces `Frame(image, 0, levels)` + `detect(frame->pyramid_)`; getPoints() holds one FeaturePoint
 * per grid cell and isOccupied(i) says whether cell i found a corner (OccupancyGrid2D::isOccupied).
 * FAST::detect is the reference's wrapper with its fixed parameters (fast_cuda.cpp:24-39: one level, 32x32
 * cells, epsilon 10, arc 10, SUM_OF_ABS_DIFF_ON_ARC); unlike the reference, which prints the grid and leaves
 * `keypoints` empty, it returns the occupied cells as key points (pt, response = score, octave = level).
 * ------------------------------------------------------------------------------------------------- */
namespace detail {
/* DetectorBase's read side (detector_base.h:48-57,75-80) and the buffers a detect() call fills, for FASTGPU and HarrisGPU */
class GridDetectorBase {
public:
    struct FeaturePoint {
        double x_, y_, score_;
        unsigned int level_;
    };
    void reset() { /* DetectorBase::reset + the constructor's keypoints_ fill (detector_base.cpp:67,76-84) */
        keypoints_.assign(n_cols_ * n_rows_, FeaturePoint{0.0, 0.0, 0.0, (unsigned int)-1});
        occupied_.assign(n_cols_ * n_rows_, 0);
    }
    const std::vector<FeaturePoint>& getPoints() const { return keypoints_; }
    bool isOccupied(std::size_t i) const { return occupied_[i] != 0; }
    std::size_t count() const {
        std::size_t c = 0;
        for (uint8_t o : occupied_) c += o;
        return c;
    }
    std::size_t getCellCountHorizontal() const { return n_cols_; }
    std::size_t getCellCountVertical() const { return n_rows_; }
    /* what FeatureTrackerGPU::setDetectorGPU binds to: the C handle and which of VSLAM_FT_DETECTOR_* it is */
    void* handle() const { return handle_; }
    int kind() const { return kind_; }
    /* how many image slots the detector's launch can take: the cameras of a FeatureTrackerGPU bound to it */
    std::size_t max_batch() const { return max_batch_; }

protected:
    GridDetectorBase() {}
    GridDetectorBase(const GridDetectorBase&) = delete;
    GridDetectorBase& operator=(const GridDetectorBase&) = delete;
    /* the fields every vslam_*_params has; the reference's tie order.  detect() takes one image per call; max_batch > 1
     * is for a FeatureTrackerGPU of several cameras */
    template <class P>
    void fill_common(P& p, std::size_t image_width, std::size_t image_height, std::size_t cell_size_width,
                     std::size_t cell_size_height, std::size_t min_level, std::size_t max_level,
                     std::size_t horizontal_border, std::size_t vertical_border, int device, int max_batch) {
        std::memset(&p, 0, sizeof(p));
        p.image_width = (int32_t)image_width;
        p.image_height = (int32_t)image_height;
        p.cell_size_width = (int32_t)cell_size_width;
        p.cell_size_height = (int32_t)cell_size_height;
        p.min_level = (int32_t)min_level;
        p.max_level = (int32_t)max_level;
        p.horizontal_border = (int32_t)horizontal_border;
        p.vertical_border = (int32_t)vertical_border;
        p.tie_rule = 0;
        p.device = device;
        p.max_batch = max_batch;
        max_batch_ = (std::size_t)(max_batch > 0 ? max_batch : 0);
    }
    void set_grid(int n_cols, int n_rows) {
        n_cols_ = (std::size_t)n_cols;
        n_rows_ = (std::size_t)n_rows;
        pos_.resize(2 * n_cols_ * n_rows_);
        score_.resize(n_cols_ * n_rows_);
        level_.resize(n_cols_ * n_rows_);
        reset();
    }
    void occupy(std::size_t i) { /* cell i of the last grid is a feature */
        keypoints_[i] = FeaturePoint{(double)pos_[2 * i], (double)pos_[2 * i + 1], (double)score_[i], (unsigned int)level_[i]};
        occupied_[i] = 1;
    }
    void* handle_ = nullptr;
    int kind_ = VSLAM_FT_DETECTOR_FAST;
    std::size_t n_cols_ = 0, n_rows_ = 0, max_batch_ = 1;
    std::vector<FeaturePoint> keypoints_;
    std::vector<uint8_t> occupied_;
    std::vector<float> pos_, score_;
    std::vector<int32_t> level_;
};
} /* namespace detail */

class FASTGPU : public detail::GridDetectorBase {
public:
    FASTGPU(std::size_t image_width, std::size_t image_height, std::size_t cell_size_width, std::size_t cell_size_height,
            std::size_t min_level, std::size_t max_level, std::size_t horizontal_border, std::size_t vertical_border,
            float threshold, int min_arc_length, int score, int device = 0, int max_batch = 1) {
        vslam_fg_params p;
        fill_common(p, image_width, image_height, cell_size_width, cell_size_height, min_level, max_level, horizontal_border,
                    vertical_border, device, max_batch);
        p.threshold = threshold;
        p.min_arc_length = min_arc_length;
        p.score = score;
        check(vslam_fg_create(&p, &fg_));
        handle_ = fg_;
        int nc = 0, nr = 0;
        vslam_fg_grid(fg_, &nc, &nr);
        set_grid(nc, nr);
    }
    ~FASTGPU() { vslam_fg_destroy(fg_); }

    void detect(const uint8_t* image, std::size_t pitch) { /* detectBase + processGrid, detector_base_gpu.cpp:204-218 */
        check(vslam_fg_detect(fg_, image, pitch, pos_.data(), score_.data(), level_.data()));
        for (std::size_t i = 0; i < score_.size(); i++)
            if (score_[i] > 0.0f) occupy(i);
    }

private:
    vslam_fg* fg_ = nullptr;
};

class FAST {
public:
    /* image: 8-bit grey (the reference converts BGR first, fast_cuda.cpp:45-47) */
    void detect(const uint8_t* image, int width, int height, std::size_t pitch, std::vector<KeyPoint>& keypoints) {
        if (!det_ || w_ != width || h_ != height) {
            det_.reset(new FASTGPU((std::size_t)width, (std::size_t)height, 32, 32, 0, 1, 0, 0, 10.0f, 10,
                                   VSLAM_FG_SUM_OF_ABS_DIFF_ON_ARC));
            w_ = width;
            h_ = height;
        }
        det_->reset();
        det_->detect(image, pitch);
        keypoints.clear();
        const std::vector<FASTGPU::FeaturePoint>& pts = det_->getPoints();
        for (std::size_t i = 0; i < pts.size(); i++) {
            if (!det_->isOccupied(i)) continue;
            KeyPoint k;
            std::memset(&k, 0, sizeof(k));
            k.pt.x = (float)pts[i].x_;
            k.pt.y = (float)pts[i].y_;
            k.size = 7.0f;
            k.angle = -1.0f;
            k.response = (float)pts[i].score_;
            k.octave = (int)pts[i].level_;
            k.class_id = -1;
            keypoints.push_back(k);
        }
    }
    const FASTGPU* detector() const { return det_.get(); }

private:
    std::unique_ptr<FASTGPU> det_;
    int w_ = 0, h_ = 0;
};

/* ---------------------------------------------------------------------------------------------------
 * The grid Harris / Shi-Tomasi detector, the sibling of FASTGPU over the same DetectorBaseGPU.  HarrisGPU carries
 * vilib::HarrisGPU's constructor (harris_gpu.h; harris_gpu.cpp:63-74) and DetectorBase's read side: detect() on an
 * 8-bit image replaces `Frame(image, 0, levels)` + `detect(frame->pyramid_)` and ends, as the reference's does, in
 * processGridAndThreshold(quality_level) (detector_base_gpu.cpp:228-248): getPoints() holds one FeaturePoint per grid
 * cell and isOccupied(i) says whether cell i scored above max score * quality_level.
 * ------------------------------------------------------------------------------------------------- */
typedef int conv_filter_border_type_t; /* VSLAM_HG_BORDER_*: vilib::conv_filter_border_type in its order */

class HarrisGPU : public detail::GridDetectorBase {
public:
    HarrisGPU(std::size_t image_width, std::size_t image_height, std::size_t cell_size_width, std::size_t cell_size_height,
              std::size_t min_level, std::size_t max_level, std::size_t horizontal_border, std::size_t vertical_border,
              conv_filter_border_type_t filter_border_type, bool use_harris, float harris_k, float quality_level,
              int device = 0, int max_batch = 1) {
        vslam_hg_params p;
        fill_common(p, image_width, image_height, cell_size_width, cell_size_height, min_level, max_level, horizontal_border,
                    vertical_border, device, max_batch);
        p.filter_border_type = filter_border_type;
        p.use_harris = use_harris ? 1 : 0;
        p.harris_k = harris_k;
        p.quality_level = quality_level;
        check(vslam_hg_create(&p, &hg_));
        handle_ = hg_;
        kind_ = VSLAM_FT_DETECTOR_HARRIS;
        int nc = 0, nr = 0;
        vslam_hg_grid(hg_, &nc, &nr);
        set_grid(nc, nr);
        keep_.resize(score_.size());
    }
    ~HarrisGPU() { vslam_hg_destroy(hg_); }

    void detect(const uint8_t* image, std::size_t pitch) { /* detectBase + processGridAndThreshold, harris_gpu.cpp:195-198 */
        int32_t n_keep = 0;
        check(vslam_hg_detect(hg_, image, pitch, pos_.data(), score_.data(), level_.data(), keep_.data(), &n_keep));
        for (std::size_t i = 0; i < keep_.size(); i++)
            if (keep_[i]) occupy(i);
    }

private:
    vslam_hg* hg_ = nullptr;
    std::vector<uint8_t> keep_;
};

/* ---------------------------------------------------------------------------------------------------
 * The pyramidal Lucas-Kanade feature tracker, the one consumer of the two grid detectors.  FeatureTrackerGPU carries
 * vilib::FeatureTrackerGPU's constructor options (feature_tracker_options.h:50-98) and its methods
 * (feature_tracker_gpu.h, feature_tracker_base.h): setDetectorGPU, track, reset, setBestNFeatures,
 * setMinTracksToDetect, getDisparity.  track() on 8-bit images, one per camera, replaces `Frame(image, 0, pyramid_levels)`
 * per camera of a FrameBundle + `track(bundle, tracked, detected)`; the form on one image is the bundle of one.
 * feature(i, camera_id) is what the reference leaves in that camera's frame (px_vec_, score_vec_, level_vec_,
 * track_id_vec_ up to num_features_).  The cameras of a tracker bind ONE detector object (one image size, one grid, one
 * stream) whose max_batch is at least camera_num; a rig whose cameras differ in image size is several trackers.
 * ------------------------------------------------------------------------------------------------- */
struct FeatureTrackerOptions {
    int klt_max_level = 4;
    int klt_min_level = 0;
    std::vector<int> klt_patch_sizes = {16, 16, 16, 8, 8};
    int klt_max_iter = VSLAM_FT_MAX_ITER; /* a compile-time constant, as in the reference */
    double klt_min_update_squared = 0.0005;
    std::size_t min_tracks_to_detect_new_features = 100;
    bool reset_before_detection = true;
    int use_best_n_features = -1;
    bool klt_template_is_first_observation = true;
    bool affine_est_offset = false;
    bool affine_est_gain = false;
    int pyramid_levels = 5; /* vilib::Frame's n_pyr_levels */
};

class FeatureTrackerGPU {
public:
    explicit FeatureTrackerGPU(const FeatureTrackerOptions& options, const std::size_t& camera_num = 1)
        : options_(options), camera_num_(camera_num), bound_(camera_num) {
        if (camera_num < 1) throw std::invalid_argument("FeatureTrackerGPU: at least one camera");
    }
    ~FeatureTrackerGPU() { vslam_ft_destroy(ft_); }
    FeatureTrackerGPU(const FeatureTrackerGPU&) = delete;
    FeatureTrackerGPU& operator=(const FeatureTrackerGPU&) = delete;

    /* The tracker shares the detector's stream and keeps the detector alive.  Every camera binds the same detector
     * object; the tracker exists once the last camera is bound (binding one again builds it anew). */
    void setDetectorGPU(const std::shared_ptr<detail::GridDetectorBase>& detector, const std::size_t& camera_id = 0) {
        if (camera_id >= camera_num_ || !detector) throw std::invalid_argument("FeatureTrackerGPU::setDetectorGPU");
        if (detector->max_batch() < camera_num_)
            throw std::invalid_argument("FeatureTrackerGPU::setDetectorGPU: the detector's max_batch is below camera_num");
        for (std::size_t c = 0; c < camera_num_; c++)
            if (c != camera_id && bound_[c] && bound_[c] != detector)
                throw std::invalid_argument("FeatureTrackerGPU::setDetectorGPU: the cameras of a tracker share one detector object");
        bound_[camera_id] = detector;
        for (const std::shared_ptr<detail::GridDetectorBase>& d : bound_)
            if (!d) return;
        vslam_ft_destroy(ft_);
        ft_ = nullptr;
        vslam_ft_params p;
        std::memset(&p, 0, sizeof(p));
        p.klt_min_level = options_.klt_min_level;
        p.klt_max_level = options_.klt_max_level;
        for (std::size_t i = 0; i < options_.klt_patch_sizes.size() && i < VSLAM_FT_MAX_LEVELS; i++)
            p.klt_patch_sizes[i] = options_.klt_patch_sizes[i];
        p.klt_min_update_squared = (float)options_.klt_min_update_squared;
        p.min_tracks_to_detect_new_features = (int32_t)options_.min_tracks_to_detect_new_features;
        p.reset_before_detection = options_.reset_before_detection ? 1 : 0;
        p.use_best_n_features = options_.use_best_n_features;
        p.klt_template_is_first_observation = options_.klt_template_is_first_observation ? 1 : 0;
        p.affine_est_offset = options_.affine_est_offset ? 1 : 0;
        p.affine_est_gain = options_.affine_est_gain ? 1 : 0;
        p.pyramid_levels = options_.pyramid_levels;
        check(vslam_ft_create_bundle(&p, detector->kind(), detector->handle(), (int)camera_num_, &ft_));
        features_.assign(camera_num_, std::vector<vslam_ft_feature>((std::size_t)vslam_ft_capacity(ft_)));
        n_features_.assign(camera_num_, 0);
    }

    /* one image per camera, all of one pitch; the two totals are the reference's, summed over the cameras */
    void track(const std::vector<const uint8_t*>& images, std::size_t pitch, std::size_t& total_tracked_features_num,
               std::size_t& total_detected_features_num) {
        if (images.size() != camera_num_) throw std::invalid_argument("FeatureTrackerGPU::track: one image per camera");
        std::vector<int32_t> tracked(camera_num_, 0), detected(camera_num_, 0);
        check(vslam_ft_track_bundle(ft_, images.data(), pitch, 0, tracked.data(), detected.data()));
        total_tracked_features_num = total_detected_features_num = 0;
        for (std::size_t c = 0; c < camera_num_; c++) {
            int n = 0;
            check(vslam_ft_features_cam(ft_, (int)c, features_[c].data(), (int)features_[c].size(), &n));
            n_features_[c] = (std::size_t)n;
            total_tracked_features_num += (std::size_t)tracked[c];
            total_detected_features_num += (std::size_t)detected[c];
        }
    }
    void track(const uint8_t* image, std::size_t pitch, std::size_t& total_tracked_features_num, std::size_t& total_detected_features_num) {
        track(std::vector<const uint8_t*>(1, image), pitch, total_tracked_features_num, total_detected_features_num);
    }
    void reset() { check(vslam_ft_reset(ft_)); }
    void setBestNFeatures(int n) {
        options_.use_best_n_features = n;
        if (ft_) check(vslam_ft_set_best_n(ft_, n));
    }
    void setMinTracksToDetect(int n) {
        options_.min_tracks_to_detect_new_features = (std::size_t)n;
        if (ft_) check(vslam_ft_set_min_tracks(ft_, n));
    }
    void getDisparity(const double& pivot_ratio, double& total_avg_disparity, std::size_t camera_id = 0) const {
        check(vslam_ft_disparity_cam(ft_, (int)camera_id, pivot_ratio, &total_avg_disparity));
    }
    std::size_t camera_num() const { return camera_num_; }
    /* the current frame's features of one camera in addFeature order */
    std::size_t num_features(std::size_t camera_id = 0) const { return n_features_.at(camera_id); }
    const vslam_ft_feature& feature(std::size_t i, std::size_t camera_id = 0) const { return features_.at(camera_id)[i]; }
    std::vector<vslam_ft_track_info> tracks(std::size_t camera_id = 0) const {
        std::vector<vslam_ft_track_info> t(ft_ ? (std::size_t)vslam_ft_capacity(ft_) : 0);
        int n = 0;
        check(vslam_ft_tracks_cam(ft_, (int)camera_id, t.data(), (int)t.size(), &n));
        t.resize((std::size_t)n);
        return t;
    }

private:
    FeatureTrackerOptions options_;
    std::size_t camera_num_;
    std::vector<std::shared_ptr<detail::GridDetectorBase>> bound_; /* per camera; all the same object */
    vslam_ft* ft_ = nullptr;
    std::vector<std::vector<vslam_ft_feature>> features_;
    std::vector<std::size_t> n_features_;
};

/* ---------------------------------------------------------------------------------------------------
 * KeyFrameDatabase (src/datastructures/keyframedatabase.cpp) with the reference's method names over ids: a keyframe
 * is KeyFrame::mnId, a map Map::GetId(), a BowVector two parallel vectors (ascending word ids, values) as
 * vslam_bow_assemble produces them.  The class keeps what the reference keeps in the KeyFrame objects between
 * queries (mRelocScore, mPlaceRecognitionScore; 0 until first scored).  Neighbours = GetBestCovisibilityKeyFrames(10)
 * of a keyframe.  PRECONDITION of DetectNBestCandidates: bad keyframes have been erased (SetBadFlag does).
 * ------------------------------------------------------------------------------------------------- */
struct BowVector {
    std::vector<int32_t> ids;
    std::vector<double> values;
};
class KeyFrameDatabase {
public:
    typedef std::function<std::vector<long long>(long long)> Neighbours;

    explicit KeyFrameDatabase(int n_words, int scoring = 0, int device = 0) { check(vslam_kfdb_create(device, n_words, scoring, &db_)); }
    ~KeyFrameDatabase() { vslam_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(long long kf_id, int map_id, const BowVector& v) {
        check(vslam_kfdb_add(db_, kf_id, map_id, v.ids.data(), v.values.data(), (int)v.ids.size()));
        maps_[kf_id] = map_id;
    }
    void erase(long long kf_id) {
        check(vslam_kfdb_erase(db_, kf_id));
        forget(kf_id);
    }
    void clear() {
        check(vslam_kfdb_clear(db_));
        maps_.clear();
        reloc_.clear();
        place_.clear();
    }
    void clearMap(int map_id) {
        check(vslam_kfdb_clear_map(db_, map_id));
        std::vector<long long> gone;
        for (const auto& kv : maps_)
            if (kv.second == map_id) gone.push_back(kv.first);
        for (long long k : gone) forget(k);
    }
    int size() const {
        int n = 0;
        check(vslam_kfdb_size(db_, &n, nullptr));
        return n;
    }

    /* tracking.cpp:3464 */
    std::vector<long long> DetectRelocalizationCandidates(const FExtractor& extractor, const BowVector& F_mBowVec, int map_id,
                                                          const Neighbours& neighbours) {
        Hits h = query(extractor, F_mBowVec, reloc_);
        std::vector<int64_t> out(h.kf.size() + 1);
        int n = 0;
        check_select(vslam_kfdb_select_relocalization(h.kf.data(), h.map.data(), h.words.data(), h.si.data(), (int)h.kf.size(),
                                                      h.io.data(), map_id, &KeyFrameDatabase::neighbours_cb, (void*)&neighbours,
                                                      out.data(), (int)out.size(), &n));
        keep(h, reloc_);
        return std::vector<long long>(out.begin(), out.begin() + n);
    }
    /* loopclosing.cpp:415 */
    void DetectNBestCandidates(const FExtractor& extractor, const BowVector& pKF_mBowVec, int map_id,
                               const std::vector<long long>& connected, std::vector<long long>& vpLoopCand,
                               std::vector<long long>& vpMergeCand, int nNumCandidates, const Neighbours& neighbours,
                               const std::vector<int32_t>& bad_maps = std::vector<int32_t>()) {
        Hits h = query(extractor, pKF_mBowVec, place_);
        const std::vector<int64_t> conn(connected.begin(), connected.end());
        std::vector<int64_t> lo((size_t)nNumCandidates + 1), me((size_t)nNumCandidates + 1);
        int nl = 0, nm = 0;
        check_select(vslam_kfdb_select_nbest(h.kf.data(), h.map.data(), h.words.data(), h.si.data(), (int)h.kf.size(), h.io.data(),
                                             map_id, conn.data(), (int)conn.size(), nNumCandidates, bad_maps.data(),
                                             (int)bad_maps.size(), &KeyFrameDatabase::neighbours_cb, (void*)&neighbours, lo.data(),
                                             &nl, me.data(), &nm));
        keep(h, place_);
        vpLoopCand.assign(lo.begin(), lo.begin() + nl);
        vpMergeCand.assign(me.begin(), me.begin() + nm);
    }

private:
    struct Hits {
        std::vector<int64_t> kf;
        std::vector<int32_t> map, words;
        std::vector<float> si, io;
    };
    static vslam_fe* context_of(const FExtractor& extractor) {
        if (!extractor.context()) throw std::runtime_error("KeyFrameDatabase: the extractor has not processed an image yet");
        return extractor.context();
    }
    static void check_select(int rc) {
        if (rc != 0) throw std::runtime_error("libvslam_fe: KeyFrameDatabase selection failed");
    }
    static int neighbours_cb(void* user, int64_t kf_id, int64_t* out) {
        const std::vector<long long> v = (*(const Neighbours*)user)(kf_id);
        const int n = v.size() < 10 ? (int)v.size() : 10;
        for (int i = 0; i < n; i++) out[i] = v[i];
        return n;
    }
    Hits query(const FExtractor& extractor, const BowVector& v, const std::map<long long, float>& stale) {
        const int32_t* ids = v.ids.data();
        const double* vals = v.values.data();
        const int n = (int)v.ids.size();
        check(vslam_kfdb_query_async(db_, context_of(extractor), 1, &ids, &vals, &n));
        Hits h;
        const size_t cap = maps_.size() + 1;
        h.kf.resize(cap);
        h.map.resize(cap);
        h.words.resize(cap);
        h.si.resize(cap);
        int nh = 0;
        check(vslam_kfdb_query_wait(db_, context_of(extractor), 0, (int)cap, h.kf.data(), h.map.data(), h.words.data(), h.si.data(),
                                    nullptr, &nh));
        h.kf.resize(nh);
        h.map.resize(nh);
        h.words.resize(nh);
        h.si.resize(nh);
        for (int i = 0; i < nh; i++) {
            auto it = stale.find(h.kf[i]);
            h.io.push_back(it == stale.end() ? 0.0f : it->second);
        }
        h.io.resize((size_t)nh + 1); /* never an empty array */
        return h;
    }
    static void keep(const Hits& h, std::map<long long, float>& stale) {
        for (size_t i = 0; i < h.kf.size(); i++) stale[h.kf[i]] = h.io[i];
    }
    void forget(long long k) {
        maps_.erase(k);
        reloc_.erase(k);
        place_.erase(k);
    }
    vslam_kfdb* db_ = nullptr;
    std::map<long long, int> maps_;
    std::map<long long, float> reloc_, place_;
};

/* ---------------------------------------------------------------------------------------------------
 * The observation graph and the covisibility counts over it (include/vslam_fe.h, Covisibility): MapPoint::mObservations,
 * nObs and mbBad, the keyframes' map and mbBad, behind ids.  The caller calls the twin wherever the reference calls the
 * original: AddObservation / EraseObservation / SetBadFlag / Replace of a MapPoint, SetBadFlag / UpdateMap of a KeyFrame.
 * order_key stands for the KeyFrame* value, by which the reference orders its maps and sorts: pass (uintptr_t)pKF.
 * UpdateConnections answers KeyFrame::UpdateConnections (keyframe.cpp:363-427), the vote of
 * Tracking::UpdateLocalKeyFrames (tracking.cpp:3309-3376) and TrackedMapPoints for up to 128 keyframes / frames in one
 * enqueue; KeyFrameCulling walks LocalMapping::KeyFrameCulling's loop (localmapping.cpp:983-1100) by the walk rule.
 * ------------------------------------------------------------------------------------------------- */
class CovisibilityMap {
public:
    enum Mode { CONNECTIONS = VSLAM_COVIS_CONNECTIONS, VOTE = VSLAM_COVIS_VOTE };
    struct ConnectionsJob {
        int mode;
        long long self_kf; /* mnId; unused by VOTE */
        int map_id;
        int min_obs;                   /* TrackedMapPoints(minObs) */
        std::vector<long long> mp_ids; /* mvpMapPoints, -1 = NULL */
    };
    struct Connections {
        int error;
        std::vector<long long> counter_kf; /* mConnectedKeyFrameWeights in ascending order_key */
        std::vector<int> counter_n;
        long long kf_max;
        int n_max;
        std::vector<long long> ordered_kf; /* mvpOrderedConnectedKeyFrames */
        std::vector<int> ordered_w;        /* mvOrderedWeights */
        int n_tracked;
    };
    struct CullingJob {
        long long kf_id;
        std::vector<long long> mp_ids; /* -1 = NULL or rejected by the depth gate (localmapping.cpp:1003-1007) */
        std::vector<int32_t> levels;   /* scaleLevel of :1012-1014 */
    };
    struct CullingResult {
        int error, nMPs, nRedundantObservations;
    };

    explicit CovisibilityMap(int device = 0, int initial_entries = 0) { check(vslam_covis_create(device, initial_entries, &c_)); }
    ~CovisibilityMap() { vslam_covis_destroy(c_); }
    CovisibilityMap(const CovisibilityMap&) = delete;
    CovisibilityMap& operator=(const CovisibilityMap&) = delete;

    void AddKeyFrame(long long kf_id, int map_id, unsigned long long order_key) { check(vslam_covis_add_keyframe(c_, kf_id, map_id, order_key)); }
    void SetKeyFrameBad(long long kf_id) { check(vslam_covis_set_keyframe_bad(c_, kf_id)); }
    void UpdateMap(long long kf_id, int map_id) { check(vslam_covis_set_keyframe_map(c_, kf_id, map_id)); }
    void EraseKeyFrame(long long kf_id) {
        check(vslam_covis_erase_keyframe(c_, kf_id));
        ordered_.erase(kf_id);
    }
    void AddMapPoint(long long mp_id) { check(vslam_covis_add_point(c_, mp_id)); }
    /* MapPoint::AddObservation: stereo = !pKF->mpCamera2 && pKF->mvuRight[idx] >= 0, is_right = pKF->NLeft != -1 && idx >= NLeft */
    void AddObservation(long long mp_id, long long kf_id, int idx, bool is_right, int octave, bool stereo) {
        check(vslam_covis_add_observation(c_, mp_id, kf_id, idx, is_right, octave, stereo));
    }
    /* MapPoint::EraseObservation -> whether the point became bad (SetBadFlag ran) */
    bool EraseObservation(long long mp_id, long long kf_id) {
        int bad = 0;
        check(vslam_covis_erase_observation(c_, mp_id, kf_id, &bad));
        return bad != 0;
    }
    /* the first block of MapPoint::SetBadFlag and of MapPoint::Replace */
    void ClearMapPoint(long long mp_id) { check(vslam_covis_clear_point(c_, mp_id)); }
    void EraseMapPoint(long long mp_id) { check(vslam_covis_erase_point(c_, mp_id)); }
    void clearMap(int map_id) {
        check(vslam_covis_clear_map(c_, map_id));
        ordered_.clear();
    }
    void clear() {
        check(vslam_covis_clear(c_));
        ordered_.clear();
    }
    /* KeyFrame::SetBadFlag as far as the graph goes (keyframe.cpp:553, :629) */
    void SetBadFlag(long long kf_id, const std::vector<long long>& mvpMapPoints) {
        for (long long m : mvpMapPoints)
            if (m != -1) EraseObservation(m, kf_id);
        SetKeyFrameBad(kf_id);
    }

    std::vector<Connections> UpdateConnections(const FExtractor& extractor, const std::vector<ConnectionsJob>& jobs) {
        std::vector<std::vector<int64_t> > ids(jobs.size());
        std::vector<vslam_covis_job> J(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) {
            ids[j].assign(jobs[j].mp_ids.begin(), jobs[j].mp_ids.end());
            J[j] = vslam_covis_job{jobs[j].mode, jobs[j].map_id, jobs[j].self_kf, jobs[j].min_obs, (int32_t)ids[j].size(), ids[j].data()};
        }
        std::vector<vslam_covis_result> R(jobs.size() + 1);
        check(vslam_covis_connections(c_, context_of(extractor), (int)jobs.size(), J.data(), R.data()));
        std::vector<Connections> out(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) {
            const vslam_covis_result& r = R[j];
            std::vector<int64_t> ck((size_t)r.n_counter + 1), ok((size_t)r.n_ordered + 1);
            std::vector<int32_t> cn((size_t)r.n_counter + 1), ow((size_t)r.n_ordered + 1);
            check(vslam_covis_connections_lists(c_, (int)j, ck.data(), cn.data(), ok.data(), ow.data()));
            Connections& o = out[j];
            o.error = r.error;
            o.counter_kf.assign(ck.begin(), ck.begin() + r.n_counter);
            o.counter_n.assign(cn.begin(), cn.begin() + r.n_counter);
            o.kf_max = r.kf_max;
            o.n_max = r.n_max;
            o.ordered_kf.assign(ok.begin(), ok.begin() + r.n_ordered);
            o.ordered_w.assign(ow.begin(), ow.begin() + r.n_ordered);
            o.n_tracked = r.n_tracked;
            /* what GetBestCovisibilityKeyFrames reads; an empty counter leaves the lists as they were (keyframe.cpp:385) */
            if (jobs[j].mode == CONNECTIONS && !r.error && r.n_counter) ordered_[jobs[j].self_kf] = o.ordered_kf;
        }
        return out;
    }

    std::vector<CullingResult> Culling(const FExtractor& extractor, const std::vector<CullingJob>& jobs, size_t first = 0, int thObs = 3) {
        std::vector<std::vector<int64_t> > ids(jobs.size());
        std::vector<vslam_covis_cull_job> J;
        for (size_t j = first; j < jobs.size(); j++) {
            if (jobs[j].levels.size() != jobs[j].mp_ids.size()) throw std::invalid_argument("CovisibilityMap::Culling: one level per MapPoint");
            ids[j].assign(jobs[j].mp_ids.begin(), jobs[j].mp_ids.end());
            J.push_back(vslam_covis_cull_job{jobs[j].kf_id, (int32_t)ids[j].size(), 0, ids[j].data(), jobs[j].levels.data()});
        }
        std::vector<vslam_covis_cull_result> R(J.size() + 1);
        check(vslam_covis_culling(c_, context_of(extractor), (int)J.size(), J.data(), thObs, R.data()));
        std::vector<CullingResult> out(J.size());
        for (size_t j = 0; j < J.size(); j++) out[j] = CullingResult{R[j].error, R[j].n_mps, R[j].n_redundant};
        return out;
    }

    /* The walk rule.  SetBadFlag on a culled keyframe erases its observations and changes the counts of the keyframes
     * behind it, so the results of one enqueue hold up to and including the first job whose keyframe is culled: the walk
     * takes the jobs in order, asks shouldCull(job, result) -- `nRedundantObservations > redundant_th * nMPs` and the
     * inertial conditions of localmapping.cpp:1054-1096 -- lets applyCull(job) call the mutators (SetBadFlag above), and
     * enqueues the jobs behind it again.  Returns every job's result as the sequential loop sees it. */
    template <class ShouldCull, class ApplyCull>
    std::vector<CullingResult> KeyFrameCulling(const FExtractor& extractor, const std::vector<CullingJob>& jobs, ShouldCull shouldCull,
                                               ApplyCull applyCull, int thObs = 3) {
        std::vector<CullingResult> out;
        size_t at = 0;
        while (at < jobs.size()) {
            const std::vector<CullingResult> res = Culling(extractor, jobs, at, thObs);
            for (size_t i = 0; i < res.size(); i++) {
                out.push_back(res[i]);
                const CullingJob& job = jobs[at++];
                if (!res[i].error && shouldCull(job, res[i])) {
                    applyCull(job);
                    break;
                }
            }
        }
        return out;
    }

    /* GetBestCovisibilityKeyFrames(10) from the ordered list of the last CONNECTIONS result of the keyframe: as a
     * vslam_kfdb_neighbours_fn (user = the CovisibilityMap) and as KeyFrameDatabase::Neighbours */
    static int neighbours(void* user, int64_t kf_id, int64_t* out_ids) {
        const CovisibilityMap* self = (const CovisibilityMap*)user;
        const auto it = self->ordered_.find(kf_id);
        if (it == self->ordered_.end()) return 0;
        const int n = it->second.size() < 10 ? (int)it->second.size() : 10;
        for (int i = 0; i < n; i++) out_ids[i] = it->second[(size_t)i];
        return n;
    }
    KeyFrameDatabase::Neighbours neighbours() const {
        return [this](long long kf_id) {
            int64_t ids[10];
            const int n = neighbours((void*)this, kf_id, ids);
            return std::vector<long long>(ids, ids + n);
        };
    }

    void size(int& keyframes, int& points, long long& observations) const { check(vslam_covis_size(c_, &keyframes, &points, &observations)); }
    vslam_covis* handle() const { return c_; }

private:
    static vslam_fe* context_of(const FExtractor& extractor) {
        if (!extractor.context()) throw std::runtime_error("CovisibilityMap: the extractor has not processed an image yet");
        return extractor.context();
    }
    vslam_covis* c_ = nullptr;
    std::map<long long, std::vector<long long> > ordered_;
};

} /* namespace geometry */

/* ---------------------------------------------------------------------------------------------------
 * DBoW3::Vocabulary (thirdparty/DBoW3/DBoW3/src/Vocabulary.h), the part tools/createVoc/createVoc.cpp:53-57 and the
 * apps use: construct with (k, L, weighting, scoring), create(training_features), save(filename), load(filename).
 * There is no cv::Mat here: the descriptors of one image are a row-major block of rows x 32 bytes (what the reference's
 * `cv::Mat descriptors` of an ORB detector holds).  create() trains on the device (vslam_voc_train) and leaves the
 * vocabulary uploaded; device() is what vslam_bow_transform takes.  The draws come from setSeed()'s value, not from
 * rand(): the same seed gives the same vocabulary.
 * ------------------------------------------------------------------------------------------------- */
namespace DBoW3 {
enum WeightingType { TF_IDF, TF, IDF, BINARY };
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };
struct Descriptors { /* non-owning: rows x 32 bytes */
    const uint8_t* data;
    int rows;
};
class Vocabulary {
public:
    explicit Vocabulary(int k = 10, int L = 5, WeightingType weighting = TF_IDF, ScoringType scoring = L1_NORM, int device = 0)
        : k_(k), L_(L), weighting_(weighting), scoring_(scoring), device_(device) {}
    explicit Vocabulary(const std::string& filename, int device = 0) : device_(device) { load(filename); }
    ~Vocabulary() { clear(); }
    Vocabulary(const Vocabulary&) = delete;
    Vocabulary& operator=(const Vocabulary&) = delete;

    void setSeed(uint64_t seed) { seed_ = seed; }
    void create(const std::vector<Descriptors>& training_features) {
        std::vector<uint8_t> all;
        std::vector<int64_t> offsets(1, 0);
        for (const Descriptors& d : training_features) {
            if (d.rows > 0) all.insert(all.end(), d.data, d.data + (size_t)d.rows * 32);
            offsets.push_back(offsets.back() + (d.rows > 0 ? d.rows : 0));
        }
        vslam_voc_train_params p;
        std::memset(&p, 0, sizeof(p));
        p.k = k_, p.L = L_, p.weighting = (int)weighting_, p.scoring = (int)scoring_, p.seed = seed_, p.rand_mask = 0x7fffffffu;
        vslam_voc_file* f = nullptr;
        geometry::check(vslam_voc_train(device_, &p, all.empty() ? (const uint8_t*)"" : all.data(), VSLAM_IMGS_HOST, offsets.data(),
                                        (int)training_features.size(), &f, &stats_));
        adopt(f);
    }
    void create(const std::vector<Descriptors>& training_features, int k, int L) {
        k_ = k, L_ = L;
        create(training_features);
    }
    void create(const std::vector<Descriptors>& training_features, int k, int L, WeightingType weighting, ScoringType scoring) {
        k_ = k, L_ = L, weighting_ = weighting, scoring_ = scoring;
        create(training_features);
    }
    /* Vocabulary::save for a name without ".yml": the plain binary stream */
    void save(const std::string& filename) const {
        if (!file_) throw std::runtime_error("DBoW3::Vocabulary::save: empty vocabulary");
        check_file(vslam_voc_file_save(file_, filename.c_str()));
    }
    void load(const std::string& filename) {
        vslam_voc_file* f = nullptr;
        check_file(vslam_voc_file_open(filename.c_str(), &f));
        adopt(f);
        int k = 0, L = 0, s = 0, w = 0;
        vslam_voc_file_info(file_, &k, &L, &s, &w, nullptr, nullptr, nullptr, nullptr, nullptr);
        k_ = k, L_ = L, scoring_ = (ScoringType)s, weighting_ = (WeightingType)w;
    }
    void clear() {
        vslam_voc_destroy(voc_);
        vslam_voc_file_close(file_);
        voc_ = nullptr;
        file_ = nullptr;
    }
    /* Frame::ComputeBoW of a two-camera rig (frame.cpp:455-461 over the vconcat'ed descriptors, :1137): transform(features,
     * mBowVec, mFeatVec, levelsup) with the per-feature descent of both extractors' slot 0 on the device and ONE assembly
     * over the Nleft + Nright features, left first.  F: both extractors are read. */
    void transform(const geometry::FMatcher::RigFrameView& F, geometry::BowVector& bow, geometry::FeatureVector& fv,
                   int levelsup) const {
        if (!voc_ || !F.left.frame.extractor || !F.right)
            throw std::invalid_argument("DBoW3::Vocabulary::transform: an empty vocabulary or a rig frame without its extractors");
        int weighting = 0, norm = 0;
        geometry::check(vslam_voc_info(voc_, nullptr, &weighting, &norm, nullptr));
        const geometry::FExtractor* ex[2] = {F.left.frame.extractor, F.right};
        int n[2] = {0, 0};
        const uint8_t* dd[2] = {nullptr, nullptr};
        for (int s = 0; s < 2; s++) {
            const vslam_kp* dk = nullptr;
            geometry::check(vslam_fe_slot_buffers(ex[s]->context(), 0, &dk, &dd[s], &n[s]));
        }
        const size_t N = (size_t)n[0] + (size_t)n[1];
        std::vector<int32_t> word(N + 1), nid(N + 1);
        std::vector<double> weight(N + 1);
        for (int s = 0, o = 0; s < 2; o += n[s], s++)
            geometry::check(vslam_bow_transform(ex[s]->context(), voc_, dd[s], n[s], levelsup, word.data() + o, weight.data() + o,
                                                nid.data() + o));
        bow.ids.assign(N + 1, 0);
        bow.values.assign(N + 1, 0.0);
        fv.nodes.assign(N + 1, 0);
        fv.off.assign(N + 2, 0);
        fv.feat.assign(N + 1, 0);
        int nb = 0, nf = 0;
        if (vslam_bow_assemble(weighting, norm, word.data(), weight.data(), nid.data(), (int)N, bow.ids.data(), bow.values.data(),
                               &nb, fv.nodes.data(), fv.off.data(), fv.feat.data(), &nf) != VSLAM_OK)
            throw std::invalid_argument("DBoW3::Vocabulary::transform: vslam_bow_assemble refused its arguments");
        bow.ids.resize((size_t)nb);
        bow.values.resize((size_t)nb);
        fv.nodes.resize((size_t)nf);
        fv.off.resize((size_t)nf + 1);
        fv.feat.resize((size_t)fv.off[(size_t)nf]);
    }
    bool empty() const { return !file_; }
    unsigned size() const { /* number of words */
        int n = 0;
        if (file_) vslam_voc_file_info(file_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, nullptr, nullptr);
        return (unsigned)n;
    }
    int getBranchingFactor() const { return k_; }
    int getDepthLevels() const { return L_; }
    const vslam_voc* device() const { return voc_; }
    const vslam_voc_file* file() const { return file_; }
    const vslam_voc_train_stats& stats() const { return stats_; }

private:
    static void check_file(int rc) {
        if (rc != VSLAM_OK) throw std::runtime_error(std::string("libvslam_fe: ") + vslam_voc_file_last_error());
    }
    void adopt(vslam_voc_file* f) {
        vslam_voc* v = nullptr;
        const int rc = vslam_voc_file_upload(device_, f, &v);
        if (rc != VSLAM_OK) {
            vslam_voc_file_close(f);
            geometry::check(rc);
        }
        clear();
        file_ = f;
        voc_ = v;
    }
    int k_ = 10, L_ = 5;
    WeightingType weighting_ = TF_IDF;
    ScoringType scoring_ = L1_NORM;
    int device_ = 0;
    uint64_t seed_ = 0;
    vslam_voc_file* file_ = nullptr;
    vslam_voc* voc_ = nullptr;
    vslam_voc_train_stats stats_ = vslam_voc_train_stats();
};
} /* namespace DBoW3 */
} /* namespace VSLAM_SHIM_NAMESPACE */
#endif /* VSLAM_SHIM_HPP */
