/* vilib::FeatureTrackerGPU over a FrameBundle of two cameras through include/vslam_shim.hpp: the set-up of lk_demo.cpp
 * (the reference's own tracker test, test/src/high_level/test_featuretracker.cpp:53-75,97-102) with camera_num = 2, both
 * cameras bound to one Harris detector whose max_batch is 2, new features below 45 tracks.
 * Output: per call, camera and feature one line "F call camera x y score level track_id" (floats as their hexadecimal
 * words), then one line of JSON with the per-call totals and each camera's track count and getDisparity(0.5).
 *   lk_bundle_demo W H N camera0.raw camera1.raw        (N frames of W x H bytes per file)
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vslam_shim.hpp"

using namespace vi_slam_amd::geometry;

#define CAMERA_NUM 2
#define FRAME_IMAGE_PYRAMID_LEVELS 5
#define FEATURE_DETECTOR_CELL_SIZE_WIDTH 32
#define FEATURE_DETECTOR_CELL_SIZE_HEIGHT 32
#define FEATURE_DETECTOR_MIN_LEVEL 0
#define FEATURE_DETECTOR_MAX_LEVEL 2
#define FEATURE_DETECTOR_HORIZONTAL_BORDER 8
#define FEATURE_DETECTOR_VERTICAL_BORDER 8
#define FEATURE_DETECTOR_HARRIS_K 0.04f
#define FEATURE_DETECTOR_HARRIS_QUALITY_LEVEL 0.1f
#define FEATURE_DETECTOR_HARRIS_BORDER_TYPE VSLAM_HG_BORDER_SKIP

static unsigned word(float v) {
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return w;
}

int main(int argc, char** argv) {
    if (argc != 4 + CAMERA_NUM) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[3]);
    std::vector<std::vector<uint8_t>> frames(CAMERA_NUM, std::vector<uint8_t>((size_t)w * h * n));
    for (int c = 0; c < CAMERA_NUM; c++) {
        FILE* f = std::fopen(argv[4 + c], "rb");
        if (!f || std::fread(frames[c].data(), 1, frames[c].size(), f) != frames[c].size()) {
            std::fprintf(stderr, "cannot read %s\n", argv[4 + c]);
            return 2;
        }
        std::fclose(f);
    }
    try {
        FeatureTrackerOptions feature_tracker_options;
        feature_tracker_options.reset_before_detection = false;
        feature_tracker_options.use_best_n_features = 50;
        feature_tracker_options.min_tracks_to_detect_new_features = 45;
        feature_tracker_options.pyramid_levels = FRAME_IMAGE_PYRAMID_LEVELS;
        std::shared_ptr<detail::GridDetectorBase> detector_gpu_(new HarrisGPU(
            (std::size_t)w, (std::size_t)h, FEATURE_DETECTOR_CELL_SIZE_WIDTH, FEATURE_DETECTOR_CELL_SIZE_HEIGHT, FEATURE_DETECTOR_MIN_LEVEL,
            FEATURE_DETECTOR_MAX_LEVEL, FEATURE_DETECTOR_HORIZONTAL_BORDER, FEATURE_DETECTOR_VERTICAL_BORDER,
            FEATURE_DETECTOR_HARRIS_BORDER_TYPE, true, FEATURE_DETECTOR_HARRIS_K, FEATURE_DETECTOR_HARRIS_QUALITY_LEVEL, 0, CAMERA_NUM));
        FeatureTrackerGPU tracker_gpu_(feature_tracker_options, CAMERA_NUM);
        for (std::size_t c = 0; c < CAMERA_NUM; c++) tracker_gpu_.setDetectorGPU(detector_gpu_, c);
        tracker_gpu_.reset();
        std::string counts;
        for (int k = 0; k < n; k++) {
            std::size_t total_tracked_ftr_cnt = 0, total_detected_ftr_cnt = 0;
            std::vector<const uint8_t*> bundle;
            for (int c = 0; c < CAMERA_NUM; c++) bundle.push_back(frames[c].data() + (size_t)k * w * h);
            tracker_gpu_.track(bundle, (std::size_t)w, total_tracked_ftr_cnt, total_detected_ftr_cnt);
            for (std::size_t c = 0; c < CAMERA_NUM; c++)
                for (std::size_t i = 0; i < tracker_gpu_.num_features(c); i++) {
                    const vslam_ft_feature& p = tracker_gpu_.feature(i, c);
                    std::printf("F %d %zu %08x %08x %08x %d %d\n", k, c, word(p.x), word(p.y), word(p.score), p.level, p.track_id);
                }
            counts += (k ? ", [" : "[") + std::to_string(total_tracked_ftr_cnt) + ", " + std::to_string(total_detected_ftr_cnt) + "]";
        }
        std::string tracks, disparity;
        for (std::size_t c = 0; c < CAMERA_NUM; c++) {
            double d = 0.0;
            tracker_gpu_.getDisparity(0.5, d, c);
            char hex[16];
            std::snprintf(hex, sizeof(hex), "\"%08x\"", word((float)d));
            tracks += (c ? ", " : "") + std::to_string(tracker_gpu_.tracks(c).size());
            disparity += (c ? ", " : "") + std::string(hex);
        }
        std::printf("{\"counts\": [%s], \"tracks\": [%s], \"disparity\": [%s]}\n", counts.c_str(), tracks.c_str(), disparity.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "lk_bundle_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
