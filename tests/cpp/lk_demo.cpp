/* vilib::FeatureTrackerGPU through include/vslam_shim.hpp, set up as the reference's own tracker test does
 * (test/src/high_level/test_featuretracker.cpp:53-75,97-102,110-146: five pyramid levels, a Harris detector on levels 0-1
 * with 32x32 cells and a border of 8, BORDER_SKIP, k = 0.04, quality level 0.1; reset_before_detection = false, the best
 * 50 features, new features below 0.3 * 50 tracks).
 * Output: per frame and feature one line "F frame x y score level track_id" (floats as their hexadecimal words), then
 * one line of JSON with the per-frame counts and the final getDisparity(0.5) for the pytest driver.
 *   lk_demo W H N frames.raw
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vslam_shim.hpp"

using namespace vi_slam_amd::geometry;

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
    if (argc != 5) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[3]);
    std::vector<uint8_t> frames((size_t)w * h * n);
    FILE* f = std::fopen(argv[4], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[4]);
        return 2;
    }
    std::fclose(f);
    try {
        FeatureTrackerOptions feature_tracker_options;
        feature_tracker_options.reset_before_detection = false;
        feature_tracker_options.use_best_n_features = 50;
        feature_tracker_options.min_tracks_to_detect_new_features = 0.3 * feature_tracker_options.use_best_n_features;
        feature_tracker_options.affine_est_gain = false;
        feature_tracker_options.affine_est_offset = false;
        feature_tracker_options.pyramid_levels = FRAME_IMAGE_PYRAMID_LEVELS;
        std::shared_ptr<detail::GridDetectorBase> detector_gpu_(new HarrisGPU(
            (std::size_t)w, (std::size_t)h, FEATURE_DETECTOR_CELL_SIZE_WIDTH, FEATURE_DETECTOR_CELL_SIZE_HEIGHT, FEATURE_DETECTOR_MIN_LEVEL,
            FEATURE_DETECTOR_MAX_LEVEL, FEATURE_DETECTOR_HORIZONTAL_BORDER, FEATURE_DETECTOR_VERTICAL_BORDER,
            FEATURE_DETECTOR_HARRIS_BORDER_TYPE, true, FEATURE_DETECTOR_HARRIS_K, FEATURE_DETECTOR_HARRIS_QUALITY_LEVEL));
        FeatureTrackerGPU tracker_gpu_(feature_tracker_options, 1);
        tracker_gpu_.setDetectorGPU(detector_gpu_, 0);
        tracker_gpu_.reset();
        std::string counts;
        for (int k = 0; k < n; k++) {
            std::size_t total_tracked_ftr_cnt = 0, total_detected_ftr_cnt = 0;
            tracker_gpu_.track(frames.data() + (size_t)k * w * h, (std::size_t)w, total_tracked_ftr_cnt, total_detected_ftr_cnt);
            for (std::size_t i = 0; i < tracker_gpu_.num_features(); i++) {
                const vslam_ft_feature& p = tracker_gpu_.feature(i);
                std::printf("F %d %08x %08x %08x %d %d\n", k, word(p.x), word(p.y), word(p.score), p.level, p.track_id);
            }
            counts += (k ? ", [" : "[") + std::to_string(total_tracked_ftr_cnt) + ", " + std::to_string(total_detected_ftr_cnt) + "]";
        }
        double disparity = 0.0;
        tracker_gpu_.getDisparity(0.5, disparity);
        std::printf("{\"counts\": [%s], \"tracks\": %zu, \"disparity\": \"%08x\"}\n", counts.c_str(), tracker_gpu_.tracks().size(),
                    word((float)disparity));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "lk_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
