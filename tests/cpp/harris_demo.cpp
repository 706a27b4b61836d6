/* vilib::HarrisGPU through include/vslam_shim.hpp, set up as the reference's own detector test does
 * (test/harris-cuda/src/test_harris.cpp:143-154: one level, 32x32 cells, no extra border, BORDER_SKIP, Harris with
 * k = 0.04, quality level 0.1), then once more as Shi-Tomasi on three levels.
 * Output: per kept point one line "P|S cell x y score level" (score as the float's hexadecimal word), then one line of
 * JSON with the counts for the pytest driver.
 *   harris_demo W H image.raw
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_shim.hpp"

using namespace vi_slam_amd::geometry;

#define PYRAMID_MIN_LEVEL 0
#define PYRAMID_MAX_LEVEL 1
#define USE_HARRIS true
#define HARRIS_K 0.04f
#define QUALITY_LEVEL 0.1f
#define CONV_FILTER_BORDER_TYPE VSLAM_HG_BORDER_SKIP
#define HORIZONTAL_BORDER 0
#define VERTICAL_BORDER 0
#define CELL_SIZE_WIDTH 32
#define CELL_SIZE_HEIGHT 32

static std::size_t print_points(const char* tag, const HarrisGPU& det) {
    const std::vector<HarrisGPU::FeaturePoint>& pts = det.getPoints();
    std::size_t n = 0;
    for (std::size_t i = 0; i < pts.size(); i++) {
        if (!det.isOccupied(i)) continue;
        const float s = (float)pts[i].score_;
        uint32_t word;
        std::memcpy(&word, &s, 4);
        std::printf("%s %zu %.1f %.1f %08x %u\n", tag, i, pts[i].x_, pts[i].y_, word, pts[i].level_);
        n++;
    }
    return n;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    std::vector<uint8_t> img((size_t)w * h);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[3]);
        return 2;
    }
    std::fclose(f);
    try {
        HarrisGPU harris((std::size_t)w, (std::size_t)h, CELL_SIZE_WIDTH, CELL_SIZE_HEIGHT, PYRAMID_MIN_LEVEL, PYRAMID_MAX_LEVEL,
                         HORIZONTAL_BORDER, VERTICAL_BORDER, CONV_FILTER_BORDER_TYPE, USE_HARRIS, HARRIS_K, QUALITY_LEVEL);
        harris.reset();
        harris.detect(img.data(), (std::size_t)w);
        const std::size_t n1 = print_points("P", harris);
        HarrisGPU shi((std::size_t)w, (std::size_t)h, CELL_SIZE_WIDTH, CELL_SIZE_HEIGHT, 0, 3, HORIZONTAL_BORDER, VERTICAL_BORDER,
                      VSLAM_HG_BORDER_REFLECT_101, false, HARRIS_K, QUALITY_LEVEL);
        shi.detect(img.data(), (std::size_t)w);
        const std::size_t n2 = print_points("S", shi);
        std::printf("{\"cols\": %zu, \"rows\": %zu, \"harris_n\": %zu, \"harris_count\": %zu, \"shi_n\": %zu}\n",
                    harris.getCellCountHorizontal(), harris.getCellCountVertical(), n1, harris.count(), n2);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "harris_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
