// dump_opencv_cvtcolor.cpp -- for a maintainer who HAS OpenCV (the reference's dependency; not in this project's image):
// settles the two OpenCV functions that the colour-input and RGB-D paths restate from memory, not from a pinned build
// (k_gray_images / k_rgbd_depth in vi_slam_amd/csrc/vslam_match_kernels.hip, tests/rgbd_ref.py):
//   cv::cvtColor(im, im, COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) on CV_8U   (tracking.cpp:1235-1258, 1290-1303, 1324-1336)
//   imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) from CV_16U / CV_32F   (tracking.cpp:1305-1306)
//
//   1. g++ -O2 -std=c++14 tools/dump_opencv_cvtcolor.cpp -o dump_opencv_cvtcolor `pkg-config --cflags --libs opencv4`
//   2. mkdir -p tests/golden/opencv_cvtcolor && ./dump_opencv_cvtcolor tests/golden/opencv/in_hut_320x240.gray tests/golden/opencv_cvtcolor
//   3. python -m pytest tests/test_opencv_cvtcolor.py   (says which gray_shift this OpenCV uses; the OpenCV comparison is
//                                                        skipped without out_cvtcolor_*)
//
// Inputs: the committed 320 x 240 gray image, its channels made from it by integer arithmetic (so that the colour image is
// the same everywhere), followed by 100000 pixels of a 32-bit LCG; every file carries its inputs next to OpenCV's outputs.
// Output format as tools/dump_opencv_primitives.cpp (little endian): magic "VSLD", u32 kind, u32 n_dims, u32 dims[n_dims],
// payload:
//   out_cvtcolor_<rgb|bgr|rgba|bgra>.bin  kind 10, uint8[n][bpp + 1]   the pixel's bytes in memory order, then the gray value
//   out_convert_u16.bin                   kind 11, float32[65536][3]   sample (every CV_16U value), factor, converted sample
//   out_convert_f32.bin                   kind 11, float32[n][3]       the same for CV_32F samples and three factors
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <opencv2/core.hpp>
#include <opencv2/imgproc.hpp>

static void write_blob(const std::string& path, uint32_t kind, const std::vector<uint32_t>& dims, const void* data,
                       size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(1);
    }
    fwrite("VSLD", 1, 4, f);
    const uint32_t nd = (uint32_t)dims.size();
    fwrite(&kind, 4, 1, f);
    fwrite(&nd, 4, 1, f);
    fwrite(dims.data(), 4, nd, f);
    fwrite(data, 1, bytes, f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <tests/golden/opencv/in_hut_320x240.gray> <tests/golden/opencv_cvtcolor>\n", argv[0]);
        return 2;
    }
    const int W = 320, H = 240, NRAND = 100000;
    std::vector<uint8_t> gray((size_t)W * H);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(gray.data(), 1, gray.size(), f) != gray.size()) {
        fprintf(stderr, "cannot read %s (320 x 240 bytes)\n", argv[1]);
        return 1;
    }
    fclose(f);
    const std::string dir = argv[2];
    // R, G, B, A of every pixel: the image, then the LCG
    const int n = W * H + NRAND;
    std::vector<uint8_t> rgba((size_t)n * 4);
    uint32_t lcg = 12345u;
    for (int i = 0; i < n; i++) {
        uint8_t* p = &rgba[(size_t)i * 4];
        if (i < W * H) {
            const int x = i % W, y = i / W;
            p[0] = gray[i];
            p[1] = (uint8_t)((gray[(size_t)y * W + (x + W - 1) % W] * 205) >> 8);
            p[2] = (uint8_t)std::min(255, ((gray[(size_t)((y + H - 1) % H) * W + x] * 294) >> 8) + 20);
            p[3] = (uint8_t)(i * 7);
        } else
            for (int k = 0; k < 4; k++) {
                lcg = lcg * 1664525u + 1013904223u;
                p[k] = (uint8_t)(lcg >> 24);
            }
    }
    struct Fmt { const char* name; int code, bpp, order[4]; } fmts[] = {
        {"rgb", cv::COLOR_RGB2GRAY, 3, {0, 1, 2, 3}}, {"bgr", cv::COLOR_BGR2GRAY, 3, {2, 1, 0, 3}},
        {"rgba", cv::COLOR_RGBA2GRAY, 4, {0, 1, 2, 3}}, {"bgra", cv::COLOR_BGRA2GRAY, 4, {2, 1, 0, 3}}};
    for (const Fmt& F : fmts) {
        cv::Mat im(1, n, CV_8UC(F.bpp));
        for (int i = 0; i < n; i++)
            for (int k = 0; k < F.bpp; k++) im.data[(size_t)i * F.bpp + k] = rgba[(size_t)i * 4 + F.order[k]];
        cv::Mat g;
        cv::cvtColor(im, g, F.code);
        std::vector<uint8_t> out((size_t)n * (F.bpp + 1));
        for (int i = 0; i < n; i++) {
            memcpy(&out[(size_t)i * (F.bpp + 1)], im.data + (size_t)i * F.bpp, F.bpp);
            out[(size_t)i * (F.bpp + 1) + F.bpp] = g.data[i];
        }
        write_blob(dir + "/out_cvtcolor_" + F.name + ".bin", 10, {(uint32_t)n, (uint32_t)F.bpp + 1}, out.data(), out.size());
    }
    {   // every CV_16U value with the TUM factor
        const float factor = 1.0f / 5000.0f;
        cv::Mat d(1, 65536, CV_16U), o;
        for (int i = 0; i < 65536; i++) d.at<uint16_t>(0, i) = (uint16_t)i;
        d.convertTo(o, CV_32F, factor);
        std::vector<float> rows;
        for (int i = 0; i < 65536; i++) {
            rows.push_back((float)i);
            rows.push_back(factor);
            rows.push_back(o.at<float>(0, i));
        }
        write_blob(dir + "/out_convert_u16.bin", 11, {65536u, 3u}, rows.data(), rows.size() * 4);
    }
    {   // CV_32F samples between 0 and 16 m (a few negative) with three factors
        const int m = 20000;
        const float factors[3] = {0.5f, 1.0f / 5000.0f, 1.00002f};
        std::vector<float> rows;
        for (float factor : factors) {
            cv::Mat d(1, m, CV_32F), o;
            for (int i = 0; i < m; i++) {
                lcg = lcg * 1664525u + 1013904223u;
                d.at<float>(0, i) = (float)(lcg >> 8) * (17.0f / 16777216.0f) - 1.0f;
            }
            d.convertTo(o, CV_32F, factor);
            for (int i = 0; i < m; i++) {
                rows.push_back(d.at<float>(0, i));
                rows.push_back(factor);
                rows.push_back(o.at<float>(0, i));
            }
        }
        write_blob(dir + "/out_convert_f32.bin", 11, {(uint32_t)(3 * m), 3u}, rows.data(), rows.size() * 4);
    }
    printf("wrote %s/out_cvtcolor_*.bin, out_convert_*.bin (OpenCV %s)\n", dir.c_str(), CV_VERSION);
    return 0;
}
