// dump_opencv_undistort.cpp -- for a maintainer who HAS OpenCV 4.2 (the reference's dependency; not in this project's
// image): settles the restatement of cv::undistortPoints in vi_slam_amd/csrc/vslam_undistort.h / tests/undistort_ref.py,
// which is OpenCV 4.2's cvUndistortPointsInternal as recalled (five fixed iterations, the icdist < 0 exit), not pinned.
//
//   1. g++ -O2 -std=c++14 tools/dump_opencv_undistort.cpp -o dump_opencv_undistort `pkg-config --cflags --libs opencv4`
//   2. mkdir -p tests/golden/opencv_undistort && ./dump_opencv_undistort tests/golden/opencv_undistort
//   3. python -m pytest tests/test_opencv_undistort.py   (compares the restatement with what OpenCV computed; the
//                                                         OpenCV comparison is skipped without out_undistort_*)
//
// The call is the reference's own (src/datastructures/frame.cpp:770-777 UndistortKeyPoints, :797-806 ComputeImageBounds):
//   cv::Mat mat(N,2,CV_32F); mat = mat.reshape(2); cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK);
// with mK = Pinhole::toK() (CV_32F) and mDistCoef CV_32F (4 or 5 coefficients).
// Output format as tools/dump_opencv_primitives.cpp (little endian): magic "VSLD", u32 kind, u32 n_dims,
// u32 dims[n_dims], payload.  Per camera <name>:
//   out_undistort_<name>_cam.bin  kind 9, float32[10]  fx, fy, cx, cy, k1, k2, p1, p2, k3, ndist
//   out_undistort_<name>.bin      kind 8, float32[n][4] x, y (input), x, y (undistorted)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <opencv2/calib3d.hpp>
#include <opencv2/core.hpp>

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
    if (argc < 2) {
        fprintf(stderr, "usage: %s <tests/golden/opencv_undistort>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    // the coefficient sets of tests/undistort_ref.py (ZED: the reference's config/zed_camera.yaml)
    struct Cam { const char* name; float K[4]; float D[5]; int nd; } cams[] = {
        {"zed0", {669.2387507702717f, 669.6062139634853f, 647.4136147885813f, 348.40757297218505f},
         {0.0018645604002542789f, -0.009206711115906055f, -0.001490842343490958f, 0.0047045781898403f, 0.f}, 4},
        {"zed1", {669.7077049723667f, 669.7830132578491f, 648.2500643003343f, 348.45508924255745f},
         {-0.0011120079644645446f, -0.006192062533471337f, -0.0011416874899672696f, 0.004836945809987094f, 0.f}, 4},
        {"euroc", {700.0f, 699.5f, 641.3f, 361.7f}, {-0.28340811f, 0.07395907f, 0.00019359f, 1.76187114e-05f, 0.f}, 4},
        {"k3", {690.0f, 689.0f, 635.5f, 355.25f}, {-0.21f, 0.035f, 0.0004f, -0.0007f, 0.012f}, 5},
        {"neg_icdist", {650.0f, 650.0f, 640.0f, 360.0f}, {-2.0f, 0.0f, 0.001f, 0.001f, 0.f}, 4},
    };
    // a 1280 x 720 lattice (corners included) and a coarser one reaching 400 px beyond every border
    std::vector<float> pts;
    for (int j = 0; j <= 36; j++)
        for (int i = 0; i <= 64; i++) {
            pts.push_back(i * 20.0f);
            pts.push_back(j * 20.0f);
        }
    for (int j = 0; j <= 26; j++)
        for (int i = 0; i <= 41; i++) {
            pts.push_back(-400.0f + i * 50.75f);
            pts.push_back(-300.0f + j * 50.5f);
        }
    const int n = (int)pts.size() / 2;
    for (const Cam& c : cams) {
        cv::Mat mK = (cv::Mat_<float>(3, 3) << c.K[0], 0.f, c.K[2], 0.f, c.K[1], c.K[3], 0.f, 0.f, 1.f);
        cv::Mat mDistCoef(c.nd, 1, CV_32F);
        for (int i = 0; i < c.nd; i++) mDistCoef.at<float>(i) = c.D[i];
        cv::Mat mat(n, 2, CV_32F);
        for (int i = 0; i < n; i++) {
            mat.at<float>(i, 0) = pts[2 * i];
            mat.at<float>(i, 1) = pts[2 * i + 1];
        }
        mat = mat.reshape(2);
        cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK);
        mat = mat.reshape(1);
        std::vector<float> out;
        for (int i = 0; i < n; i++) {
            out.push_back(pts[2 * i]);
            out.push_back(pts[2 * i + 1]);
            out.push_back(mat.at<float>(i, 0));
            out.push_back(mat.at<float>(i, 1));
        }
        const float cam[10] = {c.K[0], c.K[1], c.K[2], c.K[3], c.D[0], c.D[1], c.D[2], c.D[3], c.D[4], (float)c.nd};
        write_blob(dir + "/out_undistort_" + c.name + "_cam.bin", 9, {10}, cam, sizeof(cam));
        write_blob(dir + "/out_undistort_" + c.name + ".bin", 8, {(uint32_t)n, 4}, out.data(), out.size() * 4);
    }
    printf("wrote %s/out_undistort_*.bin (OpenCV %s)\n", dir.c_str(), CV_VERSION);
    return 0;
}
