/* A fisheye Frame through include/vslam_shim.hpp: one frame extracted, a KannalaBrandt8 camera attached to its extractor,
 * project over the MapPoints' positions, unproject over the frame's keypoints, then Tracking::SearchLocalPoints
 * (FMatcher::SearchLocalPoints) with the fisheye frustum test.  Output: one line of JSON with the counts and FNV-1a checksums
 * for the pytest driver.
 *   kb8_demo W H image.raw nfeatures camera.bin params.bin points.bin desc.bin npoints th
 * camera.bin = one vslam_kb8_camera, params.bin = one vslam_frustum_params, points.bin = npoints vslam_map_point,
 * desc.bin = npoints x 32 bytes.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "vslam_shim.hpp"

using namespace vi_slam_amd::geometry;

static std::vector<uint8_t> load(const char* path, size_t bytes) {
    std::vector<uint8_t> m(bytes);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(m.data(), 1, bytes, f) != bytes) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return m;
}

static unsigned long long fnv(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), nf = std::atoi(argv[4]), n = std::atoi(argv[9]);
    const float th = std::strtof(argv[10], nullptr);
    static_assert(sizeof(vslam_map_point) == 36 && sizeof(vslam_frustum_params) == 104 && sizeof(vslam_kb8_camera) == 36,
                  "file layouts");
    try {
        std::vector<uint8_t> img = load(argv[3], (size_t)w * h), cb = load(argv[5], sizeof(vslam_kb8_camera)),
                             pb = load(argv[6], sizeof(vslam_frustum_params)),
                             ptb = load(argv[7], (size_t)n * sizeof(vslam_map_point)), desc = load(argv[8], (size_t)n * 32);
        vslam_kb8_camera c;
        std::memcpy(&c, cb.data(), sizeof(c));
        vslam_frustum_params p;
        std::memcpy(&p, pb.data(), sizeof(p));
        std::vector<vslam_map_point> pts((size_t)n);
        if (n) std::memcpy(pts.data(), ptb.data(), ptb.size());
        FExtractor ex(nf, 1.2f, 8, 20, 7);
        Mat8u im(h, w, img.data(), (size_t)w), mask, d;
        std::vector<KeyPoint> k;
        std::vector<int> nolap = {0, 0};
        ex.compute(im, mask, k, d, nolap);
        KannalaBrandt8 cam(ex, {c.fx, c.fy, c.cx, c.cy, c.k[0], c.k[1], c.k[2], c.k[3]}, c.precision);
        std::vector<Point3f> xyz((size_t)n), rays;
        for (int i = 0; i < n; i++) xyz[i] = Point3f{pts[i].pos[0], pts[i].pos[1], pts[i].pos[2]};
        std::vector<Point2f> uv, px(k.size());
        for (size_t i = 0; i < k.size(); i++) px[i] = k[i].pt;
        cam.project(xyz, uv);
        cam.unproject(px, rays);
        const Point3f one = k.empty() ? Point3f{0, 0, 1} : cam.unproject(px[0]);
        if (!k.empty() && std::memcmp(&one, &rays[0], sizeof(one)) != 0) throw std::runtime_error("single and batch unproject differ");
        FMatcher::LocalFrameView cur;
        cur.frame.ukeypoints = &k;
        cur.frame.extractor = &ex;
        cur.frame.mnMaxX = w;
        cur.frame.mnMaxY = h;
        std::memcpy(cur.Tcw, p.Tcw, sizeof(cur.Tcw));
        std::memcpy(cur.Ow, p.Ow, sizeof(cur.Ow));
        cur.fx = p.fx; cur.fy = p.fy; cur.cx = p.cx; cur.cy = p.cy; cur.mbf = p.mbf;
        cur.mfLogScaleFactor = p.log_scale_factor;
        FMatcher matcher(0.8f, true);
        std::vector<int> idx;
        std::vector<vslam_mp_track> track;
        int nToMatch = 0;
        const int nm = matcher.SearchLocalPoints(cur, pts, desc, nullptr, th, p.far_points != 0, p.th_far_points, idx, nToMatch,
                                                 &track, p.viewing_cos_limit);
        std::printf("{\"n_cur\": %d, \"nmatches\": %d, \"n_to_match\": %d, \"match\": %llu, \"track\": %llu, \"uv\": %llu, "
                    "\"rays\": %llu}\n",
                    (int)k.size(), nm, nToMatch, fnv(idx.data(), idx.size() * sizeof(int)),
                    fnv(track.data(), track.size() * sizeof(vslam_mp_track)), fnv(uv.data(), uv.size() * sizeof(Point2f)),
                    fnv(rays.data(), rays.size() * sizeof(Point3f)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kb8_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
