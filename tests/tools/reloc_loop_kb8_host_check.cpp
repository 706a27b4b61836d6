/* The host twins of the relocalisation and the loop-closing SearchByProjection for fisheye cameras
 * (vslamh_search_by_projection_keyframe_kb8, vslamh_search_by_projection_sim3_kb8, vi_slam_amd/csrc/vslam_match_host.cpp) as a
 * program of its own, for a sanitizer build on the CPU:
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include \
 *       tests/tools/reloc_loop_kb8_host_check.cpp \
 *       $(make -s -C vi_slam_amd/csrc print-host-srcs P=vi_slam_amd/csrc/) -o reloc_loop_kb8_host_check
 *   reloc_loop_kb8_host_check case.bin ..      (written by tests/tools/dump_reloc_loop_kb8_cases.py)
 * case.bin starts with eight int32, the first of them 0 (A) or 1 (B), and six floats.
 *   A: 0, n_kf, n_cur, nlevels, gemm_float, check_orientation, orb_dist, has_occupied; th, log_scale_factor, bounds[4]; the
 *      camera (9 floats); scale factors; Tcw (12); Ow (3); the KeyFrame keypoints, flags, positions, min and max distances,
 *      descriptors; the current keypoints and descriptors; the occupancy bytes; the expected nmatches and match_cur
 *   B: 1, n_jobs, n_points, nlevels, gemm_float, th, 0, 0; ratio_hamming, log_scale_factor, bounds[4]; the camera; scale
 *      factors; the points (vslam_fuse_point) and their descriptors; per job int32 n_kf, has_matched, has_valid, 15 floats
 *      Rcw | tcw | Ow, the keypoints, the descriptors, the matched bytes, the validity bytes, the expected nmatches, n_gated and
 *      match_kf
 * Every array is an allocation of its own, so that a read past its end is a read past an allocation.  Exit 0 when the twins
 * reproduce every file. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_fe.h"

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

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "short file\n");
        std::exit(2);
    }
    return v;
}

static vslam_kb8_camera camera(const std::vector<float>& v) {
    vslam_kb8_camera c;
    c.fx = v[0]; c.fy = v[1]; c.cx = v[2]; c.cy = v[3];
    for (int i = 0; i < 4; i++) c.k[i] = v[4 + i];
    c.precision = v[8];
    return c;
}

static int run_a(const char* path, FILE* f, const std::vector<int32_t>& hd, const std::vector<float>& fl) {
    const int n = hd[1], n2 = hd[2], nlevels = hd[3];
    const std::vector<float> bounds(fl.begin() + 2, fl.end());
    const vslam_kb8_camera cam = camera(take<float>(f, 9));
    const std::vector<float> sf = take<float>(f, nlevels), T = take<float>(f, 12), Ow = take<float>(f, 3);
    const std::vector<vslam_kp> kf = take<vslam_kp>(f, n);
    const std::vector<uint8_t> flags = take<uint8_t>(f, n);
    const std::vector<float> x3 = take<float>(f, (size_t)n * 3), mn = take<float>(f, n), mx = take<float>(f, n);
    const std::vector<uint8_t> desc = take<uint8_t>(f, (size_t)n * 32);
    const std::vector<vslam_kp> cur = take<vslam_kp>(f, n2);
    const std::vector<uint8_t> cdesc = take<uint8_t>(f, (size_t)n2 * 32);
    const std::vector<uint8_t> occ = take<uint8_t>(f, hd[7] ? n2 : 0);
    const std::vector<int32_t> want_n = take<int32_t>(f, 1), want = take<int32_t>(f, n2);
    vslam_proj_params p;
    std::memset(&p, 0, sizeof(p));
    std::memcpy(p.Tcw, T.data(), sizeof(p.Tcw));
    p.fx = cam.fx; p.fy = cam.fy; p.cx = cam.cx; p.cy = cam.cy;
    p.th = fl[0];
    p.check_orientation = hd[5];
    p.img_w = (int)fl[3];
    p.img_h = (int)fl[5];
    p.gemm_float = hd[4];
    std::vector<int32_t> m((size_t)n2, 7);
    int nm = 7;
    const int rc = vslamh_search_by_projection_keyframe_kb8(&p, &cam, Ow.data(), fl[1], hd[6], n ? kf.data() : nullptr, n,
                                                            n ? flags.data() : nullptr, n ? x3.data() : nullptr,
                                                            n ? mn.data() : nullptr, n ? mx.data() : nullptr,
                                                            n ? desc.data() : nullptr, n2 ? cur.data() : nullptr,
                                                            n2 ? cdesc.data() : nullptr, n2, (hd[7] && n2) ? occ.data() : nullptr,
                                                            sf.data(), nlevels, bounds.data(), n2 ? m.data() : nullptr, &nm);
    if (rc != 0 || nm != want_n[0] || m != want) {
        std::fprintf(stderr, "%s: mismatch: rc %d, nmatches %d (want %d)\n", path, rc, nm, want_n[0]);
        return 1;
    }
    std::printf("ok: %s: A, %d entries, %d keypoints, %d matches\n", path, n, n2, nm);
    return 0;
}

static int run_b(const char* path, FILE* f, const std::vector<int32_t>& hd, const std::vector<float>& fl) {
    const int nj = hd[1], n = hd[2], nlevels = hd[3];
    const std::vector<float> bounds(fl.begin() + 2, fl.end());
    const vslam_kb8_camera cam = camera(take<float>(f, 9));
    const std::vector<float> sf = take<float>(f, nlevels);
    const std::vector<vslam_fuse_point> pts = take<vslam_fuse_point>(f, n);
    const std::vector<uint8_t> desc = take<uint8_t>(f, (size_t)n * 32);
    vslam_sim3_kb8_params p;
    std::memset(&p, 0, sizeof(p));
    p.th = hd[5];
    p.ratio_hamming = fl[0];
    p.log_scale_factor = fl[1];
    p.img_w = (int)fl[3];
    p.img_h = (int)fl[5];
    p.gemm_float = hd[4];
    std::vector<vslam_sim3_kb8_job> jobs((size_t)nj);
    std::vector<std::vector<vslam_kp>> kps((size_t)nj);
    std::vector<std::vector<uint8_t>> kd((size_t)nj), matched((size_t)nj), valid((size_t)nj);
    std::vector<std::vector<int32_t>> want((size_t)nj), got((size_t)nj);
    std::vector<int32_t*> out((size_t)nj);
    std::vector<int> want_nm, want_ng;
    for (int j = 0; j < nj; j++) {
        const std::vector<int32_t> jh = take<int32_t>(f, 3);
        const std::vector<float> pose = take<float>(f, 15);
        kps[j] = take<vslam_kp>(f, jh[0]);
        kd[j] = take<uint8_t>(f, (size_t)jh[0] * 32);
        if (jh[1]) matched[j] = take<uint8_t>(f, jh[0]);
        if (jh[2]) valid[j] = take<uint8_t>(f, n);
        const std::vector<int32_t> cnt = take<int32_t>(f, 2);
        want_nm.push_back(cnt[0]);
        want_ng.push_back(cnt[1]);
        want[j] = take<int32_t>(f, jh[0]);
        got[j].assign((size_t)jh[0], 7);
        out[j] = jh[0] ? got[j].data() : nullptr;
        vslam_sim3_kb8_job& s = jobs[j];
        std::memset(&s, 0, sizeof(s));
        std::memcpy(s.Rcw, pose.data(), sizeof(s.Rcw));
        std::memcpy(s.tcw, pose.data() + 9, sizeof(s.tcw));
        std::memcpy(s.Ow, pose.data() + 12, sizeof(s.Ow));
        s.n_kf = jh[0];
        s.dev_kps = jh[0] ? kps[j].data() : nullptr;
        s.dev_desc = jh[0] ? kd[j].data() : nullptr;
        s.kf_matched_host = (jh[1] && jh[0]) ? matched[j].data() : nullptr;
        s.valid_host = (jh[2] && n) ? valid[j].data() : nullptr;
    }
    std::vector<int> nm((size_t)nj, 7), ng((size_t)nj, 7);
    const int rc = vslamh_search_by_projection_sim3_kb8(&p, &cam, jobs.data(), nj, n ? pts.data() : nullptr, n ? desc.data() : nullptr,
                                                        n, sf.data(), nlevels, bounds.data(), out.data(), nm.data(), ng.data());
    if (rc != 0 || nm != want_nm || ng != want_ng || got != want) {
        std::fprintf(stderr, "%s: mismatch: rc %d\n", path, rc);
        return 1;
    }
    long found = 0;
    for (int v : nm) found += v;
    std::printf("ok: %s: B, %d jobs, %d points, %ld matches\n", path, nj, n, found);
    return 0;
}

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = take<int32_t>(f, 8);
    const std::vector<float> fl = take<float>(f, 6);
    const int rc = hd[0] == 0 ? run_a(path, f, hd, fl) : run_b(path, f, hd, fl);
    std::fclose(f);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    for (int i = 1; i < argc; i++)
        if (int rc = run(argv[i])) return rc;
    return 0;
}
