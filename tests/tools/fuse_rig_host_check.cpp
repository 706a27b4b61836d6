/* The host twin of the rig Fuse search (vslamh_fuse_search_rig, vi_slam_amd/csrc/vslam_match_host.cpp) as a program of its
 * own, for a sanitizer build on the CPU:
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include \
 *       tests/tools/fuse_rig_host_check.cpp \
 *       $(make -s -C vi_slam_amd/csrc print-host-srcs P=vi_slam_amd/csrc/) -o fuse_rig_host_check
 *   fuse_rig_host_check case.bin ..      (written by tests/tools/dump_fuse_rig_cases.py)
 * case.bin: int32 n_jobs, n_points, nlevels, gemm_float; float th, log_scale_factor, bounds[4]; the two cameras (9 floats each);
 * Tlr, Trl (12 floats each); scale factors and inverse sigma2 (nlevels each); the points (vslam_fuse_point) and their
 * descriptors; per job int32 camera, sim3, n_kf, idx_offset, has_valid, 15 floats Rcw | tcw | Ow, the keypoints, the descriptors
 * and, with has_valid, n_points bytes; the expected best_idx and best_dist (n_jobs * n_points int32 each).  Every array is an
 * allocation of its own, so that a read past its end is a read past an allocation.  Exit 0 when the twin reproduces every file. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_fe.h"

extern "C" int vslamh_fuse_search_rig(const vslam_fuse_params* p, const vslam_kb8_camera* cam, const vslam_kb8_rig* rig,
                                      const vslam_fuse_rig_job* jobs, int n_jobs, const vslam_fuse_point* points,
                                      const uint8_t* mp_desc, int n_points, const float* scale_factors, const float* inv_sigma2,
                                      int nlevels, const float* bounds, int32_t* best_idx, int32_t* best_dist);

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

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = take<int32_t>(f, 4);
    const int nj = hd[0], n = hd[1], nlevels = hd[2];
    const std::vector<float> fl = take<float>(f, 6);
    vslam_fuse_params p;
    std::memset(&p, 0, sizeof(p));
    p.th = fl[0];
    p.log_scale_factor = fl[1];
    p.img_w = (int)fl[3];
    p.img_h = (int)fl[5];
    p.gemm_float = hd[3];
    const std::vector<float> bounds(fl.begin() + 2, fl.end());
    const vslam_kb8_camera cam1 = camera(take<float>(f, 9));
    vslam_kb8_rig rig;
    rig.cam2 = camera(take<float>(f, 9));
    const std::vector<float> tlr = take<float>(f, 12), trl = take<float>(f, 12);
    std::memcpy(rig.Tlr, tlr.data(), sizeof(rig.Tlr));
    std::memcpy(rig.Trl, trl.data(), sizeof(rig.Trl));
    const std::vector<float> sf = take<float>(f, nlevels), is2 = take<float>(f, nlevels);
    const std::vector<vslam_fuse_point> pts = take<vslam_fuse_point>(f, n);
    const std::vector<uint8_t> desc = take<uint8_t>(f, (size_t)n * 32);
    std::vector<vslam_fuse_rig_job> jobs((size_t)nj);
    std::vector<std::vector<vslam_kp>> kps((size_t)nj);
    std::vector<std::vector<uint8_t>> kd((size_t)nj), valid((size_t)nj);
    for (int j = 0; j < nj; j++) {
        const std::vector<int32_t> jh = take<int32_t>(f, 5);
        const std::vector<float> pose = take<float>(f, 15);
        kps[j] = take<vslam_kp>(f, jh[2]);
        kd[j] = take<uint8_t>(f, (size_t)jh[2] * 32);
        if (jh[4]) valid[j] = take<uint8_t>(f, n);
        vslam_fuse_rig_job& s = jobs[j];
        std::memset(&s, 0, sizeof(s));
        std::memcpy(s.Rcw, pose.data(), sizeof(s.Rcw));
        std::memcpy(s.tcw, pose.data() + 9, sizeof(s.tcw));
        std::memcpy(s.Ow, pose.data() + 12, sizeof(s.Ow));
        s.camera = jh[0];
        s.sim3 = jh[1];
        s.n_kf = jh[2];
        s.idx_offset = jh[3];
        s.dev_kps = jh[2] ? kps[j].data() : nullptr;
        s.dev_desc = jh[2] ? kd[j].data() : nullptr;
        s.valid_host = jh[4] && n ? valid[j].data() : nullptr;
    }
    const size_t total = (size_t)nj * n;
    const std::vector<int32_t> want_i = take<int32_t>(f, total), want_d = take<int32_t>(f, total);
    std::fclose(f);
    std::vector<int32_t> bi(total, 7), bd(total, 7);
    const int rc = vslamh_fuse_search_rig(&p, &cam1, &rig, jobs.data(), nj, pts.data(), desc.data(), n, sf.data(), is2.data(),
                                          nlevels, bounds.data(), bi.data(), bd.data());
    if (rc != 0 || bi != want_i || bd != want_d) {
        size_t bad = 0;
        while (bad < total && bi[bad] == want_i[bad] && bd[bad] == want_d[bad]) bad++;
        std::fprintf(stderr, "%s: mismatch: rc %d, first at %zu\n", path, rc, bad);
        return 1;
    }
    size_t found = 0;
    for (size_t i = 0; i < total; i++) found += bi[i] >= 0;
    std::printf("ok: %s: %d jobs, %d points, %zu found\n", path, nj, n, found);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    for (int i = 1; i < argc; i++)
        if (int rc = run(argv[i])) return rc;
    return 0;
}
