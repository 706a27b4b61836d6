/* The host twin of the rig matcher (vslamh_search_by_projection_mappoints_rig, vi_slam_amd/csrc/vslam_match_host.cpp) as a
 * program of its own, for a sanitizer build on the CPU:
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include \
 *       tests/tools/local_points_rig_host_check.cpp \
 *       $(make -s -C vi_slam_amd/csrc print-host-srcs P=vi_slam_amd/csrc/) -o rig_host_check
 *   rig_host_check case.bin      (written by tests/tools/dump_local_points_rig_case.py)
 * case.bin: int32 n_mp, n_left, n_right, has_occ, nlevels; float th, nnratio, bounds[4], scale[nlevels]; then left records, right
 * records, descriptors, left keypoints, left descriptors, right keypoints, right descriptors, L2R, R2L, [occupied], and the
 * expected nmatches (int32) and match table (int32 x (n_left + n_right)).  Exit 0 when the twin reproduces them. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_fe.h"

extern "C" int vslamh_search_by_projection_mappoints_rig(const vslam_mp_track*, const vslam_mp_track*, const uint8_t*, int,
                                                         const vslam_kp*, const uint8_t*, int, const vslam_kp*, const uint8_t*, int,
                                                         const int32_t*, const int32_t*, const float*, const uint8_t*, const float*,
                                                         int, const float*, float, float, int32_t*, int*);

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "short file\n");
        std::exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = take<int32_t>(f, 5);
    const int n_mp = hd[0], nl = hd[1], nr = hd[2], has_occ = hd[3], nlevels = hd[4];
    const std::vector<float> fl = take<float>(f, 6 + (size_t)nlevels);
    const auto tl = take<vslam_mp_track>(f, n_mp), tr = take<vslam_mp_track>(f, n_mp);
    const auto desc = take<uint8_t>(f, (size_t)n_mp * 32);
    const auto kl = take<vslam_kp>(f, nl);
    const auto dl = take<uint8_t>(f, (size_t)nl * 32);
    const auto kr = take<vslam_kp>(f, nr);
    const auto dr = take<uint8_t>(f, (size_t)nr * 32);
    const auto l2r = take<int32_t>(f, nl), r2l = take<int32_t>(f, nr);
    const auto occ = take<uint8_t>(f, has_occ ? (size_t)(nl + nr) : 0);
    const auto want_nm = take<int32_t>(f, 1), want = take<int32_t>(f, (size_t)(nl + nr));
    std::fclose(f);
    std::vector<int32_t> m((size_t)(nl + nr));
    int nm = -1;
    const int rc = vslamh_search_by_projection_mappoints_rig(tl.data(), tr.data(), desc.data(), n_mp, kl.data(), dl.data(), nl,
                                                             kr.data(), dr.data(), nr, l2r.data(), r2l.data(), nullptr,
                                                             has_occ ? occ.data() : nullptr, fl.data() + 6, nlevels,
                                                             fl.data() + 2, fl[0], fl[1], m.data(), &nm);
    if (rc != 0 || nm != want_nm[0] || m != want) {
        std::fprintf(stderr, "mismatch: rc %d nmatches %d (want %d)\n", rc, nm, want_nm[0]);
        return 1;
    }
    std::printf("ok: %d MapPoints, %d + %d keypoints, %d matches\n", n_mp, nl, nr, nm);
    return 0;
}
