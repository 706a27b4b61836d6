/* The host twin of the rig motion-model matcher (vslamh_search_by_projection_frame_rig, vi_slam_amd/csrc/vslam_match_host.cpp) as
 * a program of its own, for a sanitizer build on the CPU:
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include \
 *       tests/tools/frame_rig_host_check.cpp \
 *       $(make -s -C vi_slam_amd/csrc print-host-srcs P=vi_slam_amd/csrc/) -o frame_rig_host_check
 *   frame_rig_host_check case.bin      (written by tests/tools/dump_frame_rig_case.py)
 * case.bin: int32 n_last, n_left, n_right, has_occ, nlevels; one vslam_proj_params; one vslam_kb8_camera; float Trl[12],
 * bounds[4], scale[nlevels]; then last-frame keypoints, flags, positions, descriptors, left keypoints, left descriptors, right
 * keypoints, right descriptors, [occupied], and the expected nmatches (int32) and match table (int32 x (n_left + n_right)).
 * Exit 0 when the twin reproduces them. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_fe.h"

extern "C" int vslamh_search_by_projection_frame_rig(const vslam_proj_params*, const vslam_kb8_camera*, const float*, const vslam_kp*,
                                                     int, const uint8_t*, const float*, const uint8_t*, const vslam_kp*,
                                                     const uint8_t*, int, const vslam_kp*, const uint8_t*, int, const uint8_t*,
                                                     const float*, int, const float*, int32_t*, int*);

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
    const int n = hd[0], nl = hd[1], nr = hd[2], has_occ = hd[3], nlevels = hd[4];
    const auto p = take<vslam_proj_params>(f, 1);
    const auto cam = take<vslam_kb8_camera>(f, 1);
    const std::vector<float> fl = take<float>(f, 16 + (size_t)nlevels);
    const auto kp = take<vslam_kp>(f, n);
    const auto flags = take<uint8_t>(f, n);
    const auto xw = take<float>(f, (size_t)n * 3);
    const auto desc = take<uint8_t>(f, (size_t)n * 32);
    const auto kl = take<vslam_kp>(f, nl);
    const auto dl = take<uint8_t>(f, (size_t)nl * 32);
    const auto kr = take<vslam_kp>(f, nr);
    const auto dr = take<uint8_t>(f, (size_t)nr * 32);
    const auto occ = take<uint8_t>(f, has_occ ? (size_t)(nl + nr) : 0);
    const auto want_nm = take<int32_t>(f, 1), want = take<int32_t>(f, (size_t)(nl + nr));
    std::fclose(f);
    std::vector<int32_t> m((size_t)(nl + nr));
    int nm = -1;
    const int rc = vslamh_search_by_projection_frame_rig(p.data(), cam.data(), fl.data(), kp.data(), n, flags.data(), xw.data(),
                                                         desc.data(), kl.data(), dl.data(), nl, kr.data(), dr.data(), nr,
                                                         has_occ ? occ.data() : nullptr, fl.data() + 16, nlevels, fl.data() + 12,
                                                         m.data(), &nm);
    if (rc != 0 || nm != want_nm[0] || m != want) {
        std::fprintf(stderr, "mismatch: rc %d nmatches %d (want %d)\n", rc, nm, want_nm[0]);
        return 1;
    }
    std::printf("ok: %d last-frame entries, %d + %d keypoints, %d matches\n", n, nl, nr, nm);
    return 0;
}
