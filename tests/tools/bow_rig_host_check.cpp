/* The host twin of the rig SearchByBoW (vslamh_search_by_bow_rig, vi_slam_amd/csrc/vslam_match_host.cpp) as a program of its
 * own, for a sanitizer build on the CPU:
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include \
 *       tests/tools/bow_rig_host_check.cpp \
 *       $(make -s -C vi_slam_amd/csrc print-host-srcs P=vi_slam_amd/csrc/) -o bow_rig_host_check
 *   bow_rig_host_check case.bin ..      (written by tests/tools/dump_bow_rig_cases.py)
 * case.bin: int32 n_kf, kf_n_left, n_kf_nodes, n_kf_feat, n_f, n_left, n_f_nodes, n_f_feat, check_orientation; float nnratio; then
 * the KeyFrame's keypoints, descriptors, flags, nodes, offsets, features; the frame's keypoints, descriptors, nodes, offsets,
 * features; the expected nmatches (int32) and match table (int32 x n_f).  Exit 0 when the twin reproduces every file. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_fe.h"

extern "C" int vslamh_search_by_bow_rig(const vslam_kp*, const uint8_t*, int, const uint8_t*, int, const uint8_t*, const int32_t*,
                                        const int32_t*, const int32_t*, int, const vslam_kp*, const uint8_t*, int, const vslam_kp*,
                                        const uint8_t*, int, const int32_t*, const int32_t*, const int32_t*, int, float, int,
                                        int32_t*, int*);

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "short file\n");
        std::exit(2);
    }
    return v;
}

/* the halves as arrays of their own, so that a read past a side's end is a read past an allocation */
template <typename T>
static std::vector<T> part(const std::vector<T>& v, size_t first, size_t n, size_t per) {
    return std::vector<T>(v.begin() + first * per, v.begin() + (first + n) * per);
}

static int run(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = take<int32_t>(f, 9);
    const int nk = hd[0], kl = hd[1], nkn = hd[2], nkf = hd[3], n = hd[4], nl = hd[5], nfn = hd[6], nff = hd[7], ori = hd[8];
    const float ratio = take<float>(f, 1)[0];
    const auto kk = take<vslam_kp>(f, nk);
    const auto kd = take<uint8_t>(f, (size_t)nk * 32);
    const auto kfl = take<uint8_t>(f, nk);
    const auto kn = take<int32_t>(f, nkn), ko = take<int32_t>(f, (size_t)nkn + 1), kf = take<int32_t>(f, nkf);
    const auto fk = take<vslam_kp>(f, n);
    const auto fd = take<uint8_t>(f, (size_t)n * 32);
    const auto fn = take<int32_t>(f, nfn), fo = take<int32_t>(f, (size_t)nfn + 1), ff = take<int32_t>(f, nff);
    const auto want_nm = take<int32_t>(f, 1), want = take<int32_t>(f, n);
    std::fclose(f);
    const auto kdl = part(kd, 0, kl, 32), kdr = part(kd, kl, nk - kl, 32);
    const auto fkl = part(fk, 0, nl, 1), fkr = part(fk, nl, n - nl, 1);
    const auto fdl = part(fd, 0, nl, 32), fdr = part(fd, nl, n - nl, 32);
    std::vector<int32_t> m((size_t)n);
    int nm = -1;
    const int rc = vslamh_search_by_bow_rig(kk.data(), kdl.data(), kl, kdr.data(), nk - kl, kfl.data(), kn.data(), ko.data(),
                                            kf.data(), nkn, fkl.data(), fdl.data(), nl, fkr.data(), fdr.data(), n - nl, fn.data(),
                                            fo.data(), ff.data(), nfn, ratio, ori, m.data(), &nm);
    if (rc != 0 || nm != want_nm[0] || m != want) {
        std::fprintf(stderr, "%s: mismatch: rc %d nmatches %d (want %d)\n", path, rc, nm, want_nm[0]);
        return 1;
    }
    std::printf("ok: %s: %d KeyFrame features, %d + %d frame features, %d matches\n", path, nk, nl, n - nl, nm);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    for (int i = 1; i < argc; i++)
        if (int rc = run(argv[i])) return rc;
    return 0;
}
