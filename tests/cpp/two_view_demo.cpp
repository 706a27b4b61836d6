/* The monocular initialiser's consensus through include/vslam_shim.hpp: two frames extracted, FMatcher::SearchForInitialization,
 * then MotionEstimator::Check -- CheckHomography / CheckFundamental of every hypothesis and the selection of FindHomography /
 * FindFundamental in one call.  The hypotheses come from a file: computing them (ComputeH21 / ComputeF21) is the caller's.
 * Output: one line of JSON with the counts, the scores as words and FNV-1a checksums for the pytest driver.
 *   two_view_demo W H image1.raw image2.raw nfeatures window hyp.bin nH nF
 * hyp.bin = nH x 9 floats H21, nH x 9 floats H12, nF x 9 floats F21.
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

static unsigned word(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

static std::vector<uint8_t> bytes_of(const std::vector<bool>& v) {
    std::vector<uint8_t> o(v.size());
    for (size_t i = 0; i < v.size(); i++) o[i] = v[i] ? 1 : 0;
    return o;
}

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), nf = std::atoi(argv[5]), window = std::atoi(argv[6]);
    const int nH = std::atoi(argv[8]), nF = std::atoi(argv[9]);
    try {
        std::vector<uint8_t> img1 = load(argv[3], (size_t)w * h), img2 = load(argv[4], (size_t)w * h);
        std::vector<uint8_t> hyp = load(argv[7], (size_t)(2 * nH + nF) * sizeof(Mat3f));
        std::vector<Mat3f> vH21((size_t)nH), vH12((size_t)nH), vF21((size_t)nF);
        if (nH) std::memcpy(vH21.data(), hyp.data(), (size_t)nH * sizeof(Mat3f));
        if (nH) std::memcpy(vH12.data(), hyp.data() + (size_t)nH * sizeof(Mat3f), (size_t)nH * sizeof(Mat3f));
        if (nF) std::memcpy(vF21.data(), hyp.data() + (size_t)2 * nH * sizeof(Mat3f), (size_t)nF * sizeof(Mat3f));
        FExtractor ex1(nf, 1.2f, 8, 20, 7), ex2(nf, 1.2f, 8, 20, 7);
        Mat8u im1(h, w, img1.data(), (size_t)w), im2(h, w, img2.data(), (size_t)w), mask, d1, d2;
        std::vector<KeyPoint> k1, k2;
        std::vector<int> lap = {0, 1000};
        ex1.compute(im1, mask, k1, d1, lap);
        ex2.compute(im2, mask, k2, d2, lap);
        FrameView F1, F2;
        F1.ukeypoints = &k1;
        F1.extractor = &ex1;
        F2.ukeypoints = &k2;
        F2.extractor = &ex2;
        F1.mnMaxX = F2.mnMaxX = w;
        F1.mnMaxY = F2.mnMaxY = h;
        std::vector<Point2f> vbPrevMatched(k1.size());
        for (size_t i = 0; i < k1.size(); i++) vbPrevMatched[i] = k1[i].pt;
        std::vector<int> vnMatches12;
        FMatcher matcher(0.9f, true);
        const int nm = matcher.SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, window);
        MotionEstimator me(ex2, 1.0f);
        MotionEstimator::Consensus c, ch, cf;
        me.Check(k1, k2, vnMatches12, vH21, vH12, vF21, c);
        me.CheckHomographies(k1, k2, vnMatches12, vH21, vH12, ch);
        me.CheckFundamentals(k1, k2, vnMatches12, vF21, cf);
        const bool same = ch.SH == c.SH && ch.bestH == c.bestH && ch.vbMatchesInliersH == c.vbMatchesInliersH && cf.SF == c.SF &&
                          cf.bestF == c.bestF && cf.vbMatchesInliersF == c.vbMatchesInliersF && ch.bestF == -1 && cf.bestH == -1;
        std::vector<int32_t> pairs;
        for (size_t i = 0; i < c.mvMatches12.size(); i++) {
            pairs.push_back(c.mvMatches12[i].first);
            pairs.push_back(c.mvMatches12[i].second);
        }
        const std::vector<uint8_t> inH = bytes_of(c.vbMatchesInliersH), inF = bytes_of(c.vbMatchesInliersF);
        std::printf("{\"nmatches\": %d, \"n_pairs\": %d, \"best_h\": %d, \"best_f\": %d, \"score_h\": %u, \"score_f\": %u, "
                    "\"pairs\": %llu, \"scores_h\": %llu, \"scores_f\": %llu, \"inliers_h\": %llu, \"inliers_f\": %llu, "
                    "\"single_model_calls_agree\": %s}\n",
                    nm, (int)c.mvMatches12.size(), c.bestH, c.bestF, word(c.SH), word(c.SF), fnv(pairs.data(), pairs.size() * 4),
                    fnv(c.vScoresH.data(), c.vScoresH.size() * 4), fnv(c.vScoresF.data(), c.vScoresF.size() * 4),
                    fnv(inH.data(), inH.size()), fnv(inF.data(), inF.size()), same ? "true" : "false");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "two_view_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
