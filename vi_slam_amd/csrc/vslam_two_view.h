/* vslam_two_view.h -- MotionEstimator::CheckHomography (motion_estimation.cpp:2277-2360) and CheckFundamental (:2362-2440)
 * for one pair under one hypothesis, and the selection of FindHomography / FindFundamental (:2120-2143, :2171-2194), written
 * once for the device (k_tv_score, k_tv_select in vslam_two_view.hip) and the host (vslamh_two_view_score in vslam_match_host.cpp:
 * CPU tests and the stand-alone demo, not a fallback of the product).
 *
 * What the reference evaluates per pair (u1, v1) = mvKeys1[i].pt, (u2, v2) = mvKeys2[j].pt, in its order:
 *   CheckHomography   w2in1inv = 1.0 / (h31inv*u2 + h32inv*v2 + h33inv)       the 1.0 is a double: a double division rounded
 *                                  to float, which equals the correctly rounded float division for every float divisor
 *                                  (53 >= 2*24 + 2), so it is fdvd(1.0f, x)
 *                     u2in1 = (h11inv*u2 + h12inv*v2 + h13inv) * w2in1inv,   v2in1 alike
 *                     squareDist1 = (u1-u2in1)*(u1-u2in1) + (v1-v2in1)*(v1-v2in1)
 *                     chiSquare1 = squareDist1 * invSigmaSquare;   if (chiSquare1 > th) bIn = false; else score += th - chiSquare1
 *                     the same for image 2 with H21; th = 5.991f
 *   CheckFundamental  a2, b2, c2 = F21 * x1;  num2 = a2*u2 + b2*v2 + c2;  squareDist1 = num2*num2 / (a2*a2 + b2*b2)
 *                     chiSquare1 = squareDist1 * invSigmaSquare;   if (chiSquare1 > 3.841f) bIn = false; else score += 5.991f - chiSquare1
 *                     then the transposed line a1 = f11*u2 + f21*v2 + f31, b1 = f12*u2 + f22*v2 + f32, c1 = f13*u2 + f23*v2 + f33
 *   invSigmaSquare = 1.0 / (sigma*sigma): a float product, a double division, rounded to float (inv_sigma_square, host only)
 * Every expression associates left to right as C reads it and every operation is rounded on its own: the reference builds
 * with -O3 and no -march (CMakeLists.txt:14-15), so x86-64 contracts nothing.  Subnormals are kept.
 *
 * NaN: `chi > th` is false for a NaN chi, so the pair stays an inlier and th - chi = NaN goes into the score; the term
 * functions below return exactly that.  An outlier's term is +0.0f: the reference does not add there, but s + 0.0f == s
 * bit for bit for every s the chain can hold (it starts at +0 and every term is >= +0 or NaN, so it is never -0), which
 * lets a chain have a fixed length.
 *
 * Contraction: on the device every operation goes through the _rn intrinsics; host builds rely on -ffp-contract=off
 * (vi_slam_amd/csrc/Makefile).
 */
#ifndef VSLAM_TWO_VIEW_H
#define VSLAM_TWO_VIEW_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vslam_fe.h"
#include "vslam_matchdev.h"

namespace vslam_tv {

using namespace vslam_md; /* fmul, fadd, fsub, fdvd */

/* the two score terms of one pair (image 1, image 2; +0 where the pair is an outlier there) and vbCurrentInliers[i] */
struct Terms {
    float t1, t2;
    bool in;
};

struct Mat3 {
    float m[9]; /* row-major */
};

VSLAM_HD Mat3 load_mat3(const float* p) {
    Mat3 M;
    for (int k = 0; k < 9; k++) M.m[k] = p[k];
    return M;
}

/* r0*x + r1*y + r2, as C reads it */
VSLAM_HD float row_xy1(float r0, float r1, float r2, float x, float y) { return fadd(fadd(fmul(r0, x), fmul(r1, y)), r2); }

/* `if (chi > th) bIn = false; else score += thScore - chi;` -- what is added, and whether bIn survives (results by value:
 * vslam_matchdev.h) */
VSLAM_HD float term_of(float chi, float th, float thScore) { return chi > th ? 0.0f : fsub(thScore, chi); }
VSLAM_HD bool keeps_in(float chi, float th) { return !(chi > th); }

/* squared reprojection error of (pu, pv) against M * (qu, qv, 1), times invSigmaSquare (CheckHomography, one image) */
VSLAM_HD float chi_h(const Mat3& M, float pu, float pv, float qu, float qv, float invSigmaSquare) {
    const float winv = fdvd(1.0f, row_xy1(M.m[6], M.m[7], M.m[8], qu, qv));
    const float u = fmul(row_xy1(M.m[0], M.m[1], M.m[2], qu, qv), winv);
    const float v = fmul(row_xy1(M.m[3], M.m[4], M.m[5], qu, qv), winv);
    const float du = fsub(pu, u), dv = fsub(pv, v);
    return fmul(fadd(fmul(du, du), fmul(dv, dv)), invSigmaSquare);
}

VSLAM_HD Terms check_h(const Mat3& H21, const Mat3& H12, float u1, float v1, float u2, float v2, float invSigmaSquare) {
    const float chi1 = chi_h(H12, u1, v1, u2, v2, invSigmaSquare); /* x2in1 = H12 * x2 */
    const float chi2 = chi_h(H21, u2, v2, u1, v1, invSigmaSquare); /* x1in2 = H21 * x1 */
    return Terms{term_of(chi1, 5.991f, 5.991f), term_of(chi2, 5.991f, 5.991f), keeps_in(chi1, 5.991f) && keeps_in(chi2, 5.991f)};
}

/* squared distance of (pu, pv) to the line (a, b, c), times invSigmaSquare (CheckFundamental, one image) */
VSLAM_HD float chi_f(float a, float b, float c, float pu, float pv, float invSigmaSquare) {
    const float num = fadd(fadd(fmul(a, pu), fmul(b, pv)), c);
    const float sq = fdvd(fmul(num, num), fadd(fmul(a, a), fmul(b, b)));
    return fmul(sq, invSigmaSquare);
}

VSLAM_HD Terms check_f(const Mat3& F, float u1, float v1, float u2, float v2, float invSigmaSquare) {
    /* l2 = F21 * x1 */
    const float a2 = row_xy1(F.m[0], F.m[1], F.m[2], u1, v1);
    const float b2 = row_xy1(F.m[3], F.m[4], F.m[5], u1, v1);
    const float c2 = row_xy1(F.m[6], F.m[7], F.m[8], u1, v1);
    const float chi1 = chi_f(a2, b2, c2, u2, v2, invSigmaSquare);
    /* l1 = x2^T * F21 */
    const float a1 = row_xy1(F.m[0], F.m[3], F.m[6], u2, v2);
    const float b1 = row_xy1(F.m[1], F.m[4], F.m[7], u2, v2);
    const float c1 = row_xy1(F.m[2], F.m[5], F.m[8], u2, v2);
    const float chi2 = chi_f(a1, b1, c1, u1, v1, invSigmaSquare);
    return Terms{term_of(chi1, 3.841f, 5.991f), term_of(chi2, 3.841f, 5.991f), keeps_in(chi1, 3.841f) && keeps_in(chi2, 3.841f)};
}

/* a score as it is reported: a NaN becomes the quiet NaN 0x7fc00000 (include/vslam_fe.h, deviations) */
VSLAM_HD float report_score(float s) {
    if (s == s) return s;
    const uint32_t q = 0x7fc00000u;
    float r;
    memcpy(&r, &q, 4);
    return r;
}

/* `if (currentScore > score)` against a running best that starts at (0, no winner) */
struct Best {
    float score;
    int32_t index;
};
VSLAM_HD Best best_none() { return Best{0.0f, -1}; }
VSLAM_HD Best best_take(Best b, float currentScore, int32_t it) { return currentScore > b.score ? Best{currentScore, it} : b; }
/* two running bests over disjoint index sets: the larger score, the lower index among equal ones */
VSLAM_HD Best best_merge(Best a, Best b) {
    if (b.index < 0) return a;
    if (a.index < 0) return b;
    if (b.score > a.score || (b.score == a.score && b.index < a.index)) return b;
    return a;
}

/* 1.0 / (sigma*sigma) of both checks */
static inline float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

} // namespace vslam_tv

/* The three launches of the two-view stage (vslam_two_view.hip).  One TvJobDev per job, in HBM (uploaded with the
 * hypotheses); every pointer a DEVICE pointer.
 * Inlier flags of every hypothesis: bit (p & 7) of byte flags[(p >> 3) * (nH + nF) + column], column = the H hypothesis'
 * index, or nH + the F hypothesis' index -- the 64 lanes of a wave write 64 neighbouring bytes. */
#define VSLAM_TV_SCORE_LANES 64 /* hypotheses per workgroup of k_tv_score, one per lane of each wave */
#define VSLAM_TV_SCORE_WAVES 8  /* waves per workgroup */
#define VSLAM_TV_WAVE_PAIRS 8   /* pairs a wave takes per round: its flags are one byte */
#define VSLAM_TV_STAGE_PAIRS (VSLAM_TV_SCORE_WAVES * VSLAM_TV_WAVE_PAIRS) /* pairs per round: 64 x 2 x 64 terms = 32 KB of LDS, twice */
#define VSLAM_TV_HDR_WORDS 8
enum { TV_HDR_N = 0, TV_HDR_USED = 1, TV_HDR_ERR = 2, TV_HDR_BEST_H = 3, TV_HDR_BEST_F = 4, TV_HDR_SCORE_H = 5, TV_HDR_SCORE_F = 6 };
struct TvJobDev {
    const float* xy1; /* x of keypoint i at xy1[i * stride1], y behind it */
    const float* xy2;
    const int32_t* matches; /* n1 */
    int32_t stride1, stride2; /* floats per keypoint: 7 (vslam_kp) or 2 (packed by the host) */
    int32_t n1, n2, cap;      /* cap: slots of pts / pairs / masks, min(n1, VSLAM_TWO_VIEW_MAX_PAIRS) */
    int32_t nH, nF;
    float invSigmaSquare;
    const float* H21; /* nH x 9 */
    const float* H12;
    const float* F21; /* nF x 9 */
    float* pts;       /* scratch: cap x (u1, v1, u2, v2), 16-byte aligned */
    uint8_t* flags;   /* scratch: ceil(cap / 8) x (nH + nF) bytes */
    int32_t* hdr;     /* result block: [TV_HDR_N] pairs found, [TV_HDR_USED] pairs scored (0 on overflow or error),
                         [TV_HDR_ERR] a matches entry >= n2, best_h, best_f, score_h, score_f (float words) */
    int32_t* pairs;   /* result block: cap x (i, matches[i]) */
    float* scoresH;   /* result block: nH, nF */
    float* scoresF;
    uint8_t* inlH;    /* result block: cap each */
    uint8_t* inlF;
};
#endif
