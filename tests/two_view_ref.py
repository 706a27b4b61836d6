"""Yardstick of the two-view consensus: MotionEstimator::Reconstruct's pair list (motion_estimation.cpp:2017-2029),
CheckHomography (:2277-2360), CheckFundamental (:2362-2440) and the selection of FindHomography / FindFundamental
(:2120-2143, :2171-2194) restated in numpy float32.

Every numpy operation below is ONE rounded float32 operation per element, written in the order C reads the reference's
expressions (left to right, nothing fused: the reference builds with -O3 and no -march).  The score is the serial chain
np.cumsum(terms, dtype=float32)[-1] over the interleaved terms (pair 0 image 1, pair 0 image 2, pair 1 image 1, ...) --
np.cumsum accumulates in index order, unlike np.add.reduce, which sums pairwise.  `1.0 / x` of the reference is a double
division rounded to float, which equals the float division (53 >= 2 * 24 + 2), so the reciprocal is a float32 division.
Shapes: hypotheses along axis 0, pairs along axis 1.
"""
import numpy as np

F32 = np.float32
TH_H = F32(5.991)
TH_F = F32(3.841)
TH_SCORE = F32(5.991)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
MAX_PAIRS = 8192
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def inv_sigma_square(sigma):
    """`const float invSigmaSquare = 1.0/(sigma*sigma)`: float product, double division, rounded to float"""
    s = F32(sigma)
    return F32(1.0 / float(F32(s * s)))


def pair_list(matches12):
    """-> int32 (N, 2): (i, matches12[i]) for ascending i with matches12[i] >= 0"""
    m = np.asarray(matches12, np.int32).reshape(-1)
    i = np.nonzero(m >= 0)[0].astype(np.int32)
    return np.stack([i, m[i]], axis=1).astype(np.int32).reshape(-1, 2)


def gather(xy1, xy2, pairs):
    """-> float32 (N, 4): u1, v1, u2, v2 per pair"""
    xy1 = np.asarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.asarray(xy2, np.float32).reshape(-1, 2)
    return np.concatenate([xy1[pairs[:, 0]], xy2[pairs[:, 1]]], axis=1).astype(np.float32).reshape(-1, 4)


def _row(r0, r1, r2, x, y):
    """r0*x + r1*y + r2; r*: (K, 1), x, y: (1, N)"""
    return (r0 * x + r1 * y) + r2


def _chi_h(M, pu, pv, qu, qv, inv):
    m = [M[:, k:k + 1] for k in range(9)]
    winv = F32(1.0) / _row(m[6], m[7], m[8], qu, qv)
    u = _row(m[0], m[1], m[2], qu, qv) * winv
    v = _row(m[3], m[4], m[5], qu, qv) * winv
    du, dv = pu - u, pv - v
    return (du * du + dv * dv) * inv


def _chi_f(a, b, c, pu, pv, inv):
    num = (a * pu + b * pv) + c
    return ((num * num) / (a * a + b * b)) * inv


def _finish(chi1, chi2, th):
    """-> (scores (K,), inlier flags (K, N) uint8, interleaved terms (K, 2N)); NaN chi: not `> th`, so an inlier whose
    term th - NaN = NaN goes into the chain"""
    with np.errstate(all="ignore"):
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F32(0), TH_SCORE - chi1).astype(np.float32)
        t2 = np.where(out2, F32(0), TH_SCORE - chi2).astype(np.float32)
        K, N = chi1.shape
        terms = np.empty((K, 2 * N), np.float32)
        terms[:, 0::2] = t1
        terms[:, 1::2] = t2
        scores = np.cumsum(terms, axis=1, dtype=np.float32)[:, -1] if N else np.zeros(K, np.float32)
    scores = np.where(np.isnan(scores), QNAN, scores).astype(np.float32)
    return scores, (~out1 & ~out2).astype(np.uint8), terms


def _mats(M):
    return np.ascontiguousarray(M, np.float32).reshape(-1, 9)


def check_homographies(H21, H12, pts, sigma):
    H21, H12 = _mats(H21), _mats(H12)
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    u1, v1, u2, v2 = (pts[:, k][None, :] for k in range(4))
    inv = inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        chi1 = _chi_h(H12, u1, v1, u2, v2, inv)
        chi2 = _chi_h(H21, u2, v2, u1, v1, inv)
    return _finish(chi1, chi2, TH_H)


def check_fundamentals(F21, pts, sigma):
    F = _mats(F21)
    f = [F[:, k:k + 1] for k in range(9)]
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    u1, v1, u2, v2 = (pts[:, k][None, :] for k in range(4))
    inv = inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        a2, b2, c2 = _row(f[0], f[1], f[2], u1, v1), _row(f[3], f[4], f[5], u1, v1), _row(f[6], f[7], f[8], u1, v1)
        chi1 = _chi_f(a2, b2, c2, u2, v2, inv)
        a1, b1, c1 = _row(f[0], f[3], f[6], u2, v2), _row(f[1], f[4], f[7], u2, v2), _row(f[2], f[5], f[8], u2, v2)
        chi2 = _chi_f(a1, b1, c1, u1, v1, inv)
    return _finish(chi1, chi2, TH_F)


def select(scores):
    """`score = 0; for it ascending: if (currentScore > score) take it` -> (best index or -1, its score or 0)"""
    best, score = -1, F32(0)
    for it, s in enumerate(np.asarray(scores, np.float32)):
        if s > score:
            best, score = it, s
    return best, F32(score)


def tree_sum(terms):
    """a power-of-two tree sum of each row, in float32: what a parallel reduction would compute instead of the chain"""
    t = np.asarray(terms, np.float32)
    n = 1
    while n < t.shape[1]:
        n *= 2
    t = np.concatenate([t, np.zeros((t.shape[0], n - t.shape[1]), np.float32)], axis=1)
    with np.errstate(all="ignore"):
        while t.shape[1] > 1:
            t = (t[:, 0::2] + t[:, 1::2]).astype(np.float32)
    return t[:, 0]


def two_view_score(job):
    """job: dict(xy1 (n1, 2), xy2 (n2, 2), matches12 (n1,), H21, H12 (nH, 9), F21 (nF, 9), sigma) -> dict of results with
    the C ABI's fields and `rc`; over the pair cap or with an entry >= n2 nothing is scored, as in the library"""
    m = np.asarray(job["matches12"], np.int32).reshape(-1)
    n2 = len(np.asarray(job["xy2"]).reshape(-1, 2))
    H21, H12, F21 = _mats(job["H21"]), _mats(job["H12"]), _mats(job["F21"])
    err = bool((m >= n2).any())
    pairs = pair_list(np.where(m >= n2, -1, m))
    n = len(pairs)
    cap = min(len(m), MAX_PAIRS)
    rc = ERR_INVALID if err else ERR_UNSUPPORTED if n > cap else 0
    used = pairs if rc == 0 else pairs[:0]
    pts = gather(job["xy1"], job["xy2"], used)
    sh, ih, _ = check_homographies(H21, H12, pts, job["sigma"])
    sf, jf, _ = check_fundamentals(F21, pts, job["sigma"])
    bh, score_h = select(sh)
    bf, score_f = select(sf)
    zero = np.zeros(len(used), np.uint8)
    return dict(rc=rc, n_pairs=n, pairs=pairs[:cap], best_h=bh, best_f=bf, score_h=score_h, score_f=score_f, scores_h=sh,
                scores_f=sf, inliers_h=ih[bh] if bh >= 0 else zero, inliers_f=jf[bf] if bf >= 0 else zero)
