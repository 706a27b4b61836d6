"""Stereo scenes that drive Frame::ComputeStereoMatches down the branches the regular synthetic pairs never take, with
the oracle-side reference and the preconditions that prove a scene does what it is for.  No GPU in here: the CPU
precondition test and the GPU tests import the same builders.

Scene A (320x240).  Upper band (rows 0..99): isolated bright dots on a 13-px lattice, identical in both views.  A dot is
horizontally symmetric, so the SADs left and right of the best shift are equal, deltaR == 0 and -- at octave 0 -- the
disparity is exactly 0: the clamp `disparity <= 0 -> 0.01, bestuR = uL - 0.01` (frame.cpp:963-967) fires.  Lower band:
texture with disparity 12 and +-3 grey levels of noise in the right view, so the accepted SADs are mostly non-zero, the
median is positive and the clamped matches SURVIVE the outlier cut (in a pair of identical images every SAD is 0,
thDist is 0 and the cut erases them all).  With bf / fx = 40 / 12.0, maxD = mbf / (mbf / fx) is about 12: the lower band
sits on the `disparity < maxD` edge and on the minU gate of the candidate search.

Scene B (1241x376): a regular pair with enough right keypoints that some left keypoint's row bucket holds more than 64
of them, the second turn of the candidate loop of k_stereo_best (64 lanes per turn)."""
import numpy as np

from oracle import orbo
from vi_slam_amd import synth

A_W, A_H, A_NF = 320, 240, 500
A_CAMERAS = ((40.0, 400.0), (40.0, 12.0))   # (bf, fx): ordinary, and maxD ~ 12 = the lower band's disparity
A_SEEDS = (1, 2)
A_MIN_CLAMPED = 20

B_W, B_H, B_NF = 1241, 376, 2000
B_BF, B_FX = 386.1448, 718.856


def scene_a(seed):
    big = synth.make_frame(352, 240, seed=seed).copy()
    yy, xx = np.mgrid[0:100, 0:352]
    big[:100] = np.where((xx % 13 == 6) & (yy % 13 == 6), 230, 40).astype(np.uint8)
    L = np.ascontiguousarray(big[:, 16:336])
    R = L.copy()
    noise = np.random.default_rng(seed).integers(-3, 4, (A_H - 100, A_W))
    R[100:] = np.clip(big[100:, 28:348].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return L, R


def scene_c(seed, flat_rows):
    """Left: the ordinary textured frame.  Right: the same view with rows [0, flat_rows) flat, so no right keypoint
    lies there: left keypoints in the upper part read an EMPTY row bucket (vCandidates.empty(), frame.cpp:871), the rest
    match as usual.  flat_rows == height: no right keypoint at all, vDistIdx stays empty and the outlier cut has
    nothing to take a median of (the reference reads vDistIdx[0] of an empty vector there)."""
    L, R = synth.make_stereo_pair(A_W, A_H, seed=seed)
    R = R.copy()
    R[:flat_rows] = 90
    return L, R


def scene_b():
    return synth.make_stereo_pair(B_W, B_H, step=1)


def ordinary_pair():
    """job 0 in front of scene A in a batch"""
    return synth.make_stereo_pair(A_W, A_H, seed=3)


def oracle_stereo(L, R, nf, bf, fx):
    """-> dict: left / right keypoints and descriptors, mvuRight, mvDepth, the accepted SADs (-1: not accepted before the
    cut) of the oracle, and the extractor (for its tables)."""
    eL, eR = orbo.Extractor(nf), orbo.Extractor(nf)
    kL, dL, _ = eL.compute(L)
    kR, dR, _ = eR.compute(R)
    u, dep, bi, bs = orbo.stereo(eL, eR, kL, dL, kR, dR, bf, fx)
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, u=u, depth=dep, sad=bs, ex=eL)


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clamped_survivors(ref, bf):
    """matches that went through the clamp and were not cut: u == float(double(x) - 0.01), depth == bf / 0.01f"""
    want_u = (ref["kL"]["x"].astype(np.float64) - 0.01).astype(np.float32)
    want_z = np.float32(bf) / np.float32(0.01)
    return (words(ref["u"]) == words(want_u)) & (words(ref["depth"]) == words(np.full(len(want_u), want_z, np.float32)))


def median_sad(ref):
    s = np.sort(ref["sad"][ref["sad"] >= 0])
    return int(s[len(s) // 2]) if len(s) else -1


def check_scene_a(ref, bf, fx):
    """the preconditions of scene A on the oracle's result; returns (accepted before the cut, clamped survivors)"""
    surv = clamped_survivors(ref, bf)
    assert int(surv.sum()) >= A_MIN_CLAMPED, "scene A: only %d clamped matches survive the cut" % int(surv.sum())
    assert median_sad(ref) > 0, "scene A: median SAD is 0, the cut erases every match"
    return int((ref["sad"] >= 0).sum()), int(surv.sum())


def check_scene_c(ref, flat_rows):
    """some left keypoints read an empty bucket; unless the right image is flat altogether, others still match.
    Returns (left keypoints with an empty bucket, matches)."""
    cnt = row_bucket_sizes(ref["kR"], ref["ex"].tables()["scale"], A_H)
    empty = cnt[ref["kL"]["y"].astype(np.int64)] == 0
    assert empty.sum() >= 20, "scene C: only %d left keypoints read an empty row bucket" % empty.sum()
    assert np.all(ref["u"][empty] == -1)
    nm = int((ref["u"] >= 0).sum())
    if flat_rows >= A_H:
        assert len(ref["kR"]) == 0 and nm == 0 and len(ref["kL"]) > 100
    else:
        assert nm >= 20, "scene C: only %d matches in the textured part" % nm
    return int(empty.sum()), nm


def row_bucket_sizes(kR, scale, nrows):
    """how many right keypoints each row bucket holds, with the float32 band arithmetic of k_stereo_rows
    (frame.cpp:840-858: rows floor(y - 2 s) .. ceil(y + 2 s), clipped to the image)"""
    r = np.float32(2.0) * scale.astype(np.float32)[kR["octave"]]
    y = kR["y"].astype(np.float32)
    maxr = np.minimum(np.ceil(y + r).astype(np.int64), nrows - 1)
    minr = np.maximum(np.floor(y - r).astype(np.int64), 0)
    cnt = np.zeros(nrows + 1, np.int64)
    np.add.at(cnt, minr, 1)
    np.add.at(cnt, maxr + 1, -1)
    return np.cumsum(cnt)[:nrows]


def check_scene_b(ref):
    """at least one left keypoint reads a row bucket of more than 64 right keypoints; returns the largest bucket read"""
    cnt = row_bucket_sizes(ref["kR"], ref["ex"].tables()["scale"], B_H)
    read = cnt[ref["kL"]["y"].astype(np.int64)]
    assert read.max() > 64, "scene B: largest row bucket a left keypoint reads holds %d right keypoints" % read.max()
    return int(read.max())
