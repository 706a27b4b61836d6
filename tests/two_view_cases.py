"""Cases of the two-view consensus: the smallest shapes at which the pair list, the two checks, the serial chain and the
selection can go wrong.  A case is a dict(name, xy1 (n1, 2), xy2 (n2, 2), matches12 (n1,), H21, H12 (nH, 9), F21 (nF, 9),
sigma); every array is float32 / int32 and comes from a seeded generator.  The hypotheses are inputs: a true model,
perturbed -- how a caller computes them (ComputeH21 / ComputeF21) is outside the library.
"""
import functools

import numpy as np

W, H_IMG = 640, 480
K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
MAX_PAIRS = 8192   # VSLAM_TWO_VIEW_MAX_PAIRS
MAX_HYP = 1024     # VSLAM_TWO_VIEW_MAX_HYP
TRUE_AT = 17       # where the unperturbed model sits among the hypotheses of a scene


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


R21 = _rot(0.02, -0.05, 0.03)
T21 = np.array([0.35, 0.04, 0.06])


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def true_models():
    """(H21, F21) in float64, H21[2, 2] = 1 and |F21| = 1: the homography of the plane z = 4 (n = e_z, d = 4), on which a
    planar scene lies entirely and a general one with a share of its points, and the epipolar geometry of the two views"""
    Ki = np.linalg.inv(K)
    Hm = K @ (R21 + np.outer(T21, [0, 0, 1.0]) / 4.0) @ Ki
    Fm = Ki.T @ _skew(T21) @ R21 @ Ki
    return Hm / Hm[2, 2], Fm / np.linalg.norm(Fm)


def scene(n_pairs, planar, seed, n_unmatched1=0, n_extra2=0, noise=0.7, outliers=0.3, plane_share=0.0):
    """-> xy1 (n1, 2), xy2 (n2, 2), matches12 (n1,): n_pairs matches, of which a share `outliers` point at a random place of
    image 2; a planar scene lies on z = 4, a general one at depths 2 .. 9 but for a share `plane_share` of its points, which
    lie on that plane too (a wall in a room); frame 1 has n_unmatched1 keypoints without a match among them (the first and the last keypoint are unmatched
    when there are at least two), frame 2 is in shuffled order with n_extra2 keypoints nobody matches"""
    rng = np.random.default_rng(seed)
    n = n_pairs
    p1 = np.stack([rng.uniform(20, W - 20, n), rng.uniform(20, H_IMG - 20, n)], axis=1)
    z = np.full(n, 4.0) if planar else rng.uniform(2.0, 9.0, n)
    if not planar and plane_share:
        z[rng.random(n) < plane_share] = 4.0
    X = (np.linalg.inv(K) @ np.concatenate([p1, np.ones((n, 1))], axis=1).T) * z
    x2 = K @ (R21 @ X + T21[:, None])
    p2 = (x2[:2] / x2[2]).T
    p1 = p1 + rng.normal(0, noise, p1.shape)
    p2 = p2 + rng.normal(0, noise, p2.shape)
    bad = rng.random(n) < outliers
    p2[bad] = np.stack([rng.uniform(0, W, bad.sum()), rng.uniform(0, H_IMG, bad.sum())], axis=1)
    n1, n2 = n + n_unmatched1, n + n_extra2
    slots = np.ones(n1, bool)  # which keypoints of frame 1 carry a match
    if n_unmatched1:
        free = [0, n1 - 1][:min(2, n_unmatched1)]
        rest = np.setdiff1d(np.arange(n1), free)
        free += list(rng.choice(rest, n_unmatched1 - len(free), replace=False))
        slots[free] = False
    xy1 = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H_IMG, n1)], axis=1)
    xy1[slots] = p1
    order = rng.permutation(n2)  # pair k's second keypoint is keypoint order[k] of frame 2
    xy2 = np.stack([rng.uniform(0, W, n2), rng.uniform(0, H_IMG, n2)], axis=1)
    xy2[order[:n]] = p2
    matches = np.full(n1, -1, np.int32)
    matches[slots] = order[:n]
    return xy1.astype(np.float32), xy2.astype(np.float32), matches


def hypotheses(nH, nF, seed, h_spread=1.0, f_spread=1.0, f_true=True):
    """nH homographies and nF fundamental matrices: the model perturbed (every entry by a relative step of standard
    deviation 2e-3 .. 8e-3, times spread: more than the noise can reward), the unperturbed one at index TRUE_AT where there
    are that many (f_true = False: no unperturbed F).  H12 is the float64 inverse, rounded."""
    rng = np.random.default_rng(seed + 1000)
    Ht, Ft = true_models()

    def family(M, n, spread, keep_true=True):
        out = np.repeat(M[None], n, axis=0)
        out = out * (1.0 + rng.normal(0, 1, out.shape) * rng.uniform(2e-3 * spread, 8e-3 * spread, (n, 1, 1)))
        if n > TRUE_AT and keep_true:
            out[TRUE_AT] = M
        return out
    H21 = family(Ht, nH, h_spread)
    F21 = family(Ft, nF, f_spread, f_true)
    H12 = np.linalg.inv(H21) if nH else H21
    f32 = lambda a: np.ascontiguousarray(a.reshape(-1, 9), np.float32)
    return f32(H21), f32(H12), f32(F21)


def make(name, n_pairs, nH, nF, planar=True, seed=1, sigma=1.0, n_unmatched1=0, n_extra2=0, plane_share=0.0, **hyp):
    xy1, xy2, m = scene(n_pairs, planar, seed, n_unmatched1, n_extra2, plane_share=plane_share)
    H21, H12, F21 = hypotheses(nH, nF, seed, **hyp)
    return dict(name=name, xy1=xy1, xy2=xy2, matches12=m, H21=H21, H12=H12, F21=F21, sigma=np.float32(sigma))


@functools.lru_cache(maxsize=None)
def planar_case():
    """H wins: 300 pairs on a plane, 437 keypoints in frame 1 (no multiple of 64; first and last unmatched), the F
    hypotheses off the epipolar geometry (eight coplanar points do not determine it) but near enough to score chains of
    some hundred terms"""
    return make("planar", 300, 200, 200, planar=True, seed=11, n_unmatched1=137, n_extra2=111, f_spread=10.0, f_true=False)


@functools.lru_cache(maxsize=None)
def general_case():
    """F wins: 301 pairs at depths 2 .. 9, four in ten of them on the plane z = 4, so that the homographies (that plane's,
    perturbed) score a chain of their own"""
    return make("general", 301, 200, 200, planar=False, seed=12, n_unmatched1=90, n_extra2=45, f_spread=3.0, plane_share=0.4)


@functools.lru_cache(maxsize=None)
def size_cases():
    """pair counts around the wave, the compaction chunk and the staging round; hypothesis counts around the 64-lane group"""
    out = [make("N=%d" % n, n, 65, 66, seed=20 + k, n_unmatched1=(0 if n in (0, 64) else 5))
           for k, n in enumerate((0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513))]
    out.append(make("N=0,n1=0", 0, 3, 3, seed=40))
    for k, (nh, nf) in enumerate(((0, 0), (0, 1), (1, 0), (200, 201), (201, 200), (MAX_HYP, MAX_HYP))):
        out.append(make("nH=%d,nF=%d" % (nh, nf), 65, nh, nf, planar=False, seed=50 + k, n_unmatched1=9))
    return out


@functools.lru_cache(maxsize=None)
def cap_cases():
    """exactly the pair cap (scored), and one more (VSLAM_ERR_UNSUPPORTED with the count)"""
    return [make("N=cap", MAX_PAIRS, 65, 2, seed=60, n_unmatched1=70),
            make("N=cap+1", MAX_PAIRS + 1, 2, 2, seed=61, n_unmatched1=70)]


def _with(case, name, **kw):
    c = dict(case)
    c.update(kw)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def special_cases():
    base = make("base", 130, 40, 40, planar=True, seed=70, n_unmatched1=21, n_extra2=3, f_spread=5.0)
    out = []
    # an H whose third row is zero: w = 0 and 1/w = inf.  Hypothesis 3: all of H21 is zero, so the projection is 0 * inf =
    # NaN and chi is NaN in image 2 -- a NaN score, every pair an inlier there.  Hypothesis 5: only the third row of H12 is
    # zero, the projection is +-inf, chi = inf > th: no NaN, every pair an outlier in image 1.
    H21 = base["H21"].copy()
    H21[3] = 0
    H12 = base["H12"].copy()
    H12[5, 6:9] = 0
    out.append(_with(base, "H third row zero", H21=H21, H12=H12))
    F21 = base["F21"].copy()
    F21[2] = 0  # 0/0 in both distances of every pair
    out.append(_with(base, "F all zero", F21=F21))
    # the best hypothesis again at a later index: the earlier one wins
    H21, H12, F21 = base["H21"].copy(), base["H12"].copy(), base["F21"].copy()
    H21[20:], H12[20:], F21[20:] = H21[:20], H12[:20], F21[:20]  # so the best one, whichever it is, is there twice
    out.append(_with(base, "best duplicated later", H21=H21, H12=H12, F21=F21))
    # every pair an outlier under every hypothesis: a shift by 1000 px; lines x = -5000 (the transposed line is 0, 0, c)
    Hs = np.array([[1, 0, 1000, 0, 1, 0, 0, 0, 1], [1, 0, -1000, 0, 1, 0, 0, 0, 1]], np.float32)
    Hi = np.ascontiguousarray(Hs[::-1])
    Fs = np.array([[0, 0, 1, 0, 0, 0, 0, 0, 5000], [0, 0, 1, 0, 0, 0, 0, 0, 7000]], np.float32)
    out.append(_with(base, "all outliers", H21=Hs, H12=Hi, F21=Fs))
    # a*a + b*b subnormal: the epipolar geometry at a scale of 1e-19
    gen = make("gen", 130, 5, 40, planar=False, seed=71, n_unmatched1=21)
    out.append(_with(gen, "F x 1e-19", F21=(gen["F21"].astype(np.float64) * 1e-19).astype(np.float32)))
    out.append(_with(gen, "sigma=2", sigma=np.float32(2.0)))
    return out


@functools.lru_cache(maxsize=None)
def batch_cases():
    """five jobs of different pair and hypothesis counts, for one enqueue"""
    return [make("batch0", 300, 200, 200, planar=True, seed=80, n_unmatched1=37, f_spread=20.0, f_true=False),
            make("batch1", 0, 5, 7, seed=81, n_unmatched1=4),
            make("batch2", 97, 0, 130, planar=False, seed=82, n_unmatched1=1),
            make("batch3", 700, 64, 1, planar=True, seed=83, n_extra2=50),
            make("batch4", 33, 129, 64, planar=False, seed=84, n_unmatched1=300, sigma=1.5)]


def all_scored_cases():
    """every case but the one over the cap"""
    return [planar_case(), general_case()] + size_cases() + special_cases() + batch_cases() + cap_cases()[:1]


def bad_index_case():
    """a matches12 entry == n2: the reference would read past mvKeys2"""
    c = make("entry >= n2", 40, 3, 3, seed=90, n_unmatched1=6)
    m = c["matches12"].copy()
    m[np.nonzero(m >= 0)[0][7]] = len(c["xy2"])
    return _with(c, "entry >= n2", matches12=m)


def kps_of(xy):
    """cv::KeyPoint records around the positions; the other fields hold values a stride mistake would show"""
    import vi_slam_amd as V
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), V.KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = 31.0, 271.5, 1e9, 3, -1
    return k


def job_of(case):
    """the case as FExtractor.two_view_score / two_view_score_host take it, everything on the host"""
    return dict(kps1=kps_of(case["xy1"]), kps2=kps_of(case["xy2"]), matches12=case["matches12"], H21=case["H21"],
                H12=case["H12"], F21=case["F21"], sigma=case["sigma"])


def assert_equal_words(got, want, what):
    """every field of a result against the yardstick's, floats as uint32 words"""
    w32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
    assert got["n_pairs"] == want["n_pairs"], (what, got["n_pairs"], want["n_pairs"])
    assert np.array_equal(got["pairs"], want["pairs"]), what
    for k in ("best_h", "best_f"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("score_h", "score_f", "scores_h", "scores_f"):
        bad = np.nonzero(w32(got[k]) != w32(want[k]))[0]
        assert len(bad) == 0, (what, k, len(bad), bad[:5], np.atleast_1d(got[k])[bad[:5]], np.atleast_1d(want[k])[bad[:5]])
    for k in ("inliers_h", "inliers_f"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), (what, k)


def svd_hypotheses(pts, n, seed):
    """n homographies and n fundamental matrices from seeded 8-point sets of pts (N, 4) by the normalised DLT / 8-point
    algorithm over np.linalg.svd, in float64, rounded: stand-ins for ComputeH21 / ComputeF21.  They are inputs to the
    scoring, so how they were made does not matter to it.  -> H21, H12, F21 (n, 9) float32"""
    rng = np.random.default_rng(seed)
    pts = np.asarray(pts, np.float64)

    def normalise(p):
        m = p.mean(0)
        d = np.abs(p - m).mean(0)
        T = np.array([[1 / d[0], 0, -m[0] / d[0]], [0, 1 / d[1], -m[1] / d[1]], [0, 0, 1]])
        return (p - m) / d, T
    n1, T1 = normalise(pts[:, 0:2])
    n2, T2 = normalise(pts[:, 2:4])
    H21, H12, F21 = [], [], []
    while len(H21) < n:
        idx = rng.choice(len(pts), 8, replace=False)
        A, B = [], []
        for (u1, v1), (u2, v2) in zip(n1[idx], n2[idx]):
            A += [[0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2], [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]]
            B += [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]]
        Hn = np.linalg.svd(np.array(A))[2][8].reshape(3, 3)
        U, w, Vt = np.linalg.svd(np.linalg.svd(np.array(B))[2][8].reshape(3, 3))
        Fn = U @ np.diag([w[0], w[1], 0]) @ Vt
        Hm = np.linalg.inv(T2) @ Hn @ T1
        if abs(np.linalg.det(Hm)) < 1e-12:
            continue
        H21.append(Hm)
        H12.append(np.linalg.inv(Hm))
        F21.append(T2.T @ Fn @ T1)
    f32 = lambda a: np.ascontiguousarray(np.array(a).reshape(-1, 9), np.float32)
    return f32(H21), f32(H12), f32(F21)


REAL_SEED = 7  # of svd_hypotheses in the real-pixel chain: chosen so that a winner with >= 30 inliers exists (asserted there)
