"""CPU: the two-view consensus (MotionEstimator::CheckHomography / CheckFundamental and the selection).  First the numpy
restatement (tests/two_view_ref.py) is pinned from outside -- literals worked by hand, a float64 evaluation, the property
that makes the serial chain matter -- and the cases are shown to go where they claim to go.  Then the shared arithmetic
(vi_slam_amd/csrc/vslam_two_view.h, host build in libvslam_host.so) equals the restatement as uint32 words on every case;
the export table and the Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import two_view_cases as TC
import two_view_ref as TR
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def chain(terms):
    """the reference's `score += term` loop, one float32 add at a time"""
    s = F32(0)
    for t in terms:
        s = F32(s + F32(t))
    return s


def test_hand_worked_two_pairs_under_a_shift():
    """H21 shifts x by 1.  Pair A follows it exactly (chi 0 in both images); pair B is 2 px away, 1 px off: chi = 1 on both
    sides.  The chain is ((5.991 + 5.991) + 4.991) + 4.991 in float32, in that order."""
    H21 = np.array([[1, 0, 1, 0, 1, 0, 0, 0, 1]], F32)
    H12 = np.array([[1, 0, -1, 0, 1, 0, 0, 0, 1]], F32)
    pts = np.array([[10, 20, 11, 20], [30, 40, 32, 40]], F32)
    s, inl, terms = TR.check_homographies(H21, H12, pts, 1.0)
    th = F32(5.991)
    want = [th, th, F32(th - F32(1)), F32(th - F32(1))]
    assert TR.bits(terms[0]).tolist() == TR.bits(np.array(want, F32)).tolist()
    assert TR.bits(s)[0] == TR.bits(chain(want))[0] and inl.tolist() == [[1, 1]]
    # a pure x translation: epipolar lines y2 = y1, the distance is (v1 - v2)^2.  chi = 0 | 4 (> 3.841: out) | 2.25
    Fm = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0]], F32)
    pts = np.array([[10, 20, 11, 20], [30, 40, 32, 42], [1, 1, 5, 2.5]], F32)
    s, inl, terms = TR.check_fundamentals(Fm, pts, 1.0)
    want = [th, th, F32(0), F32(0), F32(th - F32(2.25)), F32(th - F32(2.25))]
    assert TR.bits(terms[0]).tolist() == TR.bits(np.array(want, F32)).tolist()
    assert TR.bits(s)[0] == TR.bits(chain(want))[0] and inl.tolist() == [[1, 0, 1]]
    # sigma = 2 divides chi by 4: the 4 px^2 pair comes back in with chi = 1
    s2, inl2, terms2 = TR.check_fundamentals(Fm, pts, 2.0)
    assert inl2.tolist() == [[1, 1, 1]] and TR.bits(terms2[0, 2])[0] == TR.bits(F32(th - F32(1)))[0]
    assert TR.bits(TR.inv_sigma_square(2.0))[0] == TR.bits(F32(0.25))[0]


def test_identity_on_identical_points_scores_the_chain_of_2n_thresholds():
    rng = np.random.default_rng(5)
    xy = rng.uniform(0, 600, (300, 2)).astype(F32)
    pts = np.concatenate([xy, xy], axis=1)
    I = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1]], F32)
    s, inl, _ = TR.check_homographies(I, I, pts, 1.0)
    assert TR.bits(s)[0] == TR.bits(chain([F32(5.991)] * 600))[0] and inl.all()
    assert s[0] != F32(600 * 5.991)  # the chain is not the product


def _f64_checks(case):
    """both checks in float64 over the same float32 inputs -> (scores, chi1, chi2) per model"""
    pts = TR.gather(case["xy1"], case["xy2"], TR.pair_list(case["matches12"])).astype(np.float64)
    u1, v1, u2, v2 = (pts[:, k][None, :] for k in range(4))
    inv = 1.0 / (float(case["sigma"]) ** 2)
    out = {}

    def proj(M, pu, pv, qu, qv):
        m = [M[:, k:k + 1].astype(np.float64) for k in range(9)]
        w = m[6] * qu + m[7] * qv + m[8]
        return ((pu - (m[0] * qu + m[1] * qv + m[2]) / w) ** 2 + (pv - (m[3] * qu + m[4] * qv + m[5]) / w) ** 2) * inv
    with np.errstate(all="ignore"):
        c1, c2 = proj(case["H12"], u1, v1, u2, v2), proj(case["H21"], u2, v2, u1, v1)
        out["h"] = (np.where(c1 > 5.991, 0, 5.991 - c1).sum(1) + np.where(c2 > 5.991, 0, 5.991 - c2).sum(1), c1, c2, 5.991)
        f = [case["F21"][:, k:k + 1].astype(np.float64) for k in range(9)]
        a2, b2, c2_ = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        a1, b1, c1_ = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        d1 = (a2 * u2 + b2 * v2 + c2_) ** 2 / (a2 * a2 + b2 * b2) * inv
        d2 = (a1 * u1 + b1 * v1 + c1_) ** 2 / (a1 * a1 + b1 * b1) * inv
        out["f"] = (np.where(d1 > 3.841, 0, 5.991 - d1).sum(1) + np.where(d2 > 3.841, 0, 5.991 - d2).sum(1), d1, d2, 3.841)
    return out


@pytest.mark.parametrize("which", ["planar", "general"])
def test_a_float64_evaluation_agrees(which):
    """On every hypothesis of both models of both scenes: the flags wherever chi is further than 1e-3 relative from its
    threshold, and the score within 1e-5 relative (a float64 score of zero must be zero).  The cases are made so that the
    yardstick can meet this: every family scores chains of many terms -- the F family of the planar scene is off the
    epipolar geometry but not far, the general scene has a plane for its H family."""
    case = TC.planar_case() if which == "planar" else TC.general_case()
    want = TR.two_view_score(case)
    pts = TR.gather(case["xy1"], case["xy2"], want["pairs"])
    f64 = _f64_checks(case)
    for model, (s32, in32, _) in (("h", TR.check_homographies(case["H21"], case["H12"], pts, case["sigma"])),
                                  ("f", TR.check_fundamentals(case["F21"], pts, case["sigma"]))):
        s64, c1, c2, th = f64[model]
        clear = (np.abs(c1 - th) > 1e-3 * th) & (np.abs(c2 - th) > 1e-3 * th)
        in64 = (c1 <= th) & (c2 <= th)
        assert clear.mean() > 0.99 and np.array_equal(in32.astype(bool)[clear], in64[clear]), model
        rel = np.abs(s32.astype(np.float64) - s64) / np.maximum(np.abs(s64), 1e-30)
        print(which, model, "largest relative score difference to float64: %.3g; median score %.0f" % (rel.max(), np.median(s64)))
        assert len(s64) == 200 and np.median(s64) > 100 and s64.max() > 500, (model, np.median(s64))  # chains, not a few terms
        assert (rel <= 1e-5).all(), (model, rel.max(), int(rel.argmax()))


def test_the_unperturbed_model_scores_highest_and_the_right_model_wins():
    p, g = TR.two_view_score(TC.planar_case()), TR.two_view_score(TC.general_case())
    assert p["n_pairs"] == 300 and len(TC.planar_case()["matches12"]) % 64 != 0
    assert TC.planar_case()["matches12"][0] == -1 and TC.planar_case()["matches12"][-1] == -1
    assert p["best_h"] == TC.TRUE_AT and g["best_f"] == TC.TRUE_AT
    rh = p["score_h"] / (p["score_h"] + p["score_f"])
    assert rh > 0.5 and p["inliers_h"].sum() >= 150, rh  # Reconstruct goes to ReconstructH
    assert g["score_h"] + g["score_f"] > 0 and g["score_h"] / (g["score_h"] + g["score_f"]) <= 0.5
    assert g["inliers_f"].sum() >= 150


def test_a_tree_sum_changes_most_scores():
    """what pins the design: a parallel reduction of the same terms is another number for most hypotheses"""
    shares = []
    for case, model in ((TC.planar_case(), "h"), (TC.general_case(), "f")):
        pts = TR.gather(case["xy1"], case["xy2"], TR.pair_list(case["matches12"]))
        s, _, terms = (TR.check_homographies(case["H21"], case["H12"], pts, 1.0) if model == "h"
                       else TR.check_fundamentals(case["F21"], pts, 1.0))
        shares.append(float((TR.bits(TR.tree_sum(terms)) != TR.bits(s)).mean()))
        print(case["name"], model, "share of scores a power-of-two tree sum changes: %.3f" % shares[-1])
    assert min(shares) >= 0.5, shares


def test_the_special_cases_go_where_they_say():
    sp = {c["name"]: c for c in TC.special_cases()}
    r = TR.two_view_score(sp["H third row zero"])
    s = r["scores_h"]
    assert np.isnan(s[3]) and TR.bits(s[3:4])[0] == 0x7FC00000 and r["best_h"] not in (3, 5) and r["best_h"] >= 0
    pts = TR.gather(sp["H third row zero"]["xy1"], sp["H third row zero"]["xy2"], r["pairs"])
    _, inl, terms = TR.check_homographies(sp["H third row zero"]["H21"], sp["H third row zero"]["H12"], pts, 1.0)
    assert np.isnan(terms[3, 1::2]).all() and (inl[3] == (terms[3, 0::2] > 0)).all() and inl[3].any()  # NaN side: inlier
    assert not np.isnan(s[5]) and not inl[5].any() and (terms[5, 0::2] == 0).all()                      # inf side: outlier
    r = TR.two_view_score(sp["F all zero"])
    assert np.isnan(r["scores_f"][2]) and r["best_f"] not in (-1, 2)
    r = TR.two_view_score(sp["best duplicated later"])
    for best, sc in ((r["best_h"], r["scores_h"]), (r["best_f"], r["scores_f"])):
        assert 0 <= best < 20 and TR.bits(sc[best:best + 1])[0] == TR.bits(sc[best + 20:best + 21])[0]
    r = TR.two_view_score(sp["all outliers"])
    assert r["n_pairs"] == 130 and (r["best_h"], r["best_f"]) == (-1, -1) and r["score_h"] == 0 and r["score_f"] == 0
    assert (r["scores_h"] == 0).all() and (r["scores_f"] == 0).all()
    assert len(r["inliers_h"]) == 130 and not r["inliers_h"].any() and not r["inliers_f"].any()
    c = sp["F x 1e-19"]
    r = TR.two_view_score(c)
    pts = TR.gather(c["xy1"], c["xy2"], r["pairs"])
    f = [c["F21"][:, k:k + 1] for k in range(9)]
    a2 = (f[0] * pts[None, :, 0] + f[1] * pts[None, :, 1]) + f[2]
    b2 = (f[3] * pts[None, :, 0] + f[4] * pts[None, :, 1]) + f[5]
    den = a2 * a2 + b2 * b2
    tiny = np.finfo(np.float32).tiny
    assert ((den > 0) & (den < tiny)).mean() > 0.9 and r["best_f"] >= 0 and r["inliers_f"].sum() >= 60
    a, b = TR.two_view_score(sp["sigma=2"]), TR.two_view_score(TC._with(sp["sigma=2"], "sigma=1", sigma=F32(1)))
    assert a["inliers_f"].sum() > b["inliers_f"].sum() and a["score_f"] != b["score_f"]
    # the batch has five different shapes; the size cases cover the empty list and every hypothesis count of the issue
    assert len({(TR.two_view_score(c)["n_pairs"], len(c["H21"]), len(c["F21"])) for c in TC.batch_cases()}) == 5
    sizes = [TR.two_view_score(c)["n_pairs"] for c in TC.size_cases()]
    assert {0, 1, 63, 64, 65, 255, 256, 257}.issubset(sizes)
    assert {0, 1, 200, 201, TC.MAX_HYP}.issubset({len(c["H21"]) for c in TC.size_cases()} & {len(c["F21"]) for c in TC.size_cases()})
    assert TC.MAX_PAIRS == TR.MAX_PAIRS == V.TWO_VIEW_MAX_PAIRS and TC.MAX_HYP == V.TWO_VIEW_MAX_HYP


@pytest.fixture(scope="module")
def wants():
    return {c["name"]: TR.two_view_score(c) for c in TC.all_scored_cases()}


@pytest.mark.parametrize("name", [c["name"] for c in TC.all_scored_cases()])
def test_host_build_equals_the_restatement(wants, name):
    case = next(c for c in TC.all_scored_cases() if c["name"] == name)
    rc, got = V.two_view_score_host(TC.job_of(case))
    assert rc == V.VSLAM_OK and wants[name]["rc"] == 0
    TC.assert_equal_words(got, wants[name], name)


def test_host_build_limits():
    over = TC.cap_cases()[1]
    want = TR.two_view_score(over)
    rc, got = V.two_view_score_host(TC.job_of(over))
    assert rc == V.ERR_UNSUPPORTED == want["rc"] and got["n_pairs"] == TC.MAX_PAIRS + 1 == want["n_pairs"]
    assert (got["best_h"], got["best_f"], got["score_h"], got["score_f"]) == (-1, -1, 0, 0)
    bad = TC.bad_index_case()
    rc, got = V.two_view_score_host(TC.job_of(bad))
    assert rc == V.ERR_INVALID == TR.two_view_score(bad)["rc"] and (got["best_h"], got["best_f"]) == (-1, -1)
    ok = TC.size_cases()[2]
    for sigma in (0.0, float("nan"), float("inf")):
        assert V.two_view_score_host(dict(TC.job_of(ok), sigma=sigma))[0] == V.ERR_INVALID
    too_many = np.tile(ok["F21"][:1], (TC.MAX_HYP + 1, 1))
    assert V.two_view_score_host(dict(TC.job_of(ok), F21=too_many))[0] == V.ERR_INVALID


NEW_SYMBOLS = ["vslam_two_view_score_async", "vslam_two_view_score_wait", "vslam_two_view_score",
               "vslam_fe_get_two_view_profile"]


def test_exports_and_python_mirror():
    assert os.path.exists(V.LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(V.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in V.ABI_SYMBOLS, name
    assert hasattr(C.CDLL(V.HOST_LIB_PATH), "vslamh_two_view_score")
    src = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    for struct, mirror, size in (("vslam_two_view_job", V._TwoViewJob, 80), ("vslam_two_view_result", V._TwoViewResult, 64)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = re.sub(r"^\s*(const\s+)?\w+\s*\*?\s*", "", decl.strip())
            names += [re.sub(r"[\s*]", "", item) for item in decl.split(",") if item.strip()]
        assert names == [f[0] for f in mirror._fields_], struct
        assert C.sizeof(mirror) == size
    for macro, value in (("JOBS", V.TWO_VIEW_MAX_JOBS), ("HYP", V.TWO_VIEW_MAX_HYP), ("PAIRS", V.TWO_VIEW_MAX_PAIRS)):
        assert int(re.search(r"#define VSLAM_TWO_VIEW_MAX_%s (\d+)" % macro, src).group(1)) == value
