"""GPU: vslam_two_view_score (k_tv_pairs, k_tv_score, k_tv_select) against the numpy restatement (tests/two_view_ref.py)
as uint32 words -- SH, SF, every hypothesis' score, the pair list, the winners and their masks -- on the cases of
tests/two_view_cases.py; host and device placement of the inputs; batches; staging reuse; the limits; and the chain on real
pixels behind extraction and SearchForInitialization."""
import os

import numpy as np
import pytest

import two_view_cases as TC
import two_view_ref as TR
import vi_slam_amd as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fe():
    f = V.FExtractor(5000, 1.2, 8, 20, 7, 752, 480, max_batch=2)
    yield f
    f.close()


@pytest.fixture(scope="module")
def wants():
    """the yardstick's results, computed once"""
    return {c["name"]: TR.two_view_score(c) for c in TC.all_scored_cases()}


def _case(name):
    return next(c for c in TC.all_scored_cases() if c["name"] == name)


@pytest.mark.parametrize("name", [c["name"] for c in TC.all_scored_cases()])
def test_device_equals_the_restatement(fe, wants, name):
    got, = fe.two_view_score([TC.job_of(_case(name))])
    TC.assert_equal_words(got, wants[name], name)


def test_batches_in_one_enqueue(fe, wants):
    for cases in (TC.batch_cases(), TC.size_cases() + TC.special_cases(), [TC.planar_case()] * V.TWO_VIEW_MAX_JOBS):
        assert len(cases) <= V.TWO_VIEW_MAX_JOBS
        got = fe.two_view_score([TC.job_of(c) for c in cases])
        assert len(got) == len(cases)
        for g, c in zip(got, cases):
            TC.assert_equal_words(g, wants[c["name"]], c["name"])


class _Dev:
    """host arrays copied to HBM through torch, kept alive"""

    def __init__(self):
        self.keep = []

    def __call__(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr()


def test_host_and_device_placement_agree(fe, wants):
    import torch
    dev = _Dev()
    for c in (TC.planar_case(), TC.general_case(), TC.size_cases()[0], TC.size_cases()[5]):
        host = TC.job_of(c)
        n1, n2 = len(host["kps1"]), len(host["kps2"])
        k1, k2, m = dev(host["kps1"]) if n1 else 0, dev(host["kps2"]) if n2 else 0, dev(host["matches12"]) if n1 else 0
        torch.cuda.synchronize()
        both = dict(host, kps1=k1, kps2=k2, n1=n1, n2=n2, matches12=m)
        kps_only = dict(host, kps1=k1, kps2=k2, n1=n1, n2=n2)
        matches_only = dict(host, matches12=m)
        for job in (both, kps_only, matches_only):
            if n1 == 0 and job is not host:
                continue  # no arrays to place
            got, = fe.two_view_score([job])
            TC.assert_equal_words(got, wants[c["name"]], c["name"])
        got = fe.two_view_score([host, both, kps_only] if n1 else [host])
        for g in got:
            TC.assert_equal_words(g, wants[c["name"]], c["name"])


def test_small_large_small_reuses_the_staging(fe, wants):
    small, large = TC.size_cases()[3], TC.cap_cases()[0]
    for c in (small, large, small, TC.planar_case()):
        got, = fe.two_view_score([TC.job_of(c)])
        TC.assert_equal_words(got, wants[c["name"]], c["name"])


def test_limits(fe, wants):
    over, bad, ok = TC.cap_cases()[1], TC.bad_index_case(), TC.planar_case()
    with pytest.raises(V.VslamError) as e:
        fe.two_view_score([TC.job_of(ok), TC.job_of(over)])
    assert e.value.code == V.ERR_UNSUPPORTED
    r = e.value.results
    assert r[1]["n_pairs"] == TC.MAX_PAIRS + 1 and (r[1]["best_h"], r[1]["best_f"], r[1]["score_h"], r[1]["score_f"]) == (-1, -1, 0, 0)
    TC.assert_equal_words(r[0], wants[ok["name"]], "beside a job over the cap")
    with pytest.raises(V.VslamError) as e:
        fe.two_view_score([TC.job_of(bad), TC.job_of(ok)])
    assert e.value.code == V.ERR_INVALID and (e.value.results[0]["best_h"], e.value.results[0]["best_f"]) == (-1, -1)
    TC.assert_equal_words(e.value.results[1], wants[ok["name"]], "beside a job with a bad entry")
    for jobs in ([dict(TC.job_of(ok), sigma=0.0)], [dict(TC.job_of(ok), sigma=float("nan"))],
                 [TC.job_of(TC.size_cases()[0])] * (V.TWO_VIEW_MAX_JOBS + 1), [],
                 [dict(TC.job_of(ok), F21=np.tile(ok["F21"][:1], (V.TWO_VIEW_MAX_HYP + 1, 1)))]):
        with pytest.raises(V.VslamError) as e:
            fe.two_view_score(jobs)
        assert e.value.code == V.ERR_INVALID
    # one enqueue at a time; the first one is still delivered
    fe.two_view_score_async([TC.job_of(ok)])
    with pytest.raises(V.VslamError) as e:
        fe.two_view_score_async([TC.job_of(ok)])
    assert e.value.code == V.ERR_INVALID
    TC.assert_equal_words(fe.two_view_score_wait()[0], wants[ok["name"]], "after a refused second enqueue")
    assert V.lib().vslam_two_view_score_wait(fe._h, (V._TwoViewResult * 1)()) == V.ERR_INVALID  # nothing enqueued
    for _ in range(2):  # and through the mirror: a wait without an enqueue, a second wait
        with pytest.raises(V.VslamError) as e:
            fe.two_view_score_wait()
        assert e.value.code == V.ERR_INVALID


def test_profile_counts_the_three_kernels(fe):
    fe.set_profiling(True)
    try:
        before = fe.get_two_view_profile()
        fe.two_view_score([TC.job_of(TC.planar_case())])
        after = fe.get_two_view_profile()
    finally:
        fe.set_profiling(False)
    assert after[3] == before[3] + 1 and all(a > b for a, b in zip(after[:3], before[:3]))
    print("\nk_tv_pairs %.3f ms, k_tv_score %.3f ms, k_tv_select %.3f ms (300 pairs, 200 + 200 hypotheses, one job)"
          % tuple(a - b for a, b in zip(after[:3], before[:3])))


def test_the_chain_on_real_pixels(fe):
    """hut_stereo 01 / 02 through extraction and SearchForInitialization; the keypoints are read where the extraction left
    them in HBM, the matches are the matcher's; hypotheses from seeded 8-point sets"""
    z = np.load(os.path.join(HERE, "golden", "real_images.npz"))
    (k1, _, _), (k2, _, _) = fe.compute_batch([z["hut1"], z["hut2"]], (0, 1000))
    p, c = fe.slot_dev_ptrs(0), fe.slot_dev_ptrs(1)
    m = V.FMatcher(fe, 0.9, True)
    m.search_init_dev_async([(p[0], p[1], p[2], c[0], c[1], c[2], 0)], 100)
    (nm, m12), = [o[:2] for o in m.search_init_dev_wait([len(k1)])]
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    pts = TR.gather(xy1, xy2, TR.pair_list(m12))
    assert len(pts) == nm > 100
    H21, H12, F21 = TC.svd_hypotheses(pts, 200, TC.REAL_SEED)
    want = TR.two_view_score(dict(xy1=xy1, xy2=xy2, matches12=m12, H21=H21, H12=H12, F21=F21, sigma=1.0))
    assert want["best_h"] >= 0 and want["best_f"] >= 0
    assert max(want["inliers_h"].sum(), want["inliers_f"].sum()) >= 30 and min(want["inliers_h"].sum(), want["inliers_f"].sum()) >= 30
    got, = fe.two_view_score([dict(kps1=p[0], kps2=c[0], n1=len(k1), n2=len(k2), matches12=m12, H21=H21, H12=H12, F21=F21)])
    TC.assert_equal_words(got, want, "hut1 -> hut2")
    rh = got["score_h"] / (got["score_h"] + got["score_f"])
    print("\nhut1 -> hut2: %d pairs, SH %.1f (%d inliers), SF %.1f (%d inliers), RH %.3f"
          % (got["n_pairs"], got["score_h"], got["inliers_h"].sum(), got["score_f"], got["inliers_f"].sum(), rh))
