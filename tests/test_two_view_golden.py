"""tests/golden/two_view_hut.npz (generator: tests/golden/make_two_view_golden.py): inputs and yardstick outputs of the
two-view consensus on real pixels, as regression pins.  CPU: the yardstick and the host build reproduce the stored
outputs.  GPU: so does the device."""
import os

import numpy as np
import pytest

import two_view_cases as TC
import two_view_ref as TR
import vi_slam_amd as V

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("n_pairs", "pairs", "best_h", "best_f", "score_h", "score_f", "scores_h", "scores_f", "inliers_h", "inliers_f")


@pytest.fixture(scope="module")
def hut():
    z = np.load(os.path.join(HERE, "golden", "two_view_hut.npz"))
    case = {k: z[k] for k in ("xy1", "xy2", "matches12", "H21", "H12", "F21", "sigma")}
    want = {k: z["want_" + k] for k in FIELDS}
    for k in ("n_pairs", "best_h", "best_f"):
        want[k] = int(want[k])
    return case, want


def test_fixture_is_small_and_has_a_winner(hut):
    case, want = hut
    assert os.path.getsize(os.path.join(HERE, "golden", "two_view_hut.npz")) < 200 * 1024
    assert want["n_pairs"] > 100 and want["best_h"] >= 0 and want["best_f"] >= 0
    assert min(want["inliers_h"].sum(), want["inliers_f"].sum()) >= 30


def test_yardstick_and_host_build_reproduce_the_fixture(hut):
    case, want = hut
    TC.assert_equal_words(TR.two_view_score(case), want, "yardstick")
    rc, got = V.two_view_score_host(TC.job_of(case))
    assert rc == V.VSLAM_OK
    TC.assert_equal_words(got, want, "host build")


@pytest.mark.gpu
def test_device_reproduces_the_fixture(hut):
    case, want = hut
    fe = V.FExtractor(1000, 1.2, 8, 20, 7, 640, 480, max_batch=1)
    try:
        TC.assert_equal_words(fe.two_view_score([TC.job_of(case)])[0], want, "device")
    finally:
        fe.close()
