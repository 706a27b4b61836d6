"""include/vslam_shim.hpp, MotionEstimator: CheckHomography / CheckFundamental of every hypothesis and the selection in one
call.  CPU: the demo compiles and links without warnings.  GPU: behind extraction and SearchForInitialization of two real
frames it computes what the numpy restatement of the reference computes."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import orbo
import two_view_cases as TC
import two_view_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "two_view_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "two_view_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return exe


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_two_view_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_two_view_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_images.npz"))
    nf, window, nhyp = 5000, 100, 200
    e = orbo.Extractor(nf)
    k1, d1, _ = e.compute(z["hut1"], lap=(0, 1000))
    k2, d2, _ = e.compute(z["hut2"], lap=(0, 1000))
    h, w = z["hut1"].shape
    nm, m12, _ = orbo.search_for_initialization(k1, d1, k2, d2, w, h, window=window)
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    H21, H12, F21 = TC.svd_hypotheses(TR.gather(xy1, xy2, TR.pair_list(m12)), nhyp, TC.REAL_SEED)
    want = TR.two_view_score(dict(xy1=xy1, xy2=xy2, matches12=m12, H21=H21, H12=H12, F21=F21, sigma=1.0))
    assert want["best_h"] >= 0 and want["best_f"] >= 0 and want["inliers_f"].sum() >= 30
    files = {k: str(tmp_path / (k + ".bin")) for k in ("img1", "img2", "hyp")}
    z["hut1"].tofile(files["img1"])
    z["hut2"].tofile(files["img2"])
    np.concatenate([H21.ravel(), H12.ravel(), F21.ravel()]).astype(np.float32).tofile(files["hyp"])
    r = subprocess.run([exe, str(w), str(h), files["img1"], files["img2"], str(nf), str(window), files["hyp"], str(nhyp),
                        str(nhyp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["nmatches"] == nm == got["n_pairs"] == want["n_pairs"] and got["single_model_calls_agree"]
    assert (got["best_h"], got["best_f"]) == (want["best_h"], want["best_f"])
    assert got["score_h"] == int(TR.bits(want["score_h"])[0]) and got["score_f"] == int(TR.bits(want["score_f"])[0])
    for k in ("pairs", "scores_h", "scores_f", "inliers_h", "inliers_f"):
        assert got[k] == _fnv(want[k]), k
