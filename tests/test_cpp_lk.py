"""include/vslam_shim.hpp, class FeatureTrackerGPU: vilib::FeatureTrackerGPU's options and methods over the C ABI of
include/vslam_featuretracker.h.  CPU: the demo compiles and links.  GPU: set up as the reference's own tracker test is
(test/src/high_level/test_featuretracker.cpp), it prints the feature lists that tests/lk_ref.py computes."""
import json
import os
import subprocess

import numpy as np
import pytest

import lk_cases as LC
import lk_ref as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "lk_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "lk_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return exe


def test_lk_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_lk_demo_prints_the_restatements_features(tmp_path):
    exe = _build(tmp_path)
    seq = LC.frames()[:3]
    n, h, w = seq.shape
    path = str(tmp_path / "frames.raw")
    np.ascontiguousarray(seq).tofile(path)
    r = subprocess.run([exe, str(w), str(h), str(n), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip().splitlines()
    got = json.loads(out[-1])
    nc, nr = LC.grid(seq[0])
    T = lk.Tracker(lk.Options(**LC.TEST_OPTS), LC.ref_detector("harris"), nc, nr)
    want, counts = [], []
    for k, img in enumerate(seq):
        counts.append(list(T.track(img)))
        f = T.feature_table()
        px, sc = LC.u32(f["px"]), LC.u32(f["score"])
        want += ["F %d %08x %08x %08x %d %d" % (k, px[i, 0], px[i, 1], sc[i], f["level"][i], f["track_id"][i]) for i in range(len(sc))]
    assert out[:-1] == want
    assert got == {"counts": counts, "tracks": len(T.book.tracks),
                   "disparity": "%08x" % LC.u32(np.array([T.book.disparity(0.5)], np.float32))[0]}
    assert counts[0] == [0, 50] and 25 < counts[1][0] < 50
