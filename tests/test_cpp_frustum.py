"""include/vslam_shim.hpp, FMatcher::SearchLocalPoints: Frame::isInFrustum and the local-map matcher in one call.  CPU: the
demo compiles and links.  GPU: it computes what the numpy restatement of the reference and the oracle compute."""
import json
import os
import subprocess

import numpy as np
import pytest

import frustum_cases as FC
import frustum_ref as FR
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "frustum_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "frustum_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
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


def test_frustum_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_frustum_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    s = FC.hut_scene()
    far, th = True, 3.0
    kw = FC.hut_params(far)
    files = {k: str(tmp_path / (k + ".bin")) for k in ("img", "params", "points", "desc")}
    s["C"].tofile(files["img"])
    with open(files["params"], "wb") as f:
        f.write(bytes(V.frustum_params(**kw)))
    np.ascontiguousarray(s["pts"], V.MAP_POINT_DTYPE).tofile(files["points"])
    np.ascontiguousarray(s["desc"]).tofile(files["desc"])
    r = subprocess.run([exe, str(FC.HUT_W), str(FC.HUT_H), files["img"], str(FC.HUT_NF), files["params"], files["points"],
                        files["desc"], str(len(s["pts"])), repr(th)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    nm, m, ntm, kept, track = FR.search_local_points_ref(FR.params(**kw), s["pts"], s["desc"], s["kC"], s["dC"], None, s["sf"],
                                                         th, 0.8, None)
    assert got["n_cur"] == len(s["kC"]) and got["nmatches"] == nm >= 30 and got["n_to_match"] == ntm
    assert got["match"] == _fnv(m.astype(np.int32)) and got["track"] == _fnv(track)
