"""include/vslam_shim.hpp, distorted pinhole camera: FExtractor::SetCamera, UndistortKeyPoints, ComputeImageBounds and
FMatcher::SearchForInitialization over FrameView's float bounds.  CPU: the demo compiles and links.  GPU: it computes
what the ctypes path and the numpy restatement of the reference compute."""
import json
import os
import subprocess

import numpy as np
import pytest

import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "undistort_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "undistort_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_undistort_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_undistort_demo_equals_ctypes_path(tmp_path):
    import vi_slam_amd as V
    from vi_slam_amd import synth
    W, H, NF = 1280, 720, 1000
    K, D = U.EUROC_LIKE
    a, b = synth.make_frame(W, H, step=0), synth.make_frame(W, H, step=1)
    paths = []
    for name, im in (("a", a), ("b", b)):
        p = str(tmp_path / (name + ".raw"))
        im.tofile(p)
        paths.append(p)
    exe = _build(tmp_path)
    args = [exe, str(W), str(H)] + paths + [str(NF)] + [repr(float(np.float32(v))) for v in list(K) + list(D)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])

    f1 = V.FExtractor(NF, 1.2, 8, 20, 7, W, H)
    f2 = V.FExtractor(NF, 1.2, 8, 20, 7, W, H)
    try:
        for f in (f1, f2):
            f.set_camera(*K, dist=D)
        k1, d1, _ = f1.compute(a)
        k2, d2, _ = f2.compute(b)
        u1, u2 = f1.ukeypoints(0), f2.ukeypoints(0)
        bounds = f2.image_bounds()
        nm, m12, pm = V.FMatcher(f2, 0.9, True).SearchForInitialization(
            u1, f1.slot_buffers(0)[1], u2, f2.slot_buffers(0)[1], np.stack([u1["x"], u1["y"]], 1), 100, bounds=bounds)
    finally:
        f1.close()
        f2.close()
    wb = U.image_bounds(K, D, W, H)
    wn, wm, wp = U.search_for_initialization(U.undistort_keypoints(k1, K, D), d1, U.undistort_keypoints(k2, K, D), d2,
                                             wb, window=100, nnratio=0.9)
    assert np.array_equal(bounds, wb) and np.array_equal(np.float32(got["bounds"]), wb)
    assert got["n1"] == len(k1) and got["n2"] == len(k2) and got["kp1"] == _fnv(k1)
    assert got["ukp1"] == _fnv(u1) and got["ukp2"] == _fnv(u2) and got["ukp1"] != got["kp1"]
    assert got["nmatches"] == nm == wn and nm > 20 and np.array_equal(m12, wm) and np.array_equal(pm, wp)
    assert got["m12"] == _fnv(m12) and got["prev"] == _fnv(pm)
