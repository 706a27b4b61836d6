"""include/vslam_shim.hpp, the rig form of FMatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono): the left and the
right branch of the motion-model matcher in one call.  CPU: the demo compiles and links.  GPU: it computes what the numpy
restatement of the reference (tests/frame_projection_rig_ref.py) computes, the direction flags derived by the shim."""
import json
import os
import subprocess

import numpy as np
import pytest

import frame_projection_rig_cases as FP
import frustum_cases as FC
import kb8_cases as KC
import projection_bounds_ref as PB
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")
MB = 0.01  # the rig moved 4 cm along its axis: more than this baseline, so the shim must derive bBackward


def _build(tmp_path):
    exe = str(tmp_path / "frame_rig_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "frame_rig_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
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


def test_frame_rig_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def test_direction_of_the_demo_scene():
    c = FP.cases()["scene_backward"]
    assert PB.projection_direction(c["Tcw"], np.eye(3, 4, dtype=np.float32), MB, False, True) == (False, True)


@pytest.mark.gpu
def test_frame_rig_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    c = FP.cases()["scene_backward"]
    g = FP.golden()
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    files = {k: str(tmp_path / (k + ".bin")) for k in ("left", "right", "cam", "rig", "tcw", "kps", "flags", "x3dw", "desc")}
    p["L"].tofile(files["left"])
    p["R"].tofile(files["right"])
    for name, obj in (("cam", V.kb8_camera(*KC.LOCAL_CAM)),
                      ("rig", V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), g["rig"]["Tlr"], g["rig"]["Trl"]))):
        with open(files[name], "wb") as f:
            f.write(bytes(obj))
    np.ascontiguousarray(c["Tcw"], np.float32).tofile(files["tcw"])
    np.ascontiguousarray(c["last_kps"], V.KP_DTYPE).tofile(files["kps"])
    np.ascontiguousarray(c["flags"], np.uint8).tofile(files["flags"])
    np.ascontiguousarray(c["x3dw"], np.float32).tofile(files["x3dw"])
    np.ascontiguousarray(c["desc"], np.uint8).tofile(files["desc"])
    r = subprocess.run([exe, str(FC.HUT_W), str(FC.HUT_H), files["left"], files["right"], str(FC.HUT_NF), files["cam"],
                        files["rig"], files["tcw"], files["kps"], files["flags"], files["x3dw"], files["desc"],
                        str(len(c["last_kps"])), repr(float(c["th"])), repr(MB)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    nm, m, _ = FP.reference(c)
    assert got["n_left"] == len(c["kl"]) and got["n_right"] == len(c["kr"])
    assert got["nmatches"] == nm >= 100
    assert got["match"] == _fnv(m.astype(np.int32))
