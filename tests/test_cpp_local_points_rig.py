"""include/vslam_shim.hpp, the rig form of FMatcher::SearchLocalPoints: Frame::isInFrustum of both fisheye cameras and both
branches of the local-map matcher in one call.  CPU: the demo compiles and links.  GPU: it computes what the numpy restatements
of the reference (tests/kb8_ref.py, tests/local_points_rig_ref.py) compute."""
import json
import os
import subprocess

import numpy as np
import pytest

import frustum_cases as FC
import kb8_cases as KC
import local_points_rig_cases as LC
import local_points_rig_ref as RR
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "local_points_rig_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "local_points_rig_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
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


def test_local_points_rig_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_local_points_rig_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    s = LC.scene()
    th = 3.0
    P, (tl, tr, _, _, nv), (fl, fr) = LC.scene_records(True)
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    files = {k: str(tmp_path / (k + ".bin")) for k in ("left", "right", "cam", "rig", "params", "points", "desc", "l2r", "r2l")}
    p["L"].tofile(files["left"])
    p["R"].tofile(files["right"])
    for name, obj in (("cam", V.kb8_camera(*KC.LOCAL_CAM)),
                      ("rig", V.kb8_rig(V.kb8_camera(*KC.CAMERAS["strong"]), s["rig"]["Tlr"], s["rig"]["Trl"])),
                      ("params", V.frustum_params(P["Tcw"], P["Ow"], (P["fx"], P["fy"], P["cx"], P["cy"], P["mbf"]),
                                                  P["log_scale_factor"], (P["img_w"], P["img_h"]), P["viewing_cos_limit"],
                                                  P["far_points"], P["th_far_points"]))):
        with open(files[name], "wb") as f:
            f.write(bytes(obj))
    np.ascontiguousarray(s["pts"], V.MAP_POINT_DTYPE).tofile(files["points"])
    np.ascontiguousarray(s["desc"]).tofile(files["desc"])
    s["l2r"].astype(np.int32).tofile(files["l2r"])
    s["r2l"].astype(np.int32).tofile(files["r2l"])
    r = subprocess.run([exe, str(FC.HUT_W), str(FC.HUT_H), files["left"], files["right"], str(FC.HUT_NF), files["cam"],
                        files["rig"], files["params"], files["points"], files["desc"], str(len(s["pts"])), files["l2r"],
                        files["r2l"], repr(th)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    nm, m, _ = RR.search_by_projection_rig(fl, fr, s["desc"], s["kl"], s["dl"], s["kr"], s["dr"], s["l2r"], s["r2l"], s["sf"],
                                           LC.BOUNDS, th, 0.8, None)
    assert got["n_left"] == len(s["kl"]) and got["n_right"] == len(s["kr"])
    assert got["nmatches"] == nm >= 100 and got["n_to_match"] == nv
    assert got["match"] == _fnv(m.astype(np.int32))
    assert got["track_left"] == _fnv(tl) and got["track_right"] == _fnv(tr)
