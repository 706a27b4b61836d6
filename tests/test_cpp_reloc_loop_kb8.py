"""include/vslam_shim.hpp, FMatcher::SearchByProjectionKeyFrameKB8 and FMatcher::FindMatchesByProjectionKB8: the relocalisation
matcher with a fisheye frame, and LoopClosing::FindMatchesByProjection's batch -- one MapPoint list against the covisible
KeyFrames as jobs -- in one call.  CPU: the demo compiles and links.  GPU: it computes what the numpy restatement of the
reference (tests/reloc_loop_kb8_ref.py) computes."""
import json
import os
import subprocess

import numpy as np
import pytest

import frustum_cases as HC
import fuse_rig_cases as FRC
import kb8_ref as KR
import reloc_loop_kb8_cases as RC
import reloc_loop_kb8_ref as RL
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")
TH_A, ORB_DIST = 3.0, 100


def _build(tmp_path):
    exe = str(tmp_path / "reloc_loop_kb8_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "reloc_loop_kb8_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
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


def demo_case():
    """the scene's points against three poses; every KeyFrame holds the keypoints the demo extracts (the golden's left ones), and
    the list doubles as the entries of A's KeyFrame, the last third of them right-camera entries with angles of their own"""
    g = RC.golden()
    s = RC.b_cases()["b_scene"]
    n = len(s["pts"])
    rng = np.random.default_rng(90)
    jobs = [dict(pose=FRC._pose(T), kps=g["kl"], desc=g["dl"], matched=None, valid=(rng.random(n) > 0.1 * k).astype(np.uint8))
            for k, T in enumerate(FRC.scene_poses())]
    keys = np.zeros(n, V.KP_DTYPE)
    keys["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    keys["size"] = 31.0
    return dict(jobs=jobs, pts=s["pts"], desc=s["desc"], th=s["th"], ratio=s["ratio"], keys=keys, nl=2 * n // 3)


def expected(c):
    g = RC.golden()
    cam = KR.camera(*RC.CAM1)
    R, t, Ow = c["jobs"][0]["pose"]
    T = np.hstack([R, t.reshape(3, 1)])
    p = c["pts"]
    a = RL.search_by_projection_keyframe_kb8(T, Ow, cam, TH_A, ORB_DIST, RC.LSF, c["keys"], p["valid"].astype(np.uint8), p["pos"],
                                             p["min_distance"], p["max_distance"], c["desc"], g["kl"], g["dl"], g["sf"], RC.BOUNDS,
                                             True, None, True, c["nl"])
    b = RL.search_by_projection_sim3_kb8(c["jobs"], p, c["desc"], cam, c["th"], c["ratio"], RC.LSF, g["sf"], RC.BOUNDS)
    return a, b


def test_reloc_loop_kb8_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def test_the_demo_case_matches_in_both_forms():
    (nm, m), (mk, nmb, ng) = expected(demo_case())
    assert nm > 20 and (m >= 0).sum() == nm
    assert (nmb > 20).all() and (ng >= nmb).all() and len(mk) == 3


@pytest.mark.gpu
def test_reloc_loop_kb8_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    c = demo_case()
    g = RC.golden()
    p = np.load(os.path.join(HC.GOLDEN, "pipeline_hut_320x240.npz"))
    files = {k: str(tmp_path / (k + ".bin")) for k in ("left", "cam", "poses", "pts", "desc", "valid", "keys")}
    p["L"].tofile(files["left"])
    with open(files["cam"], "wb") as f:
        f.write(bytes(V.kb8_camera(*RC.CAM1)))
    np.concatenate([np.asarray(a, np.float32).reshape(-1) for j in c["jobs"] for a in j["pose"]]).tofile(files["poses"])
    np.ascontiguousarray(c["pts"], V.FUSE_POINT_DTYPE).tofile(files["pts"])
    np.ascontiguousarray(c["desc"], np.uint8).tofile(files["desc"])
    np.concatenate([j["valid"] for j in c["jobs"]]).astype(np.uint8).tofile(files["valid"])
    np.ascontiguousarray(c["keys"], V.KP_DTYPE).tofile(files["keys"])
    r = subprocess.run([exe, str(HC.HUT_W), str(HC.HUT_H), files["left"], str(HC.HUT_NF), files["cam"], files["poses"], "3",
                        files["pts"], files["desc"], str(len(c["pts"])), files["valid"], files["keys"], repr(TH_A), str(ORB_DIST),
                        str(c["th"]), repr(float(c["ratio"])), repr(RC.LSF)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    (nm, m), (mk, nmb, ng) = expected(c)
    assert got["n_kp"] == len(g["kl"])
    assert got["a_nmatches"] == nm and got["a_match"] == _fnv(m.astype(np.int32))
    assert got["b_match"] == _fnv(np.concatenate(mk).astype(np.int32))
    assert got["b_nmatches"] == _fnv(nmb.astype(np.int32)) and got["b_gated"] == _fnv(ng.astype(np.int32))
