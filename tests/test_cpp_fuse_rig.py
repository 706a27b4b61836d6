"""include/vslam_shim.hpp, FMatcher::FuseSearchRig and FMatcher::FuseWalk: the search half of Fuse(pKF, vpMapPoints, th, bRight) for
both cameras of several rig KeyFrames in one call, and the walk over its results.  CPU: the demo compiles and links.  GPU: it
computes what the numpy restatement of the reference (tests/fuse_rig_ref.py) computes, the walk -- with a Replace that
really changes a descriptor and the one-point searches redone on the host -- ends as the same walk in Python does."""
import json
import os
import subprocess

import numpy as np
import pytest

import frustum_cases as HC
import fuse_rig_cases as FC
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")
N_POINTS = 400


def _build(tmp_path):
    exe = str(tmp_path / "fuse_rig_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "fuse_rig_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
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
    """the scene's first points against all three KeyFrames; the left and the right job of a KeyFrame share its validity bytes"""
    s = FC.cases()["scene"]
    c = FC._first(s, N_POINTS, s["jobs"])
    for k in range(3):
        v = c["jobs"][2 * k]["valid"]
        v = np.ones(N_POINTS, np.uint8) if v is None else v
        c["jobs"][2 * k]["valid"] = c["jobs"][2 * k + 1]["valid"] = v
    return c


def expected_walk(c, bi, bd, stale_rule=True):
    """the demo's walk in Python: every fifth slot of the first KeyFrame holds a resident MapPoint that a fusing candidate
    replaces, which flips every bit of the candidate's descriptor; its later searches are redone with the host twin
    -> (nFused, searches redone, replaces, the log of (job, point, index))"""
    g = FC.golden()
    n = len(c["pts"])
    desc = np.ascontiguousarray(c["desc"], np.uint8).copy()
    host = []
    for j in c["jobs"]:
        k, d = np.ascontiguousarray(j["kps"], V.KP_DTYPE), np.ascontiguousarray(j["desc"], np.uint8)
        host.append((V.fuse_rig_job(*j["pose"], k.ctypes.data, d.ctypes.data, len(k), j["camera"], j["idx_offset"]), k, d))
    rig = V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"])
    in_kf = [set() for _ in range(3)]
    recomputed, replaced, log = set(), set(), []
    fused = redone = 0
    for j, job in enumerate(c["jobs"]):
        for i in range(n):
            if not c["pts"]["valid"][i] or not job["valid"][i] or i in in_kf[j // 2]:
                continue
            idx, dist = int(bi[j, i]), int(bd[j, i])
            if stale_rule and i in recomputed:
                one = V.fuse_search_rig_host(V.kb8_camera(*FC.CAM1), rig, [host[j][0]], c["pts"][i:i + 1], desc[i:i + 1], c["th"],
                                             FC.LSF, FC.IMG, g["sf"], g["is2"])
                idx, dist = int(one[0][0, 0]), int(one[1][0, 0])
                redone += 1
            if idx < 0 or dist > 50:
                continue
            if j // 2 == 0 and idx % 5 == 0 and idx not in replaced:
                replaced.add(idx)
                recomputed.add(i)
                desc[i] ^= np.uint8(0xFF)
            in_kf[j // 2].add(i)
            log.append((j, i, idx))
            fused += 1
    return fused, redone, len(replaced), np.array(log, np.int32).reshape(-1, 3)


def test_fuse_rig_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def test_the_demo_scene_fuses_on_both_sides_and_skips_the_right_job_after_the_left():
    c = demo_case()
    g = FC.golden()
    bi, bd = FC.FR.fuse_search_rig(c["jobs"], c["pts"], c["desc"], g["cams"], c["th"], FC.LSF, g["sf"], g["is2"], FC.BOUNDS)
    fused, redone, replaces, log = expected_walk(c, bi, bd)
    both = ((bi[0] >= 0) & (bd[0] <= 50) & (bi[1] >= 0) & (bd[1] <= 50) & (c["jobs"][0]["valid"] != 0) & (c["pts"]["valid"] != 0)).sum()
    assert fused > 300 and replaces > 20 and redone > 40
    # a survivor's flipped descriptor fuses nowhere later; with the stale batch results it would: the rule changes the result
    wrong = expected_walk(c, bi, bd, stale_rule=False)
    assert wrong[0] > fused and not np.array_equal(wrong[3], log)
    assert ((bi[1::2] >= len(g["kl"])) & (bd[1::2] <= 50)).sum() > 50  # right cameras fuse too
    assert both > 0  # a point the left AND the right job of one KeyFrame would fuse: the walk takes the left one only


@pytest.mark.gpu
def test_fuse_rig_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    c = demo_case()
    g = FC.golden()
    p = np.load(os.path.join(HC.GOLDEN, "pipeline_hut_320x240.npz"))
    files = {k: str(tmp_path / (k + ".bin")) for k in ("left", "right", "cam", "rig", "poses", "pts", "desc", "valid")}
    p["L"].tofile(files["left"])
    p["R"].tofile(files["right"])
    for name, obj in (("cam", V.kb8_camera(*FC.CAM1)), ("rig", V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"]))):
        with open(files[name], "wb") as f:
            f.write(bytes(obj))
    np.concatenate([np.asarray(a, np.float32).reshape(-1) for j in c["jobs"] for a in j["pose"]]).tofile(files["poses"])
    np.ascontiguousarray(c["pts"], V.FUSE_POINT_DTYPE).tofile(files["pts"])
    np.ascontiguousarray(c["desc"], np.uint8).tofile(files["desc"])
    np.concatenate([c["jobs"][2 * k]["valid"] for k in range(3)]).astype(np.uint8).tofile(files["valid"])
    r = subprocess.run([exe, str(HC.HUT_W), str(HC.HUT_H), files["left"], files["right"], str(HC.HUT_NF), files["cam"],
                        files["rig"], files["poses"], "3", files["pts"], files["desc"], str(N_POINTS), files["valid"],
                        repr(float(c["th"])), repr(FC.LSF)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    bi, bd = FC.FR.fuse_search_rig(c["jobs"], c["pts"], c["desc"], g["cams"], c["th"], FC.LSF, g["sf"], g["is2"], FC.BOUNDS)
    fused, redone, replaces, log = expected_walk(c, bi, bd)
    assert got["n_left"] == len(g["kl"]) and got["n_right"] == len(g["kr"])
    assert got["best_idx"] == _fnv(bi.astype(np.int32)) and got["best_dist"] == _fnv(bd.astype(np.int32))
    assert got["fused"] == fused and got["redone"] == redone > 0 and got["replaces"] == replaces > 0
    assert got["log"] == _fnv(log)
