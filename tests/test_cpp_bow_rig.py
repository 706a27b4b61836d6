"""include/vslam_shim.hpp, the rig forms of FMatcher::SearchByBoW and DBoW3::Vocabulary::transform.  CPU: the demo compiles and
links.  GPU: it computes what the numpy restatement of the reference (tests/bow_rig_ref.py) and the oracle's ComputeBoW compute:
one KeyFrame (TrackReferenceKeyFrame), two KeyFrames in one enqueue (the relocalisation loop), the KeyFrame-KeyFrame overload."""
import json
import os
import subprocess

import numpy as np
import pytest

import bow_rig_ref as BR
import frustum_cases as FC
import vi_slam_amd as V
from oracle import orbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")
VOC = os.path.join(FC.GOLDEN, "voc_k8_L3_quicklz.dbow3")
LEVELSUP = 1


def _build(tmp_path):
    exe = str(tmp_path / "bow_rig_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "bow_rig_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return exe


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, np.int32).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _fv_sum(fv):
    return _fnv(fv["fv_feat"]) ^ _fnv(fv["fv_nodes"]) ^ _fnv(fv["fv_off"])


def test_bow_rig_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def _expected():
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    voc = V.read_vocabulary_file(VOC, library=V.host_lib())
    kk, kd = np.concatenate([p["kL"], p["kR"]]), np.concatenate([p["dL"], p["dR"]])
    fk, fd = np.concatenate([p["kR"], p["kL"]]), np.concatenate([p["dR"], p["dL"]])
    nl, nr = len(p["kL"]), len(p["kR"])
    flags = (np.random.default_rng(4).random(nl + nr) < 0.85).astype(np.uint8)
    kfv, ffv, lfv = (orbo.bow_transform(voc, d, LEVELSUP) for d in (kd, fd, p["dL"]))
    one = BR.search_by_bow_rig(kk, kd, flags, kfv, fk, fd, nr, ffv, 0.7, True)
    left = BR.search_by_bow_rig(p["kL"], p["dL"], flags[:nl], lfv, fk, fd, nr, ffv, 0.7, True)
    kfkf = BR.search_by_bow_keyframes_rig(kk, kd, flags, nl, kfv, p["kL"], p["dL"], flags[:nl], nl, lfv, 0.8, True)
    return dict(p=p, flags=flags, kfv=kfv, ffv=ffv, one=one, left=left, kfkf=kfkf, nl=nl, nr=nr)


def test_the_demo_scene_matches_on_both_sides():
    e = _expected()
    nm, m = e["one"]
    # the frame's left camera holds the KeyFrame's right features exactly; its right slots are reached through the nested branch
    assert nm > 200 and (m[:e["nr"]] >= 0).sum() > 50 and (m[e["nr"]:] >= 0).sum() > 20
    # the left camera alone must first find its stereo partner in the frame's left slots: fewer matches, but not none
    assert e["left"][0] > 30 and not np.array_equal(e["left"][1], m)
    assert e["kfkf"][0] > 100 and (e["kfkf"][1][e["nl"]:] == -1).all()


@pytest.mark.gpu
def test_bow_rig_demo_equals_reference(tmp_path):
    exe = _build(tmp_path)
    e = _expected()
    files = {k: str(tmp_path / (k + ".bin")) for k in ("left", "right", "flags")}
    e["p"]["L"].tofile(files["left"])
    e["p"]["R"].tofile(files["right"])
    e["flags"].tofile(files["flags"])
    r = subprocess.run([exe, str(FC.HUT_W), str(FC.HUT_H), files["left"], files["right"], str(FC.HUT_NF), VOC, str(LEVELSUP),
                        files["flags"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert (got["n_left"], got["n_right"], got["kf_left"], got["kf_right"]) == (e["nr"], e["nl"], e["nl"], e["nr"])
    assert got["f_fv"] == _fv_sum(e["ffv"]) and got["kf_fv"] == _fv_sum(e["kfv"])
    assert got["one"] == [e["one"][0], _fnv(e["one"][1])]
    assert got["all"] == [[e["one"][0], _fnv(e["one"][1])], [e["left"][0], _fnv(e["left"][1])]]
    assert got["kfkf"] == [e["kfkf"][0], _fnv(e["kfkf"][1])]
