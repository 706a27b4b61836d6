"""SearchByBoW(KeyFrame, Frame) of a two-fisheye rig (fmatcher.cpp:546-748, F.Nleft != -1), the CPU part:
1. pin: with n_right == 0 the numpy restatement (tests/bow_rig_ref.py) equals the oracle's pinhole function on the sparse scene
   of bow_sparse_cases.py and on the realistic frame; the KeyFrame-KeyFrame rig restatement equals the oracle's with the right
   flags cleared;
2. conditions: across the realistic runs every census entry is taken at least 3 times in some run, every hand-made case takes the
   entries it names, every switch changes the result of at least one case, and a node of the realistic scene at levelsup 2 holds
   more than 64 frame features;
3. twin: the host twin (vslamh_search_by_bow_rig, libvslam_host.so) equals the restatement on every case, the overflow case and
   the batch's jobs included; the stand-alone check program reads the exported cases and agrees;
4. transform_rig's host half (concatenate + one assemble) equals the oracle's transform of the concatenated descriptors;
5. the ABI: header, Python mirror and shim name the new entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bow_rig_cases as BC
import bow_rig_ref as BR
import bow_sparse_cases as SC
import vi_slam_amd as V
from oracle import orbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vslam_search_by_bow_rig_async", "vslam_search_by_bow_rig_wait", "vslam_search_by_bow_rig",
               "vslam_search_by_bow_keyframes_rig", "vslam_fe_get_bow_rig_profile"]


def _twin(c):
    return V.search_by_bow_rig_host(c["kf"]["kps"], c["kf"]["desc"], c["kf"]["n_left"], c["kf"]["flags"], c["kf"]["fv"],
                                    c["f"]["kps"], c["f"]["desc"], c["f"]["n_left"], c["f"]["fv"], c["ratio"], c["ori"])


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ---- 1. pin to the oracle
@pytest.fixture(scope="module")
def sparse():
    feats = SC.oracle_features(SC.frames())
    voc = SC.vocabulary()
    return feats, {lu: SC.oracle_fvs(voc, feats, lu) for lu in SC.LEVELSUP}, SC.flags(len(feats[0][0]), len(feats[1][0]))


@pytest.mark.parametrize("levelsup", SC.LEVELSUP)
@pytest.mark.parametrize("a,b", [(0, 1), (1, 0)])
def test_without_a_right_side_it_is_the_pinhole_function_sparse(sparse, levelsup, a, b):
    feats, fvs, fl = sparse
    (ka, da), (kb, db) = feats[a], feats[b]
    matched = 0
    for ratio in (0.7, 0.9):
        for ori in (True, False):
            want = orbo.search_by_bow(ka, da, fl[a], fvs[levelsup][a], kb, db, fvs[levelsup][b], ratio, ori)
            got = BR.search_by_bow_rig(ka, da, fl[a], fvs[levelsup][a], kb, db, len(kb), fvs[levelsup][b], ratio, ori)
            assert _same(got, want), (ratio, ori)
            twin = V.search_by_bow_rig_host(ka, da, len(ka), fl[a], fvs[levelsup][a], kb, db, len(kb), fvs[levelsup][b], ratio, ori)
            assert _same(twin, want), (ratio, ori)
            matched += want[0]
    assert matched > 0


@pytest.mark.parametrize("levelsup", BC.LEVELSUP)
def test_without_a_right_side_it_is_the_pinhole_function_realistic(levelsup):
    """the realistic frame and KeyFrame read as pinhole ones: every feature is a left feature"""
    kf, f = BC.keyframe(), BC.frame()
    kfv, ffv = BC.fv_of(kf["desc"], levelsup), BC.fv_of(f["desc"], levelsup)
    for ratio in BC.RATIOS:
        for ori in (True, False):
            want = orbo.search_by_bow(kf["kps"], kf["desc"], kf["flags"], kfv, f["kps"], f["desc"], ffv, ratio, ori)
            got = BR.search_by_bow_rig(kf["kps"], kf["desc"], kf["flags"], kfv, f["kps"], f["desc"], len(f["kps"]), ffv, ratio, ori)
            assert _same(got, want) and want[0] > 100, (ratio, ori)


@pytest.mark.parametrize("levelsup", (0, 2))
def test_keyframe_keyframe_rig_is_the_oracle_with_right_flags_cleared(levelsup):
    kf = BC.keyframe()
    nl = kf["n_left"]
    sub = np.concatenate([np.arange(100, 400), nl + np.arange(50, 300)])  # another rig KeyFrame: 300 left + 250 right features
    k2 = dict(kps=kf["kps"][sub], desc=np.ascontiguousarray(kf["desc"][sub]), n_left=300)
    k2["desc"][::3, 5] ^= 0x5A
    f1 = kf["flags"]
    f2 = (np.random.default_rng(8).random(len(sub)) < 0.9).astype(np.uint8)
    fv1, fv2 = BC.fv_of(kf["desc"], levelsup), BC.fv_of(k2["desc"], levelsup)
    c1, c2 = f1.copy(), f2.copy()
    c1[nl:] = 0
    c2[300:] = 0
    assert f1[nl:].any() and f2[300:].any()
    for ratio, ori in ((0.8, True), (0.6, False)):
        want = orbo.search_by_bow_keyframes(kf["kps"], kf["desc"], c1, fv1, k2["kps"], k2["desc"], c2, fv2, ratio, ori)
        got = BR.search_by_bow_keyframes_rig(kf["kps"], kf["desc"], f1, nl, fv1, k2["kps"], k2["desc"], f2, 300, fv2, ratio, ori)
        assert _same(got, want) and want[0] > 30
        assert (want[1][nl:] == -1).all() and (want[1][want[1] >= 0] < 300).all()
        full = orbo.search_by_bow_keyframes(kf["kps"], kf["desc"], f1, fv1, k2["kps"], k2["desc"], f2, fv2, ratio, ori)
        assert not _same(full, want)  # the right features matter: the rig reading is not the pinhole one


# ---- 2. conditions
@pytest.fixture(scope="module")
def censuses():
    out = {}
    for name, c in BC.cases().items():
        cs = BR.new_census()
        r = BC.reference(c, census=cs)
        assert _same(r, BC.reference(c)), name
        out[name] = cs
    return out


def test_every_census_entry_is_taken_three_times_in_a_realistic_run(censuses):
    for entry in BR.CENSUS:
        best = max(censuses[name][entry] for name in BC.realistic())
        assert best >= 3, (entry, best)


def test_hand_made_cases_take_what_they_name(censuses):
    named = set()
    for name, c in BC.hand_made().items():
        n = len(c["kf"]["kps"]) + len(c["f"]["kps"])
        assert 2 <= len(c["f"]["kps"]) and n <= 40, name
        for entry in c["takes"]:
            assert censuses[name][entry] >= 1, (name, entry)
        named.update(c["takes"])
    assert named == set(BR.CENSUS)


def test_every_switch_changes_a_result():
    named = set()
    for name, c in BC.hand_made().items():
        for s in c["switches"]:
            assert not _same(BR.search_by_bow_rig(c["kf"]["kps"], c["kf"]["desc"], c["kf"]["flags"], c["kf"]["fv"], c["f"]["kps"],
                                                  c["f"]["desc"], c["f"]["n_left"], c["f"]["fv"], c["ratio"], c["ori"], [s]),
                             BC.reference(c)), (name, s)
        named.update(c["switches"])
    assert named == set(BR.SWITCHES)
    # and on the realistic scene, where nobody arranged it (but both cameras turned alike: the histograms agree per side)
    c = BC.realistic()["real_lu2_r7_ori"]
    for s in set(BR.SWITCHES) - {"hist_per_side"}:
        assert not _same(BC.reference(c, [s]), BC.reference(c)), s


def test_lanes_hold_several_candidates_at_levelsup_2():
    c = BC.realistic()["real_lu2_r7_ori"]
    per_node = np.diff(c["f"]["fv"]["fv_off"])
    assert per_node.max() > 64
    root = BC.realistic()["real_lu3_r7_ori"]["f"]["fv"]
    assert len(root["fv_nodes"]) == 1 and root["fv_off"][1] > 900
    o = BC.overflow()
    assert o["f"]["fv"]["fv_off"][1] == 2049 and len(o["f"]["kps"]) == 2049


def test_batch_shapes():
    jobs, f, _, _ = BC.batch()
    assert len(jobs) == 5 and len({len(j["kps"]) for j in jobs}) >= 4
    assert any(len(j["kps"]) > 0 and j["n_left"] == len(j["kps"]) for j in jobs)  # n_right == 0
    assert any(len(j["kps"]) == 0 for j in jobs)


# ---- 3. the host twin
def test_host_twin_equals_restatement_on_every_case():
    for name, c in BC.cases().items():
        assert _same(_twin(c), BC.reference(c)), name
    o = BC.overflow()
    assert _same(_twin(o), BC.reference(o)) and BC.reference(o)[0] > 10  # no 2048 rule on the host
    jobs, f, ratio, ori = BC.batch()
    for j, k in enumerate(jobs):
        c = dict(kf=k, f=f, ratio=ratio, ori=ori)
        assert _same(_twin(c), BC.reference(c)), j


def test_host_twin_refuses_a_broken_featurevector():
    c = BC.hand_made()["both_written"]
    bad = dict(c["f"])
    bad["fv"] = dict(c["f"]["fv"], fv_feat=np.array([0, 1, 3], np.int32))
    with pytest.raises(V.VslamError):
        _twin(dict(c, f=bad))


def test_stand_alone_host_check_agrees(tmp_path):
    """tests/tools/bow_rig_host_check.cpp over the exported cases (the sanitizer build of the same program is made by hand:
    its header says how)"""
    exe = str(tmp_path / "bow_rig_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "tools", "bow_rig_host_check.cpp"), "-o", exe, "-L", os.path.join(ROOT, "vi_slam_amd"),
           "-lvslam_host", "-Wl,-rpath," + os.path.join(ROOT, "vi_slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "cases")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "dump_bow_rig_cases.py"), out], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    files = sorted(os.path.join(out, f) for f in os.listdir(out))
    assert len(files) == len(BC.cases()) + 1 + 5
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == len(files)


# ---- 4. ComputeBoW of a rig
@pytest.mark.parametrize("levelsup", (0, 2))
def test_assemble_of_the_concatenation_equals_the_oracle(levelsup):
    f = BC.frame()
    voc = BC.vocabulary()
    nl = f["n_left"]
    want = orbo.bow_transform(voc, f["desc"], levelsup)
    left, right = orbo.bow_transform(voc, f["desc"][:nl], levelsup), orbo.bow_transform(voc, f["desc"][nl:], levelsup)
    got = V.bow_assemble_rig(int(voc.get("weighting", 0)), int(voc.get("norm", 1)),
                             (left["word"], left["weight"], left["nid"]), (right["word"], right["weight"], right["nid"]))
    for k in ("word", "weight", "nid", "bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat"):
        assert np.array_equal(got[k], want[k]), k
    assert got["n_left"] == nl and got["n_right"] == len(f["kps"]) - nl
    assert (got["fv_feat"] >= nl).any() and (got["fv_feat"] < nl).any()


# ---- 5. the ABI
def test_header_mirror_and_shim_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in V.ABI_SYMBOLS
    m = re.search(r"typedef struct vslam_bow_rig_kf \{(.*?)\} vslam_bow_rig_kf;", header, re.S)
    fields = re.findall(r"\b(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in V._BowRigKf._fields_], fields
    assert "vslamh_search_by_bow_rig" in open(os.path.join(ROOT, "vi_slam_amd", "csrc", "vslam_host.h")).read()
    for name in ("SearchByBoWRig", "SearchByBoWRig_async", "SearchByBoWRig_wait", "SearchByBoWKeyFramesRig"):
        assert hasattr(V.FMatcher, name), name
    assert hasattr(V.Vocabulary, "transform_rig")
    shim = open(os.path.join(ROOT, "include", "vslam_shim.hpp")).read()
    for s in ("vslam_search_by_bow_rig(", "vslam_search_by_bow_keyframes_rig(", "RigKeyFrameView"):
        assert s in shim, s
