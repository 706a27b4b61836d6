"""The search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye KeyFrame / a two-fisheye rig
(fmatcher.cpp:1918-2119, :2121-2243), the CPU part:
1. pin: with the "pinhole" switch, camera 0 and idx_offset 0 the numpy restatement (tests/fuse_rig_ref.py) equals
   orbo.fuse_search with mvuRight = -1 on the gate tables fuse and fuse_sim3 of tests/matcher_gate_cases.py, both gemm builds;
2. conditions: the cases of tests/fuse_rig_cases.py reach every census entry, the hand-made rows leave where they say, and every
   switch changes at least one result;
3. twin: the host twin (vslamh_fuse_search_rig, libvslam_host.so) equals the restatement on every case, the ones the device entry
   refuses included; the stand-alone check program, built with -fsanitize=address,undefined, runs every exported case clean;
4. walk: on a toy map with observations and MapPoint::Replace, ONE batch search plus the walk rule equals the sequential
   search-and-mutate reference where a survivor's descriptor changes between KeyFrames, and does not without the stale rule;
5. the ABI: header, Python mirror and host header name the new entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fuse_rig_cases as FC
import fuse_rig_ref as FR
import fuse_rig_walk as FW
from host_sources import host_sources
import kb8_ref as KR
import matcher_gate_cases as G
import vi_slam_amd as V
from oracle import orbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vslam_fuse_search_rig_async", "vslam_fuse_search_rig_wait", "vslam_fuse_search_rig",
               "vslam_fe_get_fuse_rig_profile"]
SERVED = [n for n in sorted(FC.cases()) if FC.cases()[n]["refuse"] is None]


# ---- 1. pin to the oracle
@pytest.mark.parametrize("dbl", [True, False])
@pytest.mark.parametrize("name", ["fuse", "fuse_sim3"])
def test_with_a_pinhole_projection_it_is_the_oracles_fuse(name, dbl):
    t = G.table(name)
    a = G.inputs(t)
    tab = G.tables()
    sf, isig2 = np.asarray(tab["scale"], np.float32), np.asarray(tab["inv_sigma2"], np.float32)
    none = np.full(len(a["kps"]), -1.0, np.float32)  # a rig's mvuRight
    want_i, want_d = orbo.fuse_search(a["pts"], a["desc_q"], a["kps"], a["desc"], none, sf, isig2, G.POSE[:, :3], G.POSE[:, 3], G.OW,
                                      G.CAM + (float(G.BF),), t.th, G.LSF, G.W, G.H, name == "fuse_sim3", dbl)
    cam = KR.camera(*G.CAM, (0, 0, 0, 0))
    job = dict(pose=(G.POSE[:, :3], G.POSE[:, 3], G.OW), left_pose=None, camera=0, sim3=name == "fuse_sim3", kps=a["kps"],
               desc=a["desc"], idx_offset=0, valid=None)
    bi, bd = FR.fuse_search_rig([job], a["pts"], a["desc_q"], (cam, None), t.th, G.LSF, sf, isig2, G.BOUNDS, dbl, ("pinhole",))
    assert (bi[0] >= 0).sum() >= 10
    assert np.array_equal(bi[0], want_i)
    assert np.array_equal(np.minimum(bd[0], 256), np.minimum(want_d, 256))


# ---- 2. the conditions on the cases
def test_the_cameras_differ_and_the_rig_is_real():
    g = FC.golden()
    assert FC.CAM1[:5] != FC.CAM2[:5] and all(a != b for a, b in zip(FC.CAM1[:4], FC.CAM2[:4]))
    Tlr = np.asarray(g["rig"]["Tlr"])
    assert np.linalg.norm(Tlr[:, 3]) > 0.05 and not np.allclose(Tlr[:, :3], np.eye(3), atol=0.1)
    s = FC.cases()["scene"]
    assert len(s["jobs"]) == 6 and 1300 <= len(s["pts"]) <= 1500
    assert [j["camera"] for j in s["jobs"]] == [0, 1] * 3
    assert len(g["kl"]) == 456 and len(g["kr"]) == 457
    h = FC.cases()["hand"]
    assert 1 <= len(h["pts"]) <= 40 and all(4 <= len(j["kps"]) <= 40 for j in h["jobs"])


def test_every_census_entry_is_reached():
    total = dict.fromkeys(FR.CENSUS, 0)
    for name in SERVED:
        for k, v in FC.reference(name)[2].items():
            total[k] += v
    assert all(v > 0 for v in total.values()), {k: v for k, v in total.items() if v == 0}
    hand = FC.reference("hand")[2]  # the hand-made case alone reaches them all
    assert all(hand.get(k, 0) > 0 for k in FR.CENSUS), [k for k in FR.CENSUS if not hand.get(k, 0)]
    scene = FC.reference("scene")
    assert (scene[0] >= 0).sum() > 1000 and ((scene[1] <= 50) & (scene[0] >= 0)).sum() > 800


def test_hand_made_rows_end_where_they_say():
    c = FC.cases()["hand"]
    bi, bd, _ = FC.reference("hand")
    nl = len(c["jobs"][0]["kps"])
    row = {v: k for k, v in c["why"].items()}
    L, R, S = 0, 1, 2
    for name in ("z_negative", "out_left", "out_right", "out_top", "out_bottom", "u_eq_max_x_outside", "below_min_distance",
                 "above_max_distance", "viewing_angle", "empty_window", "level_below", "level_above", "chi2_reject", "chi2_band",
                 "invalid_pointL"):
        assert bi[L, row[name]] == -1 and bd[L, row[name]] == 256, name
    for name in ("matchL", "z_zero_goes_on", "u_eq_min_x_inside", "tie_across_cells", "tie_within_cell", "least_distance"):
        assert 0 <= bi[L, row[name]] < nl, name
    assert bi[L, row["matchR"]] == -1 and bi[R, row["matchR"]] >= nl  # IsInKeyFrame for the left job, found by the right one
    assert bi[R, row["offset_applied"]] >= nl and bi[R, row["right_far_from_centre"]] >= nl
    assert bd[L, row["above_th_lowL"]] == 60 and bd[R, row["above_th_lowR"]] == 60
    # the tie across cells goes to the LEFT column's keypoint, which is the later one of the array; within a cell the lower index
    kx = c["jobs"][0]["kps"]["x"]
    i = bi[L, row["tie_across_cells"]]
    assert kx[i] < kx[i - 1] and bd[L, row["tie_across_cells"]] == 4
    i = bi[L, row["tie_within_cell"]]
    assert kx[i] > kx[i + 1] and bd[L, row["tie_within_cell"]] == 5
    assert bd[L, row["least_distance"]] == 3
    # sim3: no chi2 gate, and from INT_MAX a distance of 256 wins: the first of the window order
    assert bi[S, row["chi2_reject"]] >= 0 and bi[S, row["chi2_band"]] >= 0
    assert bi[L, row["sim3_far"]] == -1 and bd[S, row["sim3_far"]] == 256
    i = bi[S, row["sim3_far"]]
    assert i >= 0 and kx[i] < kx[i - 1]


@pytest.mark.parametrize("switch", FR.SWITCHES)
def test_every_switch_changes_a_result(switch):
    want = FC.reference("hand")
    got = FC.reference("hand", (switch,))
    assert not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])), switch


# ---- 3. the host twin
def _host_jobs(c):
    keep, jobs = [], []
    for j in c["jobs"]:
        k = np.ascontiguousarray(j["kps"], V.KP_DTYPE)
        d = np.ascontiguousarray(j["desc"], np.uint8)
        keep += [k, d]
        jobs.append(V.fuse_rig_job(*j["pose"], k.ctypes.data if len(k) else 0, d.ctypes.data if len(k) else 0, len(k), j["camera"],
                                   j["idx_offset"], j["valid"], j["sim3"]))
    return jobs, keep


def twin(c):
    g = FC.golden()
    jobs, keep = _host_jobs(c)
    rig = V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"])
    return V.fuse_search_rig_host(V.kb8_camera(*FC.CAM1), rig, jobs, c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG, g["sf"],
                                  g["is2"], gemm_float=c["gf"])


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_host_twin_equals_the_restatement(name):
    bi, bd = twin(FC.cases()[name])
    want = FC.reference(name)
    bad = np.argwhere((bi != want[0]) | (bd != want[1]))
    assert len(bad) == 0, (name, bad[:5])


def test_host_twin_places_the_window_from_the_keyframes_integer_origin():
    """FC.keyframe_origin(): bounds with fractions over cells narrower than a pixel, where the KeyFrame's truncated window origin
    leaves out a keypoint within the radius that the Frame's float origin would reach"""
    c, g = FC.keyframe_origin(), FC.golden()
    args = (c["jobs"], c["pts"], c["desc"], g["cams"], c["th"], FC.LSF, g["sf"], g["is2"], c["bounds"])
    want = FR.fuse_search_rig(*args)
    assert want[0].tolist() == [[-1, 1]] and want[1].tolist() == [[256, 1]]
    jobs, keep = _host_jobs(c)
    got = V.fuse_search_rig_host(V.kb8_camera(*FC.CAM1), None, jobs, c["pts"], c["desc"], c["th"], FC.LSF, FC.IMG, g["sf"], g["is2"],
                                 bounds=c["bounds"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)


def test_host_twin_refuses_bad_jobs():
    c = FC.cases()["np1"]
    for change in (dict(camera=2), dict(sim3=True, camera=1)):
        with pytest.raises(V.VslamError):
            twin(dict(c, jobs=[dict(c["jobs"][0], **change)]))


def test_stand_alone_host_check_runs_clean_under_sanitizers(tmp_path):
    """tests/tools/fuse_rig_host_check.cpp and the host sources as ONE program with -fsanitize=address,undefined, over every
    exported case"""
    exe = str(tmp_path / "fuse_rig_host_check")
    # -O0: half the build time of -O1
    cmd = ["g++", "-std=c++17", "-O0", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "fuse_rig_host_check.cpp"),
           *host_sources(), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "cases")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "dump_fuse_rig_cases.py"), out], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    files = sorted(os.path.join(out, f) for f in os.listdir(out))
    assert len(files) == len(FC.cases())
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # a sanitizer report goes there
    assert r.stdout.count("ok:") == len(files)
    assert cmd.count("-fno-sanitize-recover=all") == 1 and cmd.count("-ffp-contract=off") == 1


# ---- 4. the walk
def _toy():
    """the scene's first 160 points against its three KeyFrames; every third keypoint slot of a KeyFrame holds a resident
    MapPoint with a descriptor of its own and one or three observations, the candidates have two"""
    s = FC.cases()["scene"]
    g = FC.golden()
    nl, nr = len(g["kl"]), len(g["kr"])
    n = 160
    rng = np.random.default_rng(74)
    m = FW.ToyMap({kf: nl for kf in range(3)})
    for pid in range(n):
        m.add_point(pid, s["desc"][pid])
        m.bad[pid] = not s["pts"]["valid"][pid]
        for far in (100, 101):  # two observations elsewhere
            m.n_left.setdefault(far, 10**6)
            m.slots.setdefault(far, {})
            m.add_observation(pid, far, pid)
    rid = 1000
    for kf in range(3):
        for idx in range(kf, nl + nr, 3):
            m.add_point(rid, rng.integers(0, 256, 32).astype(np.uint8))
            m.add_observation(rid, kf, idx)
            m.slots[kf][idx] = rid
            for far in range(102, 102 + (2 if idx % 2 else 0)):
                m.n_left.setdefault(far, 10**6)
                m.slots.setdefault(far, {})
                m.add_observation(rid, far, rid)
            rid += 1
    job_kf = [0, 0, 1, 1, 2, 2]
    host = []
    for j in s["jobs"]:
        k, d = np.ascontiguousarray(j["kps"], V.KP_DTYPE), np.ascontiguousarray(j["desc"], np.uint8)
        host.append((j, k, d))
    rig = V.kb8_rig(V.kb8_camera(*FC.CAM2), g["rig"]["Tlr"], g["rig"]["Trl"])
    cam = V.kb8_camera(*FC.CAM1)
    calls = []

    def search(mm, jobs, pids):
        pts = s["pts"][pids].copy()
        pts["valid"] = [0 if mm.bad[p] else 1 for p in pids]
        desc = np.array([mm.desc[p] for p in pids], np.uint8)
        jl = []
        for jn in jobs:
            j, k, d = host[jn]
            valid = np.array([0 if mm.in_keyframe(p, job_kf[jn]) else 1 for p in pids], np.uint8)
            jl.append(V.fuse_rig_job(*j["pose"], k.ctypes.data, d.ctypes.data, len(k), j["camera"], j["idx_offset"], valid))
        calls.append((len(jobs), len(pids)))
        return V.fuse_search_rig_host(cam, rig, jl, pts, desc, s["th"], FC.LSF, FC.IMG, g["sf"], g["is2"])

    return m, job_kf, list(range(n)), search, calls


def test_batch_search_and_walk_equal_the_sequential_reference():
    m, job_kf, points, search, calls = _toy()
    want = FW.sequential(m, job_kf, points, search)
    n_seq = len(calls)
    got, redone = FW.batch_walk(m, job_kf, points, search)
    assert calls[n_seq] == (6, len(points)) and len(calls) == n_seq + 1 + redone
    assert got.state() == want.state()
    assert len(want.log) > 100 and len(want.recomputed) > 5
    # a survivor's descriptor changed between KeyFrames and it was searched again afterwards
    assert redone > 0
    # and without the stale rule the result is another one
    wrong, _ = FW.batch_walk(m, job_kf, points, search, stale_rule=False)
    assert wrong.state() != want.state()
    # fused in the left job -> in the KeyFrame or bad: the right job of the same KeyFrame skips it
    for pid, kf, idx in want.log:
        assert want.bad[pid] or want.in_keyframe(pid, kf)


# ---- 5. the ABI
def test_header_mirror_and_host_header_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in V.ABI_SYMBOLS
    m = re.search(r"typedef struct vslam_fuse_rig_job \{(.*?)\} vslam_fuse_rig_job;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?\s*[;,]", body)
    assert fields == [n for n, _ in V._FuseRigJob._fields_], fields
    assert re.search(r"#define VSLAM_FUSE_RIG_MAX_JOBS %d\b" % V.FUSE_RIG_MAX_JOBS, header)
    assert "vslamh_fuse_search_rig" in open(os.path.join(ROOT, "vi_slam_amd", "csrc", "vslam_host.h")).read()
    for name in ("fuse_search_rig", "fuse_search_rig_async", "fuse_search_rig_wait", "get_fuse_rig_profile"):
        assert hasattr(V.FExtractor, name), name
    assert "Fuse(.., bRight)" not in header.split("Not covered:")[1].split("*/")[0]
