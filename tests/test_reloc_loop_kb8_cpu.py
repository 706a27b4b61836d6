"""The relocalisation and the loop-closing SearchByProjection for fisheye cameras (fmatcher.cpp:2689-2811, :750-863), the CPU
part:
1. pin: with the "pinhole" switch the numpy restatement (tests/reloc_loop_kb8_ref.py) equals
   projection_bounds_ref.search_by_projection_keyframe / search_by_projection_sim3 and oracle/orbo.py's functions of the same
   names on the gate tables keyframe and sim3proj of tests/matcher_gate_cases.py, both gemm builds;
2. conditions: the cases of tests/reloc_loop_kb8_cases.py reach every census entry, every switch changes a result, the
   hand-made rows end where they say, the long lists gate as many points as the issue asks;
3. twin: the host twins (vslamh_search_by_projection_keyframe_kb8, vslamh_search_by_projection_sim3_kb8, libvslam_host.so) equal
   the restatement on every case, the job the device entry refuses included;
4. the ABI: symbols, struct sizes, the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from host_sources import host_sources
import kb8_ref as KR
import matcher_gate_cases as G
import reloc_loop_kb8_cases as RC
import reloc_loop_kb8_ref as RL
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vslam_search_by_projection_keyframe_kb8", "vslam_search_by_projection_sim3_kb8_async",
               "vslam_search_by_projection_sim3_kb8_wait", "vslam_search_by_projection_sim3_kb8", "vslam_fe_get_sim3_kb8_profile"]
A_SWITCHES = ("depth_test", "left_only_angles", "last_tie", "pinhole")
B_SWITCHES = ("closed_upper", "level_plus", "last_tie", "z_le_0", "float_normal_dot", "pinhole")


# ---- 1. pin to the oracle
def _pin_cam():
    return KR.camera(*G.CAM, (0, 0, 0, 0))


@pytest.mark.parametrize("dbl", [True, False])
def test_with_a_pinhole_projection_a_is_the_oracles_keyframe_matcher(dbl):
    t = G.table("keyframe")
    a = G.inputs(t)
    sf = np.asarray(G.tables()["scale"], np.float32)
    for run in t.runs:
        r = dict(run, gemm_float=not dbl)
        want_np, want_or = G.reference(t, r, "numpy"), G.reference(t, r, "orbo")
        nm, m = RL.search_by_projection_keyframe_kb8(G.POSE, G.OW, _pin_cam(), t.th, run["orb_dist"], G.LSF, a["q_kps"], a["flags"],
                                                     a["x3dw"], a["mn"], a["mx"], a["desc_q"], a["kps"], a["desc"], sf, G.BOUNDS,
                                                     True, a["occupied"], dbl, None, ("pinhole",))
        assert (m >= 0).sum() >= 5
        for want in (want_np, want_or):
            assert nm == want[0] and np.array_equal(m, want[1]), run


@pytest.mark.parametrize("dbl", [True, False])
def test_with_a_pinhole_projection_b_is_the_oracles_sim3_matcher(dbl):
    t = G.table("sim3proj")
    a = G.inputs(t)
    sf = np.asarray(G.tables()["scale"], np.float32)
    ran = 0
    for run in t.runs:
        if run["variant"] != 0:
            continue  # :865-981 projects as a pinhole whatever the camera: it has no KB8 form
        r = dict(run, gemm_float=not dbl)
        want_np, want_or = G.reference(t, r, "numpy"), G.reference(t, r, "orbo")
        job = dict(pose=(G.POSE[:, :3], G.POSE[:, 3], G.OW), kps=a["kps"], desc=a["desc"], matched=a["occupied"], valid=None)
        m, nm, ng = RL.search_by_projection_sim3_kb8([job], a["pts"], a["desc_q"], _pin_cam(), t.th, run["ratio"], G.LSF, sf,
                                                     G.BOUNDS, dbl, ("pinhole",))
        assert (m[0] >= 0).sum() >= 5 and ng[0] >= nm[0]
        for want in (want_np, want_or):
            assert nm[0] == want[0] and np.array_equal(m[0], want[1]), run
        ran += 1
    assert ran >= 1


# ---- 2. the conditions on the cases
def test_the_wide_calibration_sees_behind_the_camera():
    fx, _, cx = RC.WIDE[:3]
    assert fx * np.pi / 2 < cx
    assert not RC.CAM1[0] * np.pi / 2 < RC.CAM1[2]


def test_cases_are_small():
    for c in RC.a_cases().values():
        assert len(c["cur_kps"]) <= 300 and len(c["kf_kps"]) <= 300
    for name, c in RC.b_cases().items():
        assert all(len(j["kps"]) <= 300 for j in c["jobs"]), name
        if name not in ("b_long", "b_4096", "b_4097"):
            assert len(c["pts"]) <= 300, name
    assert len(RC.b_cases()["b_six"]["jobs"]) == 6
    assert 20 <= len(RC.a_cases()["a_hand"]["cur_kps"]) <= 60


def test_every_census_entry_is_reached():
    total = dict.fromkeys(RL.CENSUS, 0)
    for name in RC.a_cases():
        for k, v in RC.reference_a(name)[2].items():
            total[k] += v
    for name in RC.b_cases():
        for k, v in RC.reference_b(name)[3].items():
            total[k] += v
    assert all(v > 0 for v in total.values()), {k: v for k, v in total.items() if v == 0}
    hand = RC.reference_a("a_hand")[2]
    assert hand.get("a_behind_inside_takes_keypoint", 0) == 1 and hand.get("a_right_angle_differs_from_left", 0) >= 1
    assert RC.reference_b("b_hand")[3].get("b_prefix_runs_off_its_end", 0) >= 1


@pytest.mark.parametrize("switch", RL.SWITCHES)
def test_every_switch_changes_a_result(switch):
    assert switch in A_SWITCHES + B_SWITCHES
    changed = False
    if switch in A_SWITCHES:
        want, got = RC.reference_a("a_hand"), RC.reference_a("a_hand", (switch,))
        changed = changed or got[0] != want[0] or not np.array_equal(got[1], want[1])
    if switch in B_SWITCHES and not changed:
        want, got = RC.reference_b("b_hand"), RC.reference_b("b_hand", (switch,))
        changed = not np.array_equal(got[0][0], want[0][0])
    assert changed, switch


@pytest.mark.parametrize("switch", ("depth_test", "left_only_angles"))
def test_the_a_switches_change_the_a_case(switch):
    want, got = RC.reference_a("a_hand"), RC.reference_a("a_hand", (switch,))
    assert got[0] != want[0] or not np.array_equal(got[1], want[1])


@pytest.mark.parametrize("switch", ("closed_upper", "level_plus", "last_tie", "z_le_0", "float_normal_dot"))
def test_the_b_switches_change_the_b_case(switch):
    want, got = RC.reference_b("b_hand"), RC.reference_b("b_hand", (switch,))
    assert not np.array_equal(got[0][0], want[0][0])


def test_hand_made_rows_of_a_end_where_they_say():
    c = RC.a_cases()["a_hand"]
    nm, m, _ = RC.reference_a("a_hand")
    row = {v: k for k, v in c["why"].items()}
    took = {int(q): int(i2) for i2, q in enumerate(m) if q >= 0}
    for name in ("behind_outside", "out_of_bounds", "below_min", "above_max", "empty_window", "occupied_on_entry", "not_flagged",
                 "above_orb_dist", "alone_in_bin_9"):
        assert row[name] not in took, name
    for name in ("behind_inside", "contest_winner", "contest_loser", "tie", "right_decides", "right_bin3", "bin0_0", "bin3_0",
                 "bin6_0"):
        assert row[name] in took, name
    assert row["right_decides"] == c["nl"] and c["kf_kps"]["angle"][0] == 270.0
    assert c["x3dw"][row["behind_inside"]][2] < 0
    kx = c["cur_kps"]["x"]
    assert took[row["contest_winner"]] + 1 == took[row["contest_loser"]]  # A, then B
    i = took[row["tie"]]
    assert kx[i] < kx[i - 1]  # the left column's keypoint, the later one of the array
    # without the right keypoint's own angle the entry falls with entry 0 into bin 9 and is dropped
    _, m2, _ = RC.reference_a("a_hand", ("left_only_angles",))
    assert m2[took[row["right_decides"]]] == -1
    # with a depth test the keypoint stays free
    _, m3, _ = RC.reference_a("a_hand", ("depth_test",))
    assert m3[took[row["behind_inside"]]] == -1


def test_hand_made_rows_of_b_end_where_they_say():
    c = RC.b_cases()["b_hand"]
    m, nm, ng, _ = RC.reference_b("b_hand")
    row = {v: k for k, v in c["why"].items()}
    took = {int(q): int(idx) for idx, q in enumerate(m[0]) if q >= 0}
    for name in ("invalid_point", "invalid_job", "above_threshold", "z_negative", "out_left", "out_right", "out_top", "out_bottom",
                 "u_eq_max_x_outside", "below_min_distance", "above_max_distance", "viewing_angle", "empty_window", "level_below",
                 "level_above", "matched_on_entry"):
        assert row[name] not in took, name
    for name in ("match", "z_zero_goes_on", "u_eq_min_x_inside", "tie_across_cells", "tie_within_cell", "contest_winner",
                 "contest_loser", "dot_double_lets_through") + tuple("prefix_%d" % k for k in range(9)):
        assert row[name] in took, name
    kx = c["jobs"][0]["kps"]["x"]
    assert took[row["contest_winner"]] + 1 == took[row["contest_loser"]]
    assert row["contest_winner"] < row["contest_loser"]
    i = took[row["tie_across_cells"]]
    assert kx[i] < kx[i - 1]
    i = took[row["tie_within_cell"]]
    assert kx[i] > kx[i + 1]
    first = took[row["prefix_0"]]
    assert [took[row["prefix_%d" % k]] for k in range(9)] == list(range(first, first + 9))
    assert nm[0] == len(took) and ng[0] >= nm[0]


def test_the_long_lists_gate_what_the_issue_asks():
    c = RC.b_cases()["b_long"]
    assert 5500 <= len(c["pts"]) <= 6500
    assert 1000 <= RC.reference_b("b_long")[2][0] <= 4096
    m, nm, ng, _ = RC.reference_b("b_4096")
    assert ng[0] == 4096 and RC.b_cases()["b_4096"]["refuse"] is None
    m, nm, ng, _ = RC.reference_b("b_4097")
    assert ng[1] == 4097 and ng[0] < 4096 and RC.b_cases()["b_4097"]["refuse"] == 1
    assert nm[1] > 100 and nm[0] >= 0  # the host serves the job the device refuses


# ---- 3. the host twins
def twin_a(c):
    g = RC.golden()
    return V.search_by_projection_keyframe_kb8_host(V.kb8_camera(*c["cam"]), c["T"], c["Ow"], c["th"], c["orb_dist"], RC.LSF,
                                                    c["kf_kps"], c["flags"], c["x3dw"], c["mn"], c["mx"], c["desc"], c["cur_kps"],
                                                    c["cur_desc"], RC.IMG, g["sf"], c["occupied"], None, c["check_ori"], c["gf"])


def host_jobs(c):
    keep, jobs = [], []
    for j in c["jobs"]:
        k = np.ascontiguousarray(j["kps"], V.KP_DTYPE)
        d = np.ascontiguousarray(j["desc"], np.uint8)
        keep += [k, d]
        jobs.append(V.sim3_kb8_job(*j["pose"], k.ctypes.data if len(k) else 0, d.ctypes.data if len(k) else 0, len(k),
                                   j.get("matched"), j.get("valid")))
    return jobs, keep


def twin_b(c):
    jobs, keep = host_jobs(c)
    return V.search_by_projection_sim3_kb8_host(V.kb8_camera(*RC.CAM1), jobs, c["pts"], c["desc"], c["th"], c["ratio"], RC.LSF,
                                                RC.IMG, RC.golden()["sf"], gemm_float=c["gf"])


@pytest.mark.parametrize("name", sorted(RC.a_cases()))
def test_host_twin_of_a_equals_the_restatement(name):
    nm, m = twin_a(RC.a_cases()[name])
    want = RC.reference_a(name)
    assert nm == want[0] and np.array_equal(m, want[1]), (name, np.nonzero(m != want[1])[0][:5])


@pytest.mark.parametrize("name", sorted(RC.b_cases()))
def test_host_twin_of_b_equals_the_restatement(name):
    m, nm, ng = twin_b(RC.b_cases()[name])
    want = RC.reference_b(name)
    assert np.array_equal(nm, want[1]) and np.array_equal(ng, want[2]), (name, nm, ng)
    for j in range(len(m)):
        assert np.array_equal(m[j], want[0][j]), (name, j, np.nonzero(m[j] != want[0][j])[0][:5])


def test_host_twins_refuse_bad_arguments():
    c = RC.a_cases()["a_hand"]
    with pytest.raises(V.VslamError):
        twin_a(dict(c, orb_dist=0))
    with pytest.raises(V.VslamError):
        twin_a(dict(c, orb_dist=256))
    b = RC.b_cases()["b_one"]
    with pytest.raises(V.VslamError):
        twin_b(dict(b, th=-1))
    with pytest.raises(V.VslamError):
        twin_b(dict(b, jobs=[]))


def test_stand_alone_host_check_runs_clean_under_sanitizers(tmp_path):
    """tests/tools/reloc_loop_kb8_host_check.cpp and the host sources as ONE program with -fsanitize=address,undefined, over
    every exported case"""
    exe = str(tmp_path / "reloc_loop_kb8_host_check")
    # -O0: half the build time of -O1
    cmd = ["g++", "-std=c++17", "-O0", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "reloc_loop_kb8_host_check.cpp"),
           *host_sources(), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "cases")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "dump_reloc_loop_kb8_cases.py"), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = sorted(os.path.join(out, f) for f in os.listdir(out))
    assert len(files) == len(RC.a_cases()) + len(RC.b_cases())
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # a sanitizer report goes there
    assert r.stdout.count("ok:") == len(files)
    assert cmd.count("-fno-sanitize-recover=all") == 1 and cmd.count("-ffp-contract=off") == 1


# ---- 4. the ABI
def test_header_mirror_and_host_header_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in V.ABI_SYMBOLS
    for struct, mirror in (("vslam_sim3_kb8_job", V._Sim3Kb8Job), ("vslam_sim3_kb8_params", V._Sim3Kb8Params)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = re.findall(r"\b(\w+)(?:\[\d+\])?\s*[;,]", body)
        assert fields == [n for n, _ in mirror._fields_], fields
    assert C.sizeof(V._Sim3Kb8Job) == 104 and C.sizeof(V._Sim3Kb8Params) == 24
    assert re.search(r"#define VSLAM_SIM3_KB8_MAX_JOBS %d\b" % V.SIM3_KB8_MAX_JOBS, header)
    host_hdr = open(os.path.join(ROOT, "vi_slam_amd", "csrc", "vslam_host.h")).read()
    assert "vslamh_search_by_projection_keyframe_kb8" in host_hdr and "vslamh_search_by_projection_sim3_kb8" in host_hdr
    for name in ("search_by_projection_sim3_kb8", "search_by_projection_sim3_kb8_async", "search_by_projection_sim3_kb8_wait",
                 "get_sim3_kb8_profile"):
        assert hasattr(V.FExtractor, name), name
    assert hasattr(V.FMatcher, "SearchByProjectionKeyFrameKB8")
    # the oddity is stated where the Fuse entry states its own
    assert "ODDITY, NOT reproduced" in header.split("vslam_search_by_projection_keyframe_kb8(")[0].split("Tracking::Relocalization")[-1]


def test_the_host_library_exports_the_twins():
    L = V.host_lib()
    assert L.vslamh_search_by_projection_keyframe_kb8 and L.vslamh_search_by_projection_sim3_kb8
