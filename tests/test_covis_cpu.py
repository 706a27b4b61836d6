"""The covisibility mirror, the CPU part: the bookkeeping (vslam_covis_host.cpp) and the host twins of the queries
(vslamh_covis_*, libvslam_host.so) against the line-by-line restatement tests/covis_ref.py.
1. mutators: a random sequence of a few thousand calls, get_point compared after each; growth and compaction seen in stats;
2. census: the query cases of tests/covis_cases.py reach every listed branch by the restatement alone;
3. twins: every query case through vslamh_covis_connections / vslamh_covis_culling;
4. walk: a cull changes a later job's counts; the walk rule through the twin equals a sequential restatement;
5. golden: tests/golden/covis_small.npz pins the restatement's outputs;
6. the stand-alone check program under -fsanitize=address,undefined; 7. the ABI."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
import vi_slam_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = [s for s in V.ABI_SYMBOLS if s.startswith("vslam_covis_")]


def run_both(twin, op, ok):
    if ok:
        return getattr(twin, op[0])(*op[1:])
    with pytest.raises(V.VslamError) as e:
        getattr(twin, op[0])(*op[1:])
    assert e.value.code == V.ERR_INVALID, op


# ---- 1. the bookkeeping
def test_random_mutations_match_the_restatement_after_every_call():
    twin, g = V.CovisibilityMapHost(initial_entries=8), CR.Graph()
    n_ok = 0
    for step, (op, ok) in enumerate(CC.random_mutations(4000, seed=11)):
        want = None
        if ok:
            want = getattr(g, op[0])(*op[1:])
            n_ok += 1
        got = run_both(twin, op, ok)
        if ok and op[0] == "erase_observation":
            assert got == want, (step, op)
        touched = [op[1]] if op[0] in ("add_point", "add_observation", "erase_observation", "clear_point") and op[1] in g.mps \
            else (list(g.mps) if step % 97 == 0 or op[0] in ("clear_map", "clear", "erase_keyframe") else [])
        for m in touched:
            CC.same_point(twin.get_point(m), g.get_point(m))
        assert twin.size() == g.size(), (step, op)
    assert n_ok > 2500, n_ok
    for m in g.mps:
        CC.same_point(twin.get_point(m), g.get_point(m))
    st = twin.stats()
    assert st["growths"] >= 1 and st["compactions"] >= 1 and st["used"] <= st["capacity"], st


def test_segments_regrow_and_unknown_ids_are_refused():
    twin = V.CovisibilityMapHost(initial_entries=4)
    g = CR.Graph()
    ops = CC.random_scene(320, 1, 0, seed=1)
    ops += [("add_observation", 0, k, k, False, k % 8, False) for k in range(300)]  # 4 -> 8 -> .. -> 512 records
    CC.apply(twin, ops)
    CC.apply(g, ops)
    CC.same_point(twin.get_point(0), g.get_point(0))
    assert twin.stats()["growths"] >= 7
    for bad in (lambda: twin.add_point(0), lambda: twin.add_point(-3), lambda: twin.get_point(5), lambda: twin.erase_keyframe(3),
                lambda: twin.add_keyframe(999, 0, CC.key_of(3)), lambda: twin.add_observation(0, 1, 0, level=64),
                lambda: twin.add_keyframes([500, 500], [0, 0], [1, 2]), lambda: twin.erase_observation(0, 4000)):
        with pytest.raises(V.VslamError) as e:
            bad()
        assert e.value.code == V.ERR_INVALID
    CC.same_point(twin.get_point(0), g.get_point(0))
    assert twin.size() == g.size()


# ---- 2. the census
def reference_results():
    ops, jobs = CC.connections_scene()
    g = CC.build(ops)
    conn = [g.connections(j) for j in jobs]
    ops2, jobs2 = CC.culling_scene()
    g2 = CC.build(ops2)
    cull = [g2.culling(j) for j in jobs2]
    return g, conn, g2, cull


def test_census():
    g, conn, g2, cull = reference_results()
    census = g.census + g2.census
    missing = [c for c in CC.CENSUS if not census[c]]
    assert not missing, missing
    # the cases say what they are for
    assert conn[0]["ordered_w"][:2] == [21, 21] and 15 in conn[0]["ordered_w"] and 14 not in conn[0]["ordered_w"]
    assert 14 in conn[0]["counter_n"] and conn[0]["kf_max"] == g._ordered([1, 2])[0]
    assert conn[1]["ordered_w"] == [3] and conn[1]["counter_n"] == [3, 3] and conn[2]["counter_kf"] == []
    assert conn[7]["error"] == 1 and conn[8]["error"] == 2
    assert 10 not in conn[4]["counter_kf"] and 9 in conn[4]["counter_kf"] and 0 in conn[4]["counter_kf"]
    assert (cull[0]["n_mps"], cull[0]["n_redundant"]) == (6, 2)
    assert cull[3]["error"] == 1 and cull[4]["error"] == 2


# ---- 3. the host twins
def test_host_twin_connections_equal_the_restatement():
    ops, jobs = CC.connections_scene()
    g, twin = CC.build(ops), CC.build(ops, V.CovisibilityMapHost(initial_entries=16))
    got = twin.connections(jobs)
    for j, job in enumerate(jobs):
        CC.same_connections(got[j], g.connections(job))
    for j, job in enumerate(jobs):  # and one at a time
        CC.same_connections(twin.connections([job])[0], g.connections(job))


def test_host_twin_culling_equals_the_restatement():
    ops, jobs = CC.culling_scene()
    g, twin = CC.build(ops), CC.build(ops, V.CovisibilityMapHost(initial_entries=16))
    assert twin.culling(jobs) == [g.culling(j) for j in jobs]
    assert twin.culling(jobs, th_obs=2) == [g.culling(j, 2) for j in jobs]


@pytest.mark.parametrize("seed", [3, 4])
def test_host_twin_on_random_scenes(seed):
    ops = CC.random_scene(70, 400, 9, seed, n_maps=2)
    g, twin = CC.build(ops), CC.build(ops, V.CovisibilityMapHost())
    rng = np.random.RandomState(seed)
    for k in rng.choice(70, 6, replace=False):
        g.set_keyframe_bad(int(k))
        twin.set_keyframe_bad(int(k))
    jobs = [dict(mode=int(j % 2), self_kf=int(j), map_id=int(j % 2), min_obs=int(j % 5),
                 mp_ids=[None if v < 0 else int(v) for v in rng.randint(-40, 400, size=int(rng.randint(0, 300)))]) for j in range(20)]
    for got, job in zip(twin.connections(jobs), jobs):
        CC.same_connections(got, g.connections(job))
    cj = [dict(kf_id=j["self_kf"], mp_ids=j["mp_ids"], levels=list(rng.randint(0, 8, size=len(j["mp_ids"])))) for j in jobs]
    assert twin.culling(cj) == [g.culling(j) for j in cj]
    with pytest.raises(V.VslamError):
        twin.connections([jobs[0]] * 129)
    with pytest.raises(V.VslamError):
        twin.connections([dict(jobs[0], mp_ids=[0] * 8193)])
    with pytest.raises(V.VslamError):
        twin.connections([dict(jobs[0], mode=2)])


# ---- 4. the culling walk
def test_a_cull_changes_a_later_job_and_the_walk_rule_follows_it():
    ops, jobs, th = CC.walk_scene()
    # the reference, sequentially: examine, cull, examine the next
    g = CC.build(ops)
    one_shot = [g.culling(j) for j in jobs]
    seq, culled = [], []
    for j in jobs:
        r = g.culling(j)
        seq.append(r)
        if r["n_redundant"] > th * r["n_mps"]:
            CR.keyframe_set_bad_flag(g, j["kf_id"], j["mp_ids"])
            culled.append(j["kf_id"])
    assert culled == [1] and one_shot[0] == seq[0]
    assert one_shot[1] != seq[1] and one_shot[1]["n_redundant"] > th * one_shot[1]["n_mps"], "the cull must change job 1"
    # the walk through the twin
    twin = CC.build(ops, V.CovisibilityMapHost())
    calls = []

    def run(js):
        calls.append(len(js))
        return twin.culling(js)
    got, got_culled = CC.culling_walk(run, jobs, th, lambda j: CR.keyframe_set_bad_flag(twin, j["kf_id"], j["mp_ids"]))
    assert got == seq and got_culled == culled and calls == [3, 2]
    for m in g.mps:
        CC.same_point(twin.get_point(m), g.get_point(m))


# ---- 5. the golden file
def test_golden_pins_the_restatement():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_covis_golden as MG
    want = np.load(os.path.join(ROOT, "tests", "golden", "covis_small.npz"))
    got = MG.arrays()
    assert sorted(got) == sorted(want.files)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


# ---- 6. the stand-alone program
def test_stand_alone_host_check_runs_clean_under_sanitizers(tmp_path):
    """tests/tools/covis_host_check.cpp and vslam_covis_host.cpp as ONE program with -fsanitize=address,undefined: it replays
    the dumped mutation sequence (growth, compaction, erase) and the query cases, comparing with the dumped expectations"""
    exe = str(tmp_path / "covis_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "covis_host_check.cpp"),
           os.path.join(ROOT, "vi_slam_amd", "csrc", "vslam_covis_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "cases")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "dump_covis_cases.py"), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = sorted(os.path.join(out, f) for f in os.listdir(out))
    assert len(files) == 4
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compactions" in r.stdout


# ---- 7. the ABI
def test_header_mirror_and_libraries_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "vslam_fe.h")).read()
    assert len(NEW_SYMBOLS) == 26
    L, H = C.CDLL(V.LIB_PATH), C.CDLL(V.HOST_LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % s, header), s
        assert hasattr(L, s), s
    for s in ("create", "add_observation", "connections", "culling", "connections_lists", "get_point"):
        assert hasattr(H, "vslamh_covis_" + s) and hasattr(L, "vslamh_covis_" + s), s
    for struct, mirror, size in (("vslam_covis_job", V._CovisJob, 32), ("vslam_covis_result", V._CovisResult, 32),
                                 ("vslam_covis_cull_job", V._CovisCullJob, 32), ("vslam_covis_cull_result", V._CovisCullResult, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\b(\w+)\s*[;,]", body)
        assert fields == [n for n, _ in mirror._fields_], fields
        assert C.sizeof(mirror) == size
    assert V.COVIS_OBS_DTYPE.itemsize == 32
    assert re.search(r"#define VSLAM_COVIS_MAX_JOBS %d\b" % V.COVIS_MAX_JOBS, header)
    assert re.search(r"#define VSLAM_COVIS_MAX_LIST %d\b" % V.COVIS_MAX_LIST, header)
    shim = open(os.path.join(ROOT, "include", "vslam_shim.hpp")).read()
    assert "class CovisibilityMap" in shim and "KeyFrameCulling" in shim and "neighbours" in shim
