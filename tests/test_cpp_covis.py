"""include/vslam_shim.hpp, CovisibilityMap: the demo compiles and links (CPU); on the GPU it answers UpdateConnections / vote
jobs, walks KeyFrameCulling by the walk rule and feeds its `neighbours` helper to KeyFrameDatabase -- and prints what the
restatement tests/covis_ref.py and the Python path compute for the same case."""
import json
import os
import subprocess

import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
import kfdb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")
NUM, DEN = 1, 2  # redundant_th = 0.5, the inertial stereo value (localmapping.cpp:962)


def _build(tmp_path):
    exe = str(tmp_path / "covis_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "covis_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_covis_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def _bow_txt(v):
    return "%d %s" % (len(v[0]), " ".join("%d %.17g" % (i, x) for i, x in zip(v[0], v[1])))


def _ids(v):
    return " ".join(str(-1 if m is None else int(m)) for m in v)


@pytest.mark.gpu
def test_covis_demo_equals_restatement_and_python_path(tmp_path):
    import vi_slam_amd as V
    exe = _build(tmp_path)
    n_kf, n_mp, nw, rng = 16, 200, 600, np.random.default_rng(5)
    # a graph in which some keyframes are redundant: points seen by runs of neighbouring keyframes
    ops = [("add_keyframe", k, 0 if k < 14 else 1, CC.key_of(k)) for k in range(n_kf)]
    points = []
    for mp in range(n_mp):
        first, run = int(rng.integers(0, n_kf - 2)), int(rng.integers(2, 9))
        obs = [(k, mp, int(rng.integers(0, 4)) == 0, int(rng.integers(0, 5)), int(rng.integers(0, 3)) == 0)
               for k in range(first, min(first + run, n_kf))]
        points.append((mp, obs))
        ops.append(("add_point", mp))
        ops += [("add_observation", mp, k, idx, right, lv, st) for k, idx, right, lv, st in obs]
    ops.append(("set_keyframe_bad", 9))
    lists = {k: [mp for mp, obs in points if any(o[0] == k for o in obs)] + [None] for k in range(n_kf)}
    jobs = [dict(mode=CC.CONN, self_kf=k, map_id=0 if k < 14 else 1, min_obs=k % 4, mp_ids=lists[k]) for k in range(n_kf)]
    jobs.append(dict(mode=CC.VOTE, self_kf=-1, map_id=0, min_obs=0, mp_ids=lists[3] + lists[4]))
    cull = [dict(kf_id=k, mp_ids=lists[k], levels=[int(v) for v in rng.integers(2, 5, size=len(lists[k]))]) for k in range(1, 13)]
    bows = [R.random_bow(rng, nw, int(rng.integers(30, 120)), hi=300) for _ in range(n_kf)]
    queries = [(q % 2, bows[q] if q == 2 else R.random_bow(rng, nw, int(rng.integers(40, 150)), hi=300)) for q in range(4)]
    lines = [str(n_kf)] + ["%d %d %d" % (k, 0 if k < 14 else 1, CC.key_of(k)) for k in range(n_kf)]
    lines += [str(n_mp)] + ["%d %d %s" % (mp, len(obs), " ".join("%d %d %d %d %d" % o for o in obs)) for mp, obs in points]
    lines += ["1 9", str(len(jobs))]
    lines += ["%d %d %d %d %d %s" % (j["mode"], j["self_kf"], j["map_id"], j["min_obs"], len(j["mp_ids"]), _ids(j["mp_ids"])) for j in jobs]
    lines += ["%d %d %d" % (NUM, DEN, len(cull))]
    lines += ["%d %d %s" % (j["kf_id"], len(j["mp_ids"]), " ".join("%d %d" % (-1 if m is None else m, lv)
                                                                   for m, lv in zip(j["mp_ids"], j["levels"]))) for j in cull]
    lines += [str(nw)] + [_bow_txt(b) for b in bows]
    lines += [str(len(queries))] + ["%d %s" % (m, _bow_txt(b)) for m, b in queries]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [json.loads(line) for line in r.stdout.strip().splitlines()]

    # the restatement, sequentially
    g = CC.build(ops)
    for out, job in zip(got[:len(jobs)], jobs):
        CC.same_connections(out, g.connections(job))
    seq, culled = [], []
    for j in cull:
        res = g.culling(j)
        seq += [res["error"], res["n_mps"], res["n_redundant"]]
        if res["n_redundant"] * DEN > NUM * res["n_mps"]:
            CR.keyframe_set_bad_flag(g, j["kf_id"], j["mp_ids"])
            culled.append(j["kf_id"])
    walk = got[len(jobs)]
    assert walk == dict(walk=seq, culled=culled) and culled, walk
    # GetBestCovisibilityKeyFrames(10): an empty counter leaves the lists of the first UpdateConnections (keyframe.cpp:385)
    covis = {k: r["ordered_kf"][:10] for k, r in ((k, g.connections(jobs[k])) for k in range(n_kf)) if r["counter_kf"]}
    for k in range(n_kf):
        if k not in covis and got[k]["counter_kf"]:
            covis[k] = got[k]["ordered_kf"][:10]
    assert got[len(jobs) + 1] == dict(neighbours_of_first=covis.get(0, []))
    # the Python path of the selection stage with those lists
    fe, db = V.FExtractor(300, 1.2, 8, 20, 7, 320, 240), V.KeyFrameDatabase(nw)
    try:
        for k in range(n_kf):
            db.add(k, 0 if k < 14 else 1, bows[k])
        want = [dict(reloc=db.DetectRelocalizationCandidates(fe, b, m, covis)) for m, b in queries]
    finally:
        db.close()
        fe.close()
    assert got[len(jobs) + 2:-1] == want and any(w["reloc"] for w in want)
    assert got[-1] == dict(size=list(g.size()))
