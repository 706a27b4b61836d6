"""include/vslam_shim.hpp, KeyFrameDatabase: the demo compiles and links (CPU), and prints the candidate lists the Python
path computes for one fixed case (GPU)."""
import json
import os
import subprocess

import numpy as np
import pytest

import kfdb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "kfdb_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "kfdb_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_kfdb_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


def _bow_txt(v):
    return "%d %s" % (len(v[0]), " ".join("%d %.17g" % (i, x) for i, x in zip(v[0], v[1])))


@pytest.mark.gpu
def test_kfdb_demo_equals_python_path(tmp_path):
    import vi_slam_amd as V
    exe = _build(tmp_path)
    nw, rng = 600, np.random.default_rng(31)
    kfs = [(10 + k, k % 3, R.random_bow(rng, nw, int(rng.integers(30, 120)), hi=300)) for k in range(14)]
    covis = {10 + k: (10 + rng.choice(16, int(rng.integers(0, 12)), replace=False)).tolist() for k in range(14)}
    queries = []  # kind, map, ncand, connected, bad maps, bow
    for j in range(6):
        bow = kfs[j][2] if j == 4 else R.random_bow(rng, nw, int(rng.integers(40, 150)), hi=300)
        queries.append((j % 2, j % 3, 1 + j % 3, [10 + j, 12] if j % 2 else [], [2] if j == 3 else [], bow))
    lines = ["%d %d" % (nw, len(kfs))] + ["%d %d %s" % (i, m, _bow_txt(v)) for i, m, v in kfs]
    lines += [str(len(covis))] + ["%d %d %s" % (i, len(n), " ".join(map(str, n))) for i, n in covis.items()]
    lines += [str(len(queries))] + ["%d %d %d %d %s %d %s %s" % (
        kind, m, nc, len(conn), " ".join(map(str, conn)), len(bad), " ".join(map(str, bad)), _bow_txt(bow))
        for kind, m, nc, conn, bad, bow in queries]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [json.loads(line) for line in r.stdout.strip().splitlines()]
    fe = V.FExtractor(300, 1.2, 8, 20, 7, 320, 240)
    db, ref, want = V.KeyFrameDatabase(nw), R.RefDatabase(nw), []
    try:
        for i, m, v in kfs:
            db.add(i, m, v)
            ref.add(i, m, *v)
        for kind, m, nc, conn, bad, bow in queries:
            if kind == 0:
                want.append({"reloc": db.DetectRelocalizationCandidates(fe, bow, m, covis)})
                assert want[-1]["reloc"] == ref.DetectRelocalizationCandidates(bow, m, covis)
            else:
                lo, me = db.DetectNBestCandidates(fe, bow, -1, m, conn, covis, nc, bad)
                want.append({"loop": lo, "merge": me})
                assert (lo, me) == ref.DetectNBestCandidates(bow, m, conn, covis, nc, bad)
        want.append({"size": db.size()[0]})
    finally:
        db.close()
        fe.close()
    assert got == want and any(w.get("reloc") for w in want) and any(w.get("loop") for w in want)
