"""include/vslam_shim.hpp, DBoW3::Vocabulary create / save: the demo compiles and links (CPU), and on the GPU prints the
node table the Python path computes for clu3000 and writes the file the Python path writes."""
import json
import os
import subprocess

import numpy as np
import pytest

import voc_train_cases as cases
import voc_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "voc_train_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "voc_train_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_voc_train_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_voc_train_demo_equals_python_path(tmp_path):
    import vi_slam_amd as V
    exe = _build(tmp_path)
    desc, off, kw = cases.inputs("clu3000")
    case, out = tmp_path / "case.bin", tmp_path / "demo.dbow3"
    with open(case, "wb") as f:
        f.write(np.array([len(off) - 1, kw["k"], kw["L"], kw["seed"]], np.int64).tobytes())
        f.write(np.asarray(off, np.int64).tobytes())
        f.write(np.ascontiguousarray(desc).tobytes())
    r = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(line) for line in r.stdout.strip().splitlines()]
    got = lines[0]
    voc = V.train_vocabulary(desc, off, **kw)
    ref.assert_same(voc, cases.expected("clu3000"), "clu3000")
    for key in ("child_start", "child_count", "child_ids", "word_id"):
        assert got[key] == voc[key].tolist(), key
    assert got["desc"] == voc["desc"].reshape(-1).tolist()
    assert got["weight_bits"] == voc["weight"].view(np.uint64).tolist()
    assert (got["k"], got["L"], got["words"], got["passes"]) == (kw["k"], kw["L"], voc["n_words"], voc["stats"]["total_passes"])
    assert lines[1] == {"reloaded_words": voc["n_words"], "on_device": 1}
    mine = tmp_path / "python.dbow3"
    V.save_vocabulary_file(voc, str(mine))
    assert out.read_bytes() == mine.read_bytes()
