"""include/vslam_shim.hpp, class HarrisGPU: vilib::HarrisGPU's constructor and read side over the C ABI of
include/vslam_harrisgrid.h.  CPU: the demo compiles and links.  GPU: set up as the reference's own detector test is
(test/harris-cuda/src/test_harris.cpp:143-154), it prints the kept points that tests/harris_ref.py computes."""
import json
import os
import subprocess

import numpy as np
import pytest

import harris_cases as HC
import harris_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vi_slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "harris_demo")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "harris_demo.cpp"), "-o", exe, "-L", PKG, "-lvslam_fe",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return exe


def _lines(ref):
    pos, sc, lv, keep, _ = ref
    return ["%d %.1f %.1f %08x %d" % (i, pos[i, 0], pos[i, 1], int(sc[i:i + 1].view(np.uint32)[0]), lv[i]) for i in np.nonzero(keep)[0]]


def test_harris_demo_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage error: no GPU call is made


@pytest.mark.gpu
def test_harris_demo_prints_the_restatements_kept_points(tmp_path):
    exe = _build(tmp_path)
    img = HC.crops()["hut"]
    h, w = img.shape
    path = str(tmp_path / "hut.raw")
    img.tofile(path)
    r = subprocess.run([exe, str(w), str(h), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip().splitlines()
    got = json.loads(out[-1])
    harris = hr.detect(img, (32, 32), 0, 1, (0, 0), hr.BORDER_SKIP, True, 0.04, 0.1, 0)
    shi = hr.detect(img, (32, 32), 0, 3, (0, 0), hr.BORDER_REFLECT_101, False, 0.04, 0.1, 0)
    assert [l[2:] for l in out[:-1] if l.startswith("P ")] == _lines(harris)
    assert [l[2:] for l in out[:-1] if l.startswith("S ")] == _lines(shi)
    assert got == {"cols": (w + 31) // 32, "rows": (h + 31) // 32, "harris_n": harris[4], "harris_count": harris[4], "shi_n": shi[4]}
    assert 3 < harris[4] < int((harris[1] > 0).sum()) and shi[4] > 3  # the relative threshold dropped some corners
