"""CPU: settle the cv::undistortPoints restatement (tests/undistort_ref.py, the arithmetic of vslam_undistort.h) against
REAL OpenCV 4.2 output, IF a maintainer has produced it (tools/dump_opencv_undistort.cpp ->
tests/golden/opencv_undistort/out_undistort_*.bin; OpenCV is not in this image).  Without those files the OpenCV
comparison is skipped and the restatement stays "OpenCV 4.2 as recalled".  The consumer itself always runs: a dump in
the tool's format is synthesised from the restatement in a temporary directory and pushed through the same check."""
import glob
import os
import struct

import numpy as np
import pytest

import undistort_ref as U

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "opencv_undistort")
HAVE = bool(glob.glob(os.path.join(DIR, "out_undistort_*.bin")))


def read_blob(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"VSLD"
    kind, nd = struct.unpack_from("<II", raw, 4)
    dims = struct.unpack_from("<%dI" % nd, raw, 12)
    return kind, dims, np.frombuffer(raw[12 + 4 * nd:], np.float32).reshape(dims)


def write_blob(path, kind, arr):
    arr = np.ascontiguousarray(arr, np.float32)
    with open(path, "wb") as f:
        f.write(b"VSLD" + struct.pack("<II", kind, arr.ndim) + struct.pack("<%dI" % arr.ndim, *arr.shape) + arr.tobytes())


def check_dir(d):
    """every camera of the dump: the restatement equals OpenCV bit for bit; returns the cameras checked"""
    names = sorted(os.path.basename(p)[len("out_undistort_"):-len("_cam.bin")]
                   for p in glob.glob(os.path.join(d, "out_undistort_*_cam.bin")))
    assert names
    for name in names:
        kind, _, cam = read_blob(os.path.join(d, "out_undistort_%s_cam.bin" % name))
        assert kind == 9
        K, D = cam[:4], cam[4:4 + int(cam[9])]
        kind, _, rows = read_blob(os.path.join(d, "out_undistort_%s.bin" % name))
        assert kind == 8
        got = U.undistort_points(rows[:, :2], K, D)
        bad = np.nonzero(np.any(got.view(np.uint32) != np.ascontiguousarray(rows[:, 2:]).view(np.uint32), axis=1))[0]
        assert len(bad) == 0, (name, rows[bad[:5]], got[bad[:5]])
    return names


def test_consumer_on_a_synthesised_dump(tmp_path):
    gx, gy = np.meshgrid(np.arange(65) * 20.0, np.arange(37) * 20.0)
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    for name, (K, D) in U.CAMERAS.items():
        if name == "k1_zero":
            continue
        write_blob(str(tmp_path / ("out_undistort_%s_cam.bin" % name)), 9,
                   list(K) + list(D) + [0.0] * (5 - len(D)) + [len(D)])
        write_blob(str(tmp_path / ("out_undistort_%s.bin" % name)), 8,
                   np.concatenate([pts, U.undistort_points(pts, K, D)], 1))
    assert len(check_dir(str(tmp_path))) == 5
    # a one-ulp difference is caught
    _, _, rows = read_blob(str(tmp_path / "out_undistort_euroc.bin"))
    rows = rows.copy()
    rows[7, 2] = np.nextafter(rows[7, 2], np.float32(np.inf))
    write_blob(str(tmp_path / "out_undistort_euroc.bin"), 8, rows)
    with pytest.raises(AssertionError):
        check_dir(str(tmp_path))


@pytest.mark.skipif(not HAVE, reason="no OpenCV dump under tests/golden/opencv_undistort "
                                     "(see tools/dump_opencv_undistort.cpp)")
def test_restatement_equals_opencv():
    check_dir(DIR)
