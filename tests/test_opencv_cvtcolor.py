"""CPU: settle the restatements of cv::cvtColor (8-bit RGB2Gray) and cv::Mat::convertTo (16U / 32F -> 32F) in
tests/rgbd_ref.py -- the arithmetic of k_gray_images and k_rgbd_depth -- against REAL OpenCV output, IF a maintainer has
produced it (tools/dump_opencv_cvtcolor.cpp -> tests/golden/opencv_cvtcolor/out_*.bin; OpenCV is not in this image).
Without those files the OpenCV comparison is skipped and the restatements stay "OpenCV as recalled".  The consumer
itself always runs: a dump in the tool's format is synthesised from the restatement in a temporary directory and pushed
through the same check."""
import glob
import os
import struct

import numpy as np
import pytest

import rgbd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "opencv_cvtcolor")
HAVE = bool(glob.glob(os.path.join(DIR, "out_cvtcolor_*.bin")))
FMTS = {"rgb": R.PIX_RGB8, "bgr": R.PIX_BGR8, "rgba": R.PIX_RGBA8, "bgra": R.PIX_BGRA8}


def read_blob(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"VSLD"
    kind, nd = struct.unpack_from("<II", raw, 4)
    dims = struct.unpack_from("<%dI" % nd, raw, 12)
    return kind, np.frombuffer(raw[12 + 4 * nd:], np.uint8 if kind == 10 else np.float32).reshape(dims)


def write_blob(path, kind, arr):
    arr = np.ascontiguousarray(arr, np.uint8 if kind == 10 else np.float32)
    with open(path, "wb") as f:
        f.write(b"VSLD" + struct.pack("<II", kind, arr.ndim) + struct.pack("<%dI" % arr.ndim, *arr.shape) + arr.tobytes())


def check_dir(d):
    """every file of the dump equals the restatement bit for bit; returns the gray_shift this OpenCV uses"""
    shifts = set()
    for name, fmt in FMTS.items():
        kind, rows = read_blob(os.path.join(d, "out_cvtcolor_%s.bin" % name))
        assert kind == 10 and rows.shape[1] == R.BPP[fmt] + 1
        px = np.ascontiguousarray(rows[:, :-1]).reshape(1, -1, R.BPP[fmt])
        match = [s for s in (15, 14) if np.array_equal(R.cvt_gray(px, fmt, s)[0], rows[:, -1])]
        assert match, (name, "neither coefficient set reproduces this OpenCV")
        shifts.add(match[0])
    assert len(shifts) == 1, shifts
    for name, dtype in (("u16", R.DEPTH_U16), ("f32", R.DEPTH_F32)):
        kind, rows = read_blob(os.path.join(d, "out_convert_%s.bin" % name))
        assert kind == 11 and rows.shape[1] == 3
        for f in np.unique(rows[:, 1]):
            sel = rows[rows[:, 1] == f]
            src = sel[:, 0].astype(np.uint16) if dtype == R.DEPTH_U16 else np.ascontiguousarray(sel[:, 0])
            assert R.depth_scaled(dtype, f)
            got = R.depth_to_float(src, dtype, f)
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(sel[:, 2]).view(np.uint32)), (name, f)
    return shifts.pop()


def _synthesise(d, shift):
    rng = np.random.default_rng(1)
    for name, fmt in FMTS.items():
        px = rng.integers(0, 256, (1, 50000, R.BPP[fmt]), dtype=np.uint8)
        write_blob(os.path.join(d, "out_cvtcolor_%s.bin" % name), 10,
                   np.concatenate([px[0], R.cvt_gray(px, fmt, shift)[0][:, None]], 1))
    f = np.float32(1.0 / 5000.0)
    u = np.arange(65536, dtype=np.uint16)
    write_blob(os.path.join(d, "out_convert_u16.bin"), 11,
               np.stack([u.astype(np.float32), np.full(65536, f), R.depth_to_float(u, R.DEPTH_U16, f)], 1))
    x = (rng.random(3000) * 17 - 1).astype(np.float32)
    rows = [np.stack([x, np.full(len(x), g, np.float32), R.depth_to_float(x, R.DEPTH_F32, g)], 1)
            for g in (np.float32(0.5), f, np.float32(1.00002))]
    write_blob(os.path.join(d, "out_convert_f32.bin"), 11, np.concatenate(rows))


@pytest.mark.parametrize("shift", [15, 14])
def test_consumer_on_a_synthesised_dump(tmp_path, shift):
    _synthesise(str(tmp_path), shift)
    assert check_dir(str(tmp_path)) == shift
    # one gray value off by one is caught
    p = str(tmp_path / "out_cvtcolor_bgr.bin")
    _, rows = read_blob(p)
    rows = rows.copy()
    rows[7, -1] ^= 1
    write_blob(p, 10, rows)
    with pytest.raises(AssertionError):
        check_dir(str(tmp_path))


def test_one_ulp_in_a_converted_sample_is_caught(tmp_path):
    _synthesise(str(tmp_path), 15)
    p = str(tmp_path / "out_convert_u16.bin")
    _, rows = read_blob(p)
    rows = rows.copy()
    rows[5000, 2] = np.nextafter(rows[5000, 2], np.float32(np.inf))
    write_blob(p, 11, rows)
    with pytest.raises(AssertionError):
        check_dir(str(tmp_path))


@pytest.mark.skipif(not HAVE, reason="no OpenCV dump under tests/golden/opencv_cvtcolor (see tools/dump_opencv_cvtcolor.cpp)")
def test_restatement_equals_opencv():
    shift = check_dir(DIR)
    print("this OpenCV converts with gray_shift", shift)
