"""CPU: pins the numpy reference of the colour conversion and the RGB-D depth step (tests/rgbd_ref.py) with hand-computed
values, and proves that the inputs of tests/test_gpu_rgbd.py (tests/rgbd_cases.py) can tell the variants apart."""
import numpy as np
import pytest

import rgbd_cases as K
import rgbd_ref as R
import undistort_ref as U
import vi_slam_amd as V

COLOUR = (R.PIX_RGB8, R.PIX_BGR8, R.PIX_RGBA8, R.PIX_BGRA8)


def _px(r, g, b, fmt=R.PIX_RGB8, shift=15):
    p = [r, g, b] if fmt in (R.PIX_RGB8, R.PIX_RGBA8) else [b, g, r]
    if R.BPP[fmt] == 4:
        p.append(77)  # alpha: ignored
    return int(R.cvt_gray(np.array([[p]], np.uint8), fmt, shift)[0, 0])


# (r, g, b) -> (gray at shift 15, gray at shift 14), worked out by hand:
#   (100, 150, 200)  15: 979800 + 2885250 + 747000 + 16384 = 4628434 = 141 * 32768 + 8146          -> 141
#                    14: 489900 + 1442550 + 373600 +  8192 = 2314242 = 141 * 16384 + 4098          -> 141
#   (255, 0, 0)      15: 2498490 + 16384 = 2514874 = 76 * 32768 + 24506                            -> 76
#                    14: 1249245 +  8192 = 1257437 = 76 * 16384 + 12253                            -> 76
#   (0, 0, 255)      15: 952425 + 16384 = 968809 = 29 * 32768 + 18537                              -> 29
#                    14: 476340 +  8192 = 484532 = 29 * 16384 + 9396                               -> 29
#   white            15: 255 * 32768 + 16384 = 255 * 32768 + 16384                                 -> 255  (the coefficients sum to 2^shift)
#   black            the rounding term alone: 16384 >> 15 = 0, 8192 >> 14 = 0                      -> 0
# and four on which the two settings disagree (the shift-14 coefficients are not the halved ones: 19235 / 2 = 9617.5 -> 9617,
# 3735 / 2 = 1867.5 -> 1868, so green weighs 1 / 32768 less and blue 1 / 32768 more):
#   (0, 0, 250)      15: 933750 + 16384 = 950134 = 28 * 32768 + 32630                              -> 28
#                    14: 467000 +  8192 = 475192 = 29 * 16384 + 56                                 -> 29
#   (228, 205, 35)   15: 2233944 + 3943175 + 130725 + 16384 = 6324228 = 193 * 32768 + 4            -> 193
#                    14: 1116972 + 1971485 +  65380 +  8192 = 3162029 = 192 * 16384 + 16301        -> 192
#   (167, 46, 233)   15: 1636266 + 884810 + 870255 + 16384 = 3407715 = 103 * 32768 + 32611         -> 103
#                    14:  818133 + 442382 + 435244 +  8192 = 1703951 = 104 * 16384 + 15            -> 104
#   (12, 103, 118)   15: 117576 + 1981205 + 440730 + 16384 = 2555895 = 77 * 32768 + 32759          -> 77
#                    14:  58788 +  990551 + 220424 +  8192 = 1277955 = 78 * 16384 + 3              -> 78
LITERALS = {(100, 150, 200): (141, 141), (255, 0, 0): (76, 76), (0, 0, 255): (29, 29), (255, 255, 255): (255, 255),
            (0, 0, 0): (0, 0), (0, 0, 250): (28, 29), (228, 205, 35): (193, 192), (167, 46, 233): (103, 104),
            (12, 103, 118): (77, 78)}


@pytest.mark.parametrize("fmt", COLOUR)
def test_cvt_gray_hand_computed(fmt):
    for rgb, (g15, g14) in LITERALS.items():
        assert _px(*rgb, fmt=fmt, shift=15) == g15, rgb
        assert _px(*rgb, fmt=fmt, shift=14) == g14, rgb
    assert sum(1 for a, b in LITERALS.values() if a != b) >= 3
    assert sum(R.COEF[15]) == 1 << 15 and sum(R.COEF[14]) == 1 << 14


def test_shift_settings_differ_on_a_quarter_percent_of_random_triples():
    t = np.random.default_rng(0).integers(0, 256, (1000, 1000, 3), dtype=np.uint8)
    a, b = R.cvt_gray(t, R.PIX_RGB8, 15).astype(int), R.cvt_gray(t, R.PIX_RGB8, 14).astype(int)
    frac = float((a != b).mean())
    assert 0.002 < frac < 0.0032 and np.abs(a - b).max() == 1  # 0.26 %


def test_cvt_gray_rejects_what_it_cannot_read():
    img = np.zeros((4, 4, 3), np.uint8)
    for bad in (lambda: R.cvt_gray(img, R.PIX_GRAY8), lambda: R.cvt_gray(img, R.PIX_RGBA8), lambda: R.cvt_gray(img, 7),
                lambda: R.cvt_gray(img, R.PIX_RGB8, 13), lambda: R.cvt_gray(img.astype(np.int32), R.PIX_RGB8)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("name", sorted(K.scenes()))
def test_inputs_tell_shifts_and_channel_orders_apart(name):
    planes = K.scenes()[name]
    assert planes[0].shape == (K.H, K.W)
    assert int((K.gray_of(planes, 15) != K.gray_of(planes, 14)).sum()) >= 50
    rgb = K.interleave(planes, R.PIX_RGB8)
    assert float((R.cvt_gray(rgb, R.PIX_RGB8) != R.cvt_gray(rgb, R.PIX_BGR8)).mean()) > 0.5
    for fmt in COLOUR:  # every format of a scene reads as the same gray image; alpha does not matter
        assert np.array_equal(R.cvt_gray(K.interleave(planes, fmt, seed=fmt), fmt), K.gray_of(planes))


def test_structured_image_sweeps_every_channel_against_both_extremes():
    planes = np.stack(K.scenes()["structured"])
    for c in range(3):
        o = [k for k in range(3) if k != c]
        for a in (0, 255):
            rows = [y for y in range(K.H) if planes[o[0], y, 0] == a and planes[o[1], y, 0] == a and
                    planes[c, y, 0] == 0 and planes[c, y, -1] == 255]
            assert rows and len(np.unique(planes[c, rows[0]])) == 256


def test_depth_conversion_rule():
    f5000 = np.float32(1.0 / 5000.0)
    d16, d32 = K.depth_u16(), K.depth_f32()
    assert d16.dtype == np.uint16 and d32.dtype == np.float32 and d16.shape == d32.shape == (K.H, K.W)
    assert d16[d16 > 0].min() >= 500 and d16.max() <= 60000 and (d16 == 0).mean() > 0.2
    # CV_16U is always converted, even with factor 1 (type != CV_32F): 60000 -> 60000.0f, times 1/5000
    assert R.depth_scaled(R.DEPTH_U16, 1.0) and R.depth_scaled(R.DEPTH_U16, f5000)
    got = R.depth_to_float(d16, R.DEPTH_U16, f5000)
    assert got.dtype == np.float32 and np.array_equal(got, d16.astype(np.float32) * f5000)
    assert R.depth_to_float(np.array([[5000]], np.uint16), R.DEPTH_U16, f5000)[0, 0] == np.float32(5000) * f5000
    # CV_32F: raw for a factor within 1e-5 of 1 (1 + 5e-6 rounds to 1 + 42 ulp = 1.0000050068: |f - 1| = 5.0068e-6), scaled
    # otherwise; the raw samples are values that either multiplication would change
    near = np.float32(1.0 + 5e-6)
    assert near != np.float32(1.0) and abs(float(near - np.float32(1))) < 1e-5
    assert not R.depth_scaled(R.DEPTH_F32, 1.0) and not R.depth_scaled(R.DEPTH_F32, near)
    assert R.depth_scaled(R.DEPTH_F32, 0.5) and R.depth_scaled(R.DEPTH_F32, f5000) and R.depth_scaled(R.DEPTH_F32, 1.00002)
    for f in (1.0, near):
        assert np.array_equal(R.depth_to_float(d32, R.DEPTH_F32, f).view(np.uint32), d32.view(np.uint32))
    valid = d32 > 0
    with np.errstate(all="ignore"):
        assert (d32[valid] * near != d32[valid]).mean() > 0.5 and np.all(d32[valid] * f5000 != d32[valid])
        assert np.array_equal(R.depth_to_float(d32, R.DEPTH_F32, 0.5)[valid], d32[valid] * np.float32(0.5))
    with pytest.raises(ValueError):
        R.depth_to_float(d16, R.DEPTH_F32, 1.0)


def test_stereo_from_rgbd_hand_computed():
    kps = np.zeros(6, V.KP_DTYPE)
    kps["x"] = [1.9, 0.2, 2.0, 1.0, 0.99, 7.0]   # truncation toward zero; the last lies outside
    kps["y"] = [0.7, 1.999, 1.0, 1.5, 0.0, 0.0]
    ukps = kps.copy()
    ukps["x"] += np.float32(0.25)
    depth = np.array([[-2.0, 4.0, 9.0], [0.0, np.nan, 0.5]], np.float32)
    ur, d = R.stereo_from_rgbd(kps, ukps, depth, 40.0)
    assert np.array_equal(d, np.float32([4.0, -1, 0.5, -1, -1, -1]))
    assert np.array_equal(ur, np.float32([np.float32(2.15) - np.float32(10), -1, np.float32(2.25) - np.float32(80), -1, -1, -1]))


@pytest.mark.parametrize("name", ["hut1", "hut2", "lenna"])
def test_depth_images_bite_on_the_oracle_keypoints(name):
    kps, _, _ = K.oracle(name)
    assert len(kps) > 150
    f5000 = np.float32(1.0 / 5000.0)
    for depthf in (R.depth_to_float(K.depth_u16(), R.DEPTH_U16, f5000), K.depth_f32()):
        ur, d = R.stereo_from_rgbd(kps, kps, depthf, K.BF)
        frac = float((d > 0).mean())
        assert 0.1 <= frac <= 0.9, frac
        assert np.all((ur == -1) == (d == -1))
    raw = K.depth_f32()[np.trunc(kps["y"]).astype(int), np.trunc(kps["x"]).astype(int)]
    assert np.isnan(raw).any() and (raw == 0).any() and (raw < 0).any()  # every rejecting kind is hit
    # a distorted camera moves mvuRight but not mvDepth
    cam = (K.FX, K.FY, K.CX, K.CY), U.EUROC_LIKE[1]
    u2, d2 = R.stereo_from_rgbd(kps, U.undistort_keypoints(kps, *cam), K.depth_f32(), K.BF)
    u1, d1 = R.stereo_from_rgbd(kps, kps, K.depth_f32(), K.BF)
    assert np.array_equal(d1, d2) and (u1 != u2).sum() > 0.5 * (d1 > 0).sum()


def test_mirror_argument_checks_need_no_device():
    assert V.check_pixel_format(V.PIX_BGRA8) == (V.PIX_BGRA8, 15) and V.check_pixel_format(V.PIX_RGB8, 14) == (V.PIX_RGB8, 14)
    assert [V.pixel_bytes(f) for f in range(5)] == [1, 3, 3, 4, 4]
    assert (V.PIX_GRAY8, V.PIX_RGB8, V.PIX_BGR8, V.PIX_RGBA8, V.PIX_BGRA8) == \
        (R.PIX_GRAY8, R.PIX_RGB8, R.PIX_BGR8, R.PIX_RGBA8, R.PIX_BGRA8) and (V.DEPTH_U16, V.DEPTH_F32) == (R.DEPTH_U16, R.DEPTH_F32)
    for fmt, shift in ((5, 0), (-1, 0), (V.PIX_RGB8, 13), (V.PIX_RGB8, 16), (V.PIX_GRAY8, 1)):
        with pytest.raises(V.VslamError) as e:
            V.check_pixel_format(fmt, shift)
        assert e.value.code == V.ERR_INVALID
    assert V.check_depth_args(V.DEPTH_U16, 1 / 5000.0)[0] == np.uint16 and V.check_depth_args(V.DEPTH_F32, 1.0)[0] == np.float32
    for dt, f, bf in ((2, 1.0, 40.0), (-1, 1.0, 40.0), (V.DEPTH_F32, float("nan"), 40.0), (V.DEPTH_U16, float("inf"), 40.0),
                      (V.DEPTH_U16, 1.0, float("nan"))):
        with pytest.raises(V.VslamError) as e:
            V.check_depth_args(dt, f, bf)
        assert e.value.code == V.ERR_INVALID
    for s in ("vslam_fe_set_pixel_format", "vslam_fe_get_pixel_format", "vslam_frame_rgbd_batch_async", "vslam_frame_rgbd_wait"):
        assert s in V.ABI_SYMBOLS
