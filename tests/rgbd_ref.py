"""CPU reference for the colour-input and RGB-D tests: numpy restatements of

  * cv::cvtColor(src, dst, COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) on CV_8U images (OpenCV's RGB2Gray<uchar>: 16-bit fixed-point
    coefficients, round to nearest, alpha ignored) as Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular call
    it (tracking.cpp:1235-1258, 1290-1303, 1324-1336);
  * cv::Mat::convertTo(CV_32F, mDepthMapFactor) under the condition of tracking.cpp:1305-1306 (CV_16U or CV_32F source,
    zero offset: one float multiplication per sample);
  * Frame::ComputeStereoFromRGBD (frame.cpp:1000-1021).

Everything is integer or np.float32 element-wise arithmetic (IEEE, no contraction), so these are bit-exact references
for k_gray_images and k_rgbd_depth.  The two OpenCV functions are restated from memory of OpenCV 4.x / 3.x, not pinned to a
build: tools/dump_opencv_cvtcolor.cpp + tests/test_opencv_cvtcolor.py settle them where OpenCV is installed.
"""
import numpy as np

PIX_GRAY8, PIX_RGB8, PIX_BGR8, PIX_RGBA8, PIX_BGRA8 = 0, 1, 2, 3, 4
DEPTH_U16, DEPTH_F32 = 0, 1
#: (cr, cg, cb) by gray_shift: OpenCV 4.x (15) and 3.x (14)
COEF = {15: (9798, 19235, 3735), 14: (4899, 9617, 1868)}
BPP = {PIX_GRAY8: 1, PIX_RGB8: 3, PIX_BGR8: 3, PIX_RGBA8: 4, PIX_BGRA8: 4}


def cvt_gray(img, fmt, shift=15):
    """img: H x W x 3 | 4 uint8, interleaved in the order `fmt` names -> H x W uint8"""
    img = np.asarray(img)
    if fmt not in BPP or fmt == PIX_GRAY8 or shift not in COEF:
        raise ValueError("fmt must be a colour PIX_* format and shift 14 or 15")
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != BPP[fmt]:
        raise ValueError("image must be H x W x %d uint8" % BPP[fmt])
    cr, cg, cb = COEF[shift]
    c = img.astype(np.int64)
    r, b = (c[..., 0], c[..., 2]) if fmt in (PIX_RGB8, PIX_RGBA8) else (c[..., 2], c[..., 0])
    return ((r * cr + c[..., 1] * cg + b * cb + (1 << (shift - 1))) >> shift).astype(np.uint8)


def depth_scaled(depth_type, factor):
    """the condition of tracking.cpp:1305: an image that is not float is always converted, a float image only when the
    factor is further than 1e-5 from 1 (a float difference, compared as a double)"""
    f = np.float32(factor)
    return bool(depth_type != DEPTH_F32 or abs(float(np.float32(f - np.float32(1.0)))) > 1e-5)


def depth_to_float(depth, depth_type, factor):
    """the depth image Frame::Frame receives: float32 H x W"""
    depth = np.asarray(depth)
    want = np.float32 if depth_type == DEPTH_F32 else np.uint16
    if depth_type not in (DEPTH_U16, DEPTH_F32) or depth.dtype != want:
        raise ValueError("depth must be uint16 (DEPTH_U16) or float32 (DEPTH_F32)")
    if not depth_scaled(depth_type, factor):
        return depth.copy()
    with np.errstate(all="ignore"):
        return depth.astype(np.float32) * np.float32(factor)


def stereo_from_rgbd(kps, ukps, depthf, bf):
    """Frame::ComputeStereoFromRGBD -> (mvuRight, mvDepth) float32; kps index the depth image, ukps give the x"""
    depthf = np.asarray(depthf, np.float32)
    u = np.trunc(kps["x"]).astype(np.int64)  # cv::Mat::at<float>(float, float): the arguments convert to int
    v = np.trunc(kps["y"]).astype(np.int64)
    inside = (u >= 0) & (u < depthf.shape[1]) & (v >= 0) & (v < depthf.shape[0])
    d = np.full(len(kps), -1, np.float32)
    d[inside] = depthf[v[inside], u[inside]]
    with np.errstate(all="ignore"):
        ok = d > 0  # false for NaN
        ur = np.asarray(ukps["x"], np.float32) - np.float32(bf) / d
    return np.where(ok, ur, np.float32(-1)).astype(np.float32), np.where(ok, d, np.float32(-1)).astype(np.float32)
