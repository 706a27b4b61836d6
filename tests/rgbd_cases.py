"""Inputs of the colour-input and RGB-D tests, synthesised from the committed gray images: a scene is three uint8 planes
(R, G, B) of W x H; `interleave` writes it in any pixel format, so every format of a scene has the same gray image and
one oracle extraction serves them all."""
import functools
import os

import numpy as np

import rgbd_ref as R

W, H, NF = 333, 251, 300  # width a multiple of neither 4 nor 16; rows of 3-byte pixels start at odd addresses
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# TUM-like camera for the test size; BF = fx * 0.16 m
FX, FY, CX, CY, BF = 250.0, 250.0, 166.5, 125.5, 40.0


def _textured(gray, seed):
    """channels = the gray image, and rolled / scaled copies of it plus noise: texture survives the conversion"""
    rng = np.random.default_rng(seed)
    g = gray.astype(np.float32)
    r = g
    gg = np.roll(g, 1, axis=1) * 0.8 + rng.integers(-6, 7, g.shape)
    b = np.roll(g, 1, axis=0) * 1.15 + 20 + rng.integers(-6, 7, g.shape)
    return tuple(np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (r, gg, b))


def _structured():
    """every channel swept through 0..255 against 0 and 255 in the two others, in bands of rows"""
    planes = np.zeros((3, H, W), np.uint8)
    sweep = (np.arange(W) * 255 // (W - 1)).astype(np.uint8)
    bands = [(c, a, b) for c in range(3) for a in (0, 255) for b in (0, 255)]
    for y in range(H):
        c, a, b = bands[y * len(bands) // H]
        o = [k for k in range(3) if k != c]
        planes[c, y], planes[o[0], y], planes[o[1], y] = sweep, a, b
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (R, G, B) planes"""
    z = np.load(os.path.join(GOLDEN, "real_images.npz"))
    out = {}
    for i, (name, src, x0, y0) in enumerate((("hut1", "hut1", 200, 100), ("hut2", "hut2", 203, 101), ("hut3", "hut3", 150, 60),
                                             ("lenna", "lenna", 90, 130), ("lenna2", "lenna", 170, 20))):
        out[name] = _textured(z[src][y0:y0 + H, x0:x0 + W], 11 + i)
    rng = np.random.default_rng(5)
    out["random"] = tuple(rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3))
    out["structured"] = _structured()
    return out


def black():
    return tuple(np.zeros((H, W), np.uint8) for _ in range(3))


def interleave(planes, fmt, seed=0):
    """H x W x bpp uint8 in the byte order of `fmt`; alpha is noise"""
    r, g, b = planes
    ch = [r, g, b] if fmt in (R.PIX_RGB8, R.PIX_RGBA8) else [b, g, r]
    if R.BPP[fmt] == 4:
        ch.append(np.random.default_rng(100 + seed).integers(0, 256, r.shape, dtype=np.uint8))
    return np.ascontiguousarray(np.stack(ch, axis=2))


def gray_of(planes, shift=15):
    return R.cvt_gray(interleave(planes, R.PIX_RGB8), R.PIX_RGB8, shift)


def _cells():
    """32 x 32 px cells: kinds 0, 1, 2 reject (zero / NaN / negative in float images), 3..5 keep the ramp"""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx // 32) + 2 * (yy // 32)) % 6


def depth_u16():
    """a smooth ramp in 500..60000 with blocks of zeros"""
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 500 + (59500 * (xx + 2 * yy)) // (W - 1 + 2 * (H - 1))
    return np.where(_cells() < 3, 0, ramp).astype(np.uint16)


def depth_f32():
    """the same in metres (DepthMapFactor 5000) with blocks of zero, NaN and negative samples"""
    k = _cells()
    d = depth_u16().astype(np.float32) / np.float32(5000)
    ramp = (500 + (59500 * (np.mgrid[0:H, 0:W][1] + 2 * np.mgrid[0:H, 0:W][0])) // (W - 1 + 2 * (H - 1))).astype(np.float32)
    d = np.where(k == 1, np.float32(np.nan), np.where(k == 2, -ramp / np.float32(5000), d))
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle(name, shift=15):
    """(keypoints, descriptors, monoIndex) of the oracle's extraction on the scene's gray image (computed once)"""
    from oracle import orbo
    planes = black() if name == "black" else scenes()[name]
    return orbo.Extractor(NF).compute(gray_of(planes, shift))
