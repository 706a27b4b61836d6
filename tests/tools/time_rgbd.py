#!/usr/bin/env python3
"""Colour input and RGB-D frames on the GPU box: 32 frames of 640 x 480, N = 1000.  Checks its outputs against
tests/rgbd_ref.py and the oracle first, then times
  * one extraction pass for GRAY8 / RGB8 / BGRA8 images in pinned and in device memory,
  * k_gray_images alone against the gray re-pitch k_pull_images alone, both reading HBM with 8 loads per lane in flight
    (what the DMA route launches behind its copy): HIP events on the context's stream around back-to-back launches,
  * an RGB-D pass against the plain extraction pass of the same frames, depth in device and in pinned memory.
Writes profiles/rgbd_colour_timing.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rgbd_ref as R
import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

W, H, NF, B = 640, 480, 1000, 32
WARM, REPS = 5, 30
BF = 40.0
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rgbd_colour_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def colour(gray, fmt, seed):
    rng = np.random.default_rng(seed)
    g = gray.astype(np.float32)
    planes = [g, np.roll(g, 1, 1) * 0.8 + rng.integers(-6, 7, g.shape), np.roll(g, 1, 0) * 1.15 + 20 + rng.integers(-6, 7, g.shape)]
    r, gg, b = (np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in planes)
    ch = [r, gg, b] if fmt in (R.PIX_RGB8, R.PIX_RGBA8) else [b, gg, r]
    if R.BPP[fmt] == 4:
        ch.append(rng.integers(0, 256, g.shape, dtype=np.uint8))
    return np.ascontiguousarray(np.stack(ch, 2))


frames = [synth.make_frame(W, H, step=s) for s in range(B)]
imgs = {V.PIX_GRAY8: frames}
for fmt in (V.PIX_RGB8, V.PIX_BGRA8):
    imgs[fmt] = [colour(f, fmt, s) for s, f in enumerate(frames)]
yy, xx = np.mgrid[0:H, 0:W]
depth = (500 + (59500 * (xx + 2 * yy)) // (W - 1 + 2 * (H - 1))).astype(np.uint16)
depth[((xx // 32) + 2 * (yy // 32)) % 6 < 2] = 0
F5000 = float(np.float32(1.0 / 5000.0))


def buffers(fmt, where):
    bpp = R.BPP[fmt]
    a = np.stack([np.ascontiguousarray(im).reshape(H, W * bpp) for im in imgs[fmt]])
    if where == V.IMGS_DEVICE:
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        return t, [t[i].data_ptr() for i in range(B)], W * bpp
    p = V.PinnedImages(B, H, W * bpp)
    p.array[:] = a
    return p, [p.ptrs[i] for i in range(B)], W * bpp


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, max_batch=B)
# ---- checks before any timing
ref_kps = {}
for fmt in (V.PIX_RGB8, V.PIX_BGRA8):
    fe.set_pixel_format(fmt)
    keep, ptrs, pitch = buffers(fmt, V.IMGS_PINNED)
    fe.compute_batch_async(ptrs, pitch, where=V.IMGS_PINNED)
    res = fe.wait(copy=True)
    for s in range(B):
        want = R.cvt_gray(imgs[fmt][s], fmt)
        assert np.array_equal(fe.mvImagePyramid(0, s), want), ("level 0", fmt, s)
        if s < 2:
            wk, wd, _ = orbo.Extractor(NF).compute(want)
            assert len(wk) == len(res[s][0]) and all(np.array_equal(wk[f], res[s][0][f]) for f in wk.dtype.names)
            assert np.array_equal(wd, res[s][1])
    dk, dptrs, dpitch = buffers(fmt, V.IMGS_DEVICE)
    dd = torch.from_numpy(np.stack([np.roll(depth, 5 * s, 1) for s in range(B)])).cuda()
    torch.cuda.synchronize()
    fe.frame_rgbd_async(dptrs, dpitch, [dd[s].data_ptr() for s in range(B)], W * 2, V.DEPTH_U16, F5000, BF)
    feats, st = fe.frame_rgbd_wait()
    for s in range(B):
        k = feats[s][0]
        assert all(np.array_equal(k[f], res[s][0][f]) for f in k.dtype.names)
        wu, wdep = R.stereo_from_rgbd(k, k, R.depth_to_float(np.roll(depth, 5 * s, 1), R.DEPTH_U16, F5000), BF)
        assert np.array_equal(st[s][0].view(np.uint32), wu.view(np.uint32)) and np.array_equal(st[s][1].view(np.uint32), wdep.view(np.uint32))
    if hasattr(keep, "close"):
        keep.close()
say("checks passed: level 0 == cvt_gray on 32 frames, keypoints == oracle on 2, mvuRight / mvDepth == reference on 32 (RGB8, BGRA8)")

# ---- 1. ms per extraction pass
say("extraction pass, %d frames %d x %d, N = %d: median (min) ms over %d passes" % (B, W, H, NF, REPS))
for where, wname in ((V.IMGS_PINNED, "pinned"), (V.IMGS_DEVICE, "device")):
    for fmt, fname in ((V.PIX_GRAY8, "GRAY8"), (V.PIX_RGB8, "RGB8"), (V.PIX_BGRA8, "BGRA8")):
        fe.set_pixel_format(fmt)
        keep, ptrs, pitch = buffers(fmt, where)

        def one():
            fe.compute_batch_async(ptrs, pitch, where=where)
            fe.wait()
        med, mn = timed(one)
        say("  %-6s %-6s %.3f (%.3f) ms per pass" % (wname, fname, med, mn))
        if hasattr(keep, "close"):
            keep.close()

# ---- 2. the conversion kernel alone against the gray re-pitch kernel alone (sources in HBM, 8 loads per lane in flight)
fk = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, max_batch=B, tuning=dict(h2d_route=1, pull_depth=8, graphs=0))
stream = torch.cuda.ExternalStream(fk.stream())
rates = {}
for fmt, fname, kname in ((V.PIX_GRAY8, "GRAY8", "k_pull_images"), (V.PIX_RGB8, "RGB8", "k_gray_images"),
                          (V.PIX_BGRA8, "BGRA8", "k_gray_images")):
    fk.set_pixel_format(fmt)
    keep, ptrs, pitch = buffers(fmt, V.IMGS_DEVICE)
    arr = (V.C.c_void_p * B)(*ptrs)
    n = 50
    for _ in range(10):
        fk.stage_images_async(arr, pitch, V.IMGS_PINNED)  # the pull route only dereferences the pointers: HBM here
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        e0.record(stream)
        for _ in range(n):
            fk.stage_images_async(arr, pitch, V.IMGS_PINNED)
        e1.record(stream)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / n)
    moved = B * W * H * (R.BPP[fmt] + 1)  # bytes read + bytes written
    rates[fname] = moved / best
    say("  %-14s %-6s alone: %.1f us per launch of %d frames, %.0f bytes moved per us (read + written)"
        % (kname, fname, best, B, moved / best))
for fname in ("RGB8", "BGRA8"):
    say("  %s conversion moves %.2f of the gray re-pitch's bytes per us (expected >= 0.8)" % (fname, rates[fname] / rates["GRAY8"]))
fk.close()

# ---- 3. RGB-D pass against the plain extraction pass of the same frames
fe.set_pixel_format(V.PIX_RGB8)
keep, ptrs, pitch = buffers(V.PIX_RGB8, V.IMGS_DEVICE)
dd = torch.from_numpy(np.stack([np.roll(depth, 5 * s, 1) for s in range(B)])).cuda()
dp = V.PinnedImages(B, H, W * 2)
dp.array[:] = np.stack([np.roll(depth, 5 * s, 1) for s in range(B)]).view(np.uint8).reshape(B, H, W * 2)
torch.cuda.synchronize()


def plain():
    fe.compute_batch_async(ptrs, pitch, where=V.IMGS_DEVICE)
    fe.wait()


base = timed(plain)
say("RGB-D pass (RGB8 device images), median (min) ms: plain extraction %.3f (%.3f)" % base)
gather = {}
for name, dptrs, dwhere in (("device", [dd[s].data_ptr() for s in range(B)], V.IMGS_DEVICE),
                            ("pinned", [dp.ptrs[s] for s in range(B)], V.IMGS_PINNED)):
    def rgbd():
        fe.frame_rgbd_async(ptrs, pitch, dptrs, W * 2, V.DEPTH_U16, F5000, BF, where=V.IMGS_DEVICE, depth_where=dwhere)
        fe.frame_rgbd_wait()
    med, mn = timed(rgbd)
    fe.set_profiling(True)  # HIP events around k_rgbd_depth on the context's stream
    for _ in range(REPS):
        rgbd()
    ms, n = fe.rgbd_profile()
    fe.set_profiling(False)
    gather[name] = 1e3 * ms / n
    say("  depth in %s memory: %.3f (%.3f) ms per pass; k_rgbd_depth alone %.1f us per launch (%d frames, HIP events, mean of %d)"
        % (name, med, mn, gather[name], B, n))
# what an upload of the 32 depth images would cost instead of reading ~1000 samples per frame over the link
up = torch.empty((B, H, W * 2), dtype=torch.uint8, device="cuda")
host = torch.from_numpy(np.ascontiguousarray(dp.array)).pin_memory()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
best = 1e9
for _ in range(5):
    e0.record()
    up.copy_(host, non_blocking=True)
    e1.record()
    e1.synchronize()
    best = min(best, e0.elapsed_time(e1) * 1e3)
say("  uploading the %d pinned depth images first would take %.1f us (one copy, HIP events) + the %.1f us device gather: the "
    "in-place pinned gather is %s" % (B, best, gather["device"], "faster" if gather["pinned"] < best + gather["device"] else
                                      "SLOWER -- an upload variant is left for later"))
dp.close()
fe.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
