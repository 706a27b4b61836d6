"""GPU (-m gpu): batches of 9 to 64 images through the plain API, every returned slot against the oracle, exact.

Everywhere else in the suite max_batch is 1..8 (the bench tests: 32).  Above 8 slots k_fast_bands deals whole images to
XCDs (slot = xk + 8 * sl, guarded by slot >= nslots), the pyramid, blur and descriptor kernels cut their work lists into
eight per-XCD runs, the sdma upload takes one copy for equally spaced sources, and the host side indexes arrays of
VSLAM_MAX_BATCH = 64 entries: slot counts that are not a multiple of 8, the ABI maximum, and calls with fewer images than
the context holds are run here.  Every slot gets a frame of its own, so a swapped or stale slot cannot pass.

The oracle's keypoint counts for these frames (computed on the CPU): synth.make_frame(640, 360, step=0..63) at nf = 600
gives 609 to 612 per frame, make_frame(1241, 376, step=0..63) at nf = 1000 gives 1003 to 1004, the 17 stereo pairs
make_stereo_pair(640, 360, step=0..16) at nf = 600 give 609 to 612 per image and 223 to 277 keypoints with
u_right >= 0 per pair; `_expected` asserts at least nf / 2 per frame before any GPU result is compared."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

pytestmark = pytest.mark.gpu

BF, FX = 386.1448, 718.856
SMALL = (640, 360, 600)
KITTI = (1241, 376, 1000)
THREADS = min(16, os.cpu_count() or 1)
_CACHE = {}


def _expected(geom, steps, right=False):
    """[(frame, (keypoints, descriptors, monoIndex) of the oracle)] for make_frame(step=s), s in steps; made once per module"""
    w, h, nf = geom
    todo = [s for s in steps if (geom, s, right) not in _CACHE]

    def one(s):
        fr = synth.make_frame(w, h, step=s, right=right)
        return fr, orbo.Extractor(nf).compute(fr)
    if todo:
        with ThreadPoolExecutor(THREADS) as pool:
            for s, r in zip(todo, pool.map(one, todo)):
                assert len(r[1][0]) >= nf / 2, (geom, s, len(r[1][0]))
                _CACHE[(geom, s, right)] = r
    return [_CACHE[(geom, s, right)] for s in steps]


def _same(res, want, tag):
    assert len(res) == len(want), tag
    for s, ((k, d, mono), (_, (ko, do, mo))) in enumerate(zip(res, want)):
        assert len(k) == len(ko), (tag, s, len(k), len(ko))
        for f in k.dtype.names:
            assert np.array_equal(k[f], ko[f]), (tag, s, f)
        assert np.array_equal(d, do), (tag, s)
        assert mono == mo, (tag, s)


class _DeviceFrames:
    """frames in HBM, rows padded to a multiple of 128 bytes"""

    def __init__(self, frames):
        import torch
        self.torch = torch
        h, w = frames[0].shape
        self.pitch = (w + 127) & ~127
        self.dev = torch.zeros((len(frames), h, self.pitch), dtype=torch.uint8, device="cuda")
        self.dev[:, :, :w] = torch.from_numpy(np.stack(frames)).cuda()
        torch.cuda.synchronize()
        self.ptrs = [self.dev[s].data_ptr() for s in range(len(frames))]


def _device_and_host(fe, want, tag):
    """one call with device-resident images, then two with host images (the second replays the captured graph)"""
    frames = [fr for fr, _ in want]
    dv = _DeviceFrames(frames)
    _same(fe.compute_batch(None, device_ptrs=dv.ptrs, pitch=dv.pitch), want, tag + " device")
    for rep in range(2):
        _same(fe.compute_batch(frames), want, tag + " host call %d" % rep)


@pytest.mark.parametrize("m,geom", [(9, SMALL), (12, SMALL), (16, SMALL), (17, SMALL), (33, KITTI), (64, KITTI)])
def test_full_batches_between_9_and_64_slots_equal_oracle(m, geom):
    w, h, nf = geom
    want = _expected(geom, range(m))
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, w, h, max_batch=m)
    try:
        _device_and_host(fe, want, "M=%d" % m)
    finally:
        fe.close()


def test_17_pinned_images_equally_and_unequally_spaced():
    """vslam IMGS_PINNED at 17 slots: the images of one PinnedImages block are equally spaced (one sdma copy for all);
    with one buffer of the ring left out they are not (one copy per image).  Each twice: the second call replays the
    captured graph, and must see the new content put into the same buffers."""
    w, h, nf = SMALL
    n = 17
    want = _expected(SMALL, range(n + 1))
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, w, h, max_batch=n)
    pin = V.PinnedImages(n + 1, h, w)
    try:
        for name, idx in (("equally spaced", list(range(n))), ("one buffer skipped", list(range(8)) + list(range(9, n + 1)))):
            ptrs = [pin.ptrs[i] for i in idx]
            gaps = {ptrs[i + 1] - ptrs[i] for i in range(n - 1)}
            assert (len(gaps) == 1) == (name == "equally spaced")
            for rep in range(2):
                now = [want[(j + rep) % (n + 1)] for j in range(n)]  # buffer idx[j] gets another frame on the second call
                for j, i in enumerate(idx):
                    pin.array[i][:] = now[j][0]
                fe.compute_batch_async(ptrs, pin.pitch, (0, 0), where=V.IMGS_PINNED)
                _same(fe.wait(copy=True), now, "pinned %s call %d" % (name, rep))
    finally:
        pin.close()
        fe.close()


def test_one_32_slot_context_through_larger_and_smaller_calls():
    """31, 3, 8, 32, 1, 32 images on ONE context of 32 slots: what a larger or smaller call left behind (slot counts, the
    quadtree's per-slot masks, k_fast_bands switching between dealing by image and by chunk) must not reach the next call.
    Every call gets frames no earlier call put into the same slots."""
    w, h, nf = SMALL
    want = _expected(SMALL, range(64))
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, w, h, max_batch=32)
    try:
        for call, nimg in enumerate((31, 3, 8, 32, 1, 32)):
            now = [want[(s + 11 * call) % 64] for s in range(nimg)]
            _device_and_host(fe, now, "call %d with %d images" % (call, nimg))
    finally:
        fe.close()


def test_17_stereo_pairs_on_a_34_slot_context_equal_oracle():
    """frame_stereo_async / frame_stereo_wait with 34 images (17 pairs), device-resident and pinned (twice: graph replay)"""
    w, h, nf = SMALL
    npairs = 17
    wl, wr = _expected(SMALL, range(npairs)), _expected(SMALL, range(npairs), right=True)
    ref = []
    for j in range(npairs):
        eL, eR = orbo.Extractor(nf), orbo.Extractor(nf)
        kL, dL, _ = eL.compute(wl[j][0])
        kR, dR, _ = eR.compute(wr[j][0])
        u, dep = orbo.stereo(eL, eR, kL, dL, kR, dR, BF, FX)[:2]
        assert (u >= 0).sum() > 0, j
        ref.append((u, dep))
    frames = [w_[j][0] for j in range(npairs) for w_ in (wl, wr)]
    want = [w_[j] for j in range(npairs) for w_ in (wl, wr)]
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, w, h, max_batch=2 * npairs)
    pin = V.PinnedImages(2 * npairs, h, w)
    try:
        dv = _DeviceFrames(frames)
        for s in range(2 * npairs):
            pin.array[s][:] = frames[s]
        for tag, ptrs, pitch, where in (("device", dv.ptrs, dv.pitch, V.IMGS_DEVICE), ("pinned 0", pin.ptrs, pin.pitch, V.IMGS_PINNED),
                                        ("pinned 1", pin.ptrs, pin.pitch, V.IMGS_PINNED)):
            fe.frame_stereo_async(ptrs, pitch, BF, FX, where=where)
            feats, st = fe.frame_stereo_wait()
            # copies: the views die with the context, and a failure is reported after the context has been closed
            feats = [(k.copy(), d.copy()) for k, d in feats]
            st = [(u.copy(), dep.copy()) for u, dep in st]
            assert len(feats) == 2 * npairs and len(st) == npairs
            _same([(k, d, o[1][2]) for (k, d), o in zip(feats, want)], want, "stereo " + tag)
            for j in range(npairs):
                assert np.array_equal(st[j][0], ref[j][0]) and np.array_equal(st[j][1], ref[j][1]), (tag, j)
    finally:
        pin.close()
        fe.close()
