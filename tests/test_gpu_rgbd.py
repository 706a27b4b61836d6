"""GPU: colour input images (vslam_fe_set_pixel_format, k_gray_images) and RGB-D frames (vslam_frame_rgbd_batch_async,
k_rgbd_depth) against the numpy restatement of cv::cvtColor, cv::Mat::convertTo and Frame::ComputeStereoFromRGBD
(tests/rgbd_ref.py) and the oracle's extraction on the converted image.  333 x 251 images (width a multiple of neither 4 nor
16, rows at odd addresses), N = 300, contexts of 8 and of 2 slots, source pitches width * bpp and width * bpp + 1."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rgbd_cases as K
import rgbd_ref as R
import undistort_ref as U
import vi_slam_amd as V
from oracle import orbo

pytestmark = pytest.mark.gpu

W, H, NF = K.W, K.H, K.NF
COLOUR = (V.PIX_RGB8, V.PIX_BGR8, V.PIX_RGBA8, V.PIX_BGRA8)
WHERES = (V.IMGS_HOST, V.IMGS_PINNED, V.IMGS_DEVICE, V.IMGS_STAGED)
NAMES = ["hut1", "hut2", "hut3", "lenna", "lenna2", "random", "structured"]
F5000 = float(np.float32(1.0 / 5000.0))
CAM = ((K.FX, K.FY, K.CX, K.CY), U.EUROC_LIKE[1])  # EuRoC-strength distortion, intrinsics for the test size


@pytest.fixture(scope="module")
def fe8():
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=8)
    yield fe
    fe.close()


@pytest.fixture(scope="module")
def fe2():
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2)
    yield fe
    fe.close()


class Buf:
    """images (arrays of H x rowbytes-compatible shape) in pageable, pinned or device memory, rows `pitch` bytes apart"""

    def __init__(self, where, imgs, pad=0):
        n = len(imgs)
        rows = [np.ascontiguousarray(im).view(np.uint8).reshape(im.shape[0], -1) for im in imgs]
        rowb = rows[0].shape[1]
        self.pitch, self.where, self.pin = rowb + pad, where, None
        if where in (V.IMGS_PINNED, V.IMGS_STAGED):
            self.pin = V.PinnedImages(n, rows[0].shape[0], rowb, self.pitch)
            for i in range(n):
                self.pin.array[i][:] = rows[i]
            self.ptrs = [self.pin.ptrs[i] for i in range(n)]
        else:
            a = np.full((n, rows[0].shape[0], self.pitch), 0xA5, np.uint8)
            for i in range(n):
                a[i, :, :rowb] = rows[i]
            if where == V.IMGS_DEVICE:
                self.keep = torch.from_numpy(a).cuda()
                torch.cuda.synchronize()
                self.ptrs = [self.keep[i].data_ptr() for i in range(n)]
            else:
                self.keep = a
                self.ptrs = [a[i].ctypes.data for i in range(n)]

    def fill(self, i, img):
        assert self.pin is not None
        self.pin.array[i][:] = np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)

    def close(self):
        if self.pin is not None:
            self.pin.close()


def _extract(fe, buf, to_host=True):
    if buf.where == V.IMGS_STAGED:
        fe.stage_images_async(buf.ptrs, buf.pitch, V.IMGS_PINNED)
    fe.compute_batch_async(buf.ptrs, buf.pitch, to_host=to_host, where=buf.where)
    return fe.wait(copy=True)


def _same_kps(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in a.dtype.names)


def _check_oracle(res, name, what):
    wk, wd, wm = K.oracle(name)
    k, d, m = res
    assert _same_kps(k, wk) and np.array_equal(d, wd) and m == wm, what


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. level 0
@pytest.mark.parametrize("fmt", COLOUR)
def test_level0_equals_cvt_gray(fe8, fe2, fmt):
    for wi, where in enumerate(WHERES):
        for nb in (1, 2, 3, 5):  # 1, 2: pull route, 32-workgroup grid; 3, 5: DMA staging + the batch grid
            for pad in (0, 1):   # pitch width * bpp and width * bpp + 1, on every route and grid
                fe = fe2 if nb <= 2 else fe8
                fe.set_pixel_format(fmt)
                assert fe.pixel_format == (fmt, 15)
                names = [NAMES[(wi + nb + pad + s) % len(NAMES)] for s in range(nb)]
                buf = Buf(where, [K.interleave(K.scenes()[nm], fmt, seed=s) for s, nm in enumerate(names)], pad=pad)
                try:
                    _extract(fe, buf, to_host=False)
                    for s, nm in enumerate(names):
                        assert np.array_equal(fe.mvImagePyramid(0, s), K.gray_of(K.scenes()[nm])), (fmt, where, nb, pad, s)
                finally:
                    buf.close()


@pytest.mark.parametrize("route", [1, 2])
def test_level0_with_forced_h2d_route(route):
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=4, tuning=dict(h2d_route=route))
    try:
        fe.set_pixel_format(V.PIX_BGR8)
        for nb in (1, 4):
            for where in (V.IMGS_HOST, V.IMGS_PINNED):
                buf = Buf(where, [K.interleave(K.scenes()[NAMES[s]], V.PIX_BGR8) for s in range(nb)], pad=1)
                try:
                    _extract(fe, buf, to_host=False)
                    for s in range(nb):
                        assert np.array_equal(fe.mvImagePyramid(0, s), K.gray_of(K.scenes()[NAMES[s]])), (route, nb, where, s)
                finally:
                    buf.close()
    finally:
        fe.close()


def test_level0_with_gray_shift_14(fe8, fe2):
    for fe, nb in ((fe2, 2), (fe8, 3)):
        fe.set_pixel_format(V.PIX_RGBA8, 14)
        assert fe.pixel_format == (V.PIX_RGBA8, 14)
        buf = Buf(V.IMGS_HOST, [K.interleave(K.scenes()[NAMES[s]], V.PIX_RGBA8) for s in range(nb)])
        _extract(fe, buf, to_host=False)
        for s in range(nb):
            want = K.gray_of(K.scenes()[NAMES[s]], 14)
            assert np.array_equal(fe.mvImagePyramid(0, s), want)
            assert not np.array_equal(want, K.gray_of(K.scenes()[NAMES[s]], 15))
        fe.set_pixel_format(V.PIX_RGBA8)  # shift 0 = the default again


# ---------------------------------------------------------------- 2. extraction
@pytest.mark.parametrize("fmt", [V.PIX_RGB8, V.PIX_BGRA8])
def test_extraction_equals_oracle_on_the_gray_image(fe8, fe2, fmt):
    for fe, names in ((fe2, ["hut1"]), (fe8, ["hut2", "lenna", "hut1", "hut3", "lenna2"])):
        fe.set_pixel_format(fmt)
        for where in (V.IMGS_HOST, V.IMGS_DEVICE):
            buf = Buf(where, [K.interleave(K.scenes()[nm], fmt) for nm in names], pad=1)
            res = _extract(fe, buf)
            for s, nm in enumerate(names):
                _check_oracle(res[s], nm, (fmt, where, s))
    # the synchronous single-image and batch forms over numpy arrays
    fe2.set_pixel_format(fmt)
    _check_oracle(fe2.compute(K.interleave(K.scenes()["lenna"], fmt)), "lenna", "compute")
    res = fe2.compute_batch([K.interleave(K.scenes()[nm], fmt) for nm in ("hut3", "hut1")])
    _check_oracle(res[0], "hut3", "compute_batch")
    _check_oracle(res[1], "hut1", "compute_batch")


def test_stereo_frame_in_bgr8(golden_dir):
    g = np.load(os.path.join(golden_dir, "pipeline_hut_320x240.npz"))
    bf, fx, nf = 40.0, 400.0, 500
    planes = [K._textured(g[k], 3) for k in ("L", "R")]
    gray = [K.gray_of(p) for p in planes]
    eL, eR = orbo.Extractor(nf), orbo.Extractor(nf)
    kL, dL, _ = eL.compute(gray[0])
    kR, dR, _ = eR.compute(gray[1])
    wu, wd, _, _ = orbo.stereo(eL, eR, kL, dL, kR, dR, bf, fx)
    assert (wd > 0).sum() > 50
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, 320, 240, max_batch=2)
    try:
        fe.set_pixel_format(V.PIX_BGR8)
        for where in (V.IMGS_DEVICE, V.IMGS_PINNED):
            buf = Buf(where, [K.interleave(p, V.PIX_BGR8) for p in planes], pad=1)
            try:
                fe.frame_stereo_async(buf.ptrs, buf.pitch, bf, fx, where=where)
                feats, st = fe.frame_stereo_wait()
                assert _same_kps(feats[0][0], kL) and _same_kps(feats[1][0], kR)
                assert np.array_equal(feats[0][1], dL) and np.array_equal(feats[1][1], dR)
                assert np.array_equal(_bits(st[0][0]), _bits(wu)) and np.array_equal(_bits(st[0][1]), _bits(wd)), where
            finally:
                buf.close()
    finally:
        fe.close()


# ---------------------------------------------------------------- 3. graph replay
def test_graph_replay_follows_contents_and_format_changes():
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2)
    plain = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2)
    col = Buf(V.IMGS_PINNED, [K.interleave(K.scenes()[nm], V.PIX_RGB8) for nm in ("hut1", "hut2")])
    gry = Buf(V.IMGS_PINNED, [K.gray_of(K.scenes()[nm]) for nm in ("lenna", "hut3")])
    try:
        fe.set_pixel_format(V.PIX_RGB8)
        for names in (("hut1", "hut2"), ("lenna", "hut3"), ("hut3", "hut1")):  # same pointers: pass 1 captures, 2 and 3 replay
            for s, nm in enumerate(names):
                col.fill(s, K.interleave(K.scenes()[nm], V.PIX_RGB8))
            res = _extract(fe, col)
            for s, nm in enumerate(names):
                _check_oracle(res[s], nm, ("replay", names, s))
        fe.set_pixel_format(V.PIX_GRAY8)
        want = _extract(plain, gry)  # a context that never set a format
        for rep in range(2):
            res = _extract(fe, gry)
            for s, nm in enumerate(("lenna", "hut3")):
                _check_oracle(res[s], nm, ("gray", rep, s))
                assert _same_kps(res[s][0], want[s][0]) and np.array_equal(res[s][1], want[s][1]) and res[s][2] == want[s][2]
        # zero copy is back for device images: level 0 is read from the caller's buffer
        dev = Buf(V.IMGS_DEVICE, [K.gray_of(K.scenes()["hut2"])])
        _check_oracle(_extract(fe, dev)[0], "hut2", "gray device")
        dev.keep[0, :, :W] = torch.from_numpy(K.gray_of(K.scenes()["hut1"])).cuda()
        torch.cuda.synchronize()
        assert np.array_equal(fe.mvImagePyramid(0, 0), K.gray_of(K.scenes()["hut1"]))
        fe.set_pixel_format(V.PIX_BGR8)
        for s, nm in enumerate(("hut3", "hut1")):
            col.fill(s, K.interleave(K.scenes()[nm], V.PIX_BGR8))
        for rep in range(2):
            res = _extract(fe, col)
            for s, nm in enumerate(("hut3", "hut1")):
                _check_oracle(res[s], nm, ("bgr", rep, s))
    finally:
        for b in (col, gry):
            b.close()
        fe.close()
        plain.close()


# ---------------------------------------------------------------- 4. RGB-D
def _depth(kind):
    return (K.depth_u16(), V.DEPTH_U16) if kind == "u16" else (K.depth_f32(), V.DEPTH_F32)


def _rgbd(fe, names, fmt, kind, factor, where, dwhere, to_host=True, depths=None, cam=None, pad=1):
    """one RGB-D pass over the named scenes ("black" = an image without keypoints); checks every output against the
    reference and returns the buffers' owners"""
    d0, dtype = _depth(kind)
    depths = depths if depths is not None else [np.roll(d0, 7 * s, axis=1) for s in range(len(names))]
    planes = [K.black() if nm == "black" else K.scenes()[nm] for nm in names]
    ib = Buf(where, [K.interleave(p, fmt) if fmt != V.PIX_GRAY8 else K.gray_of(p) for p in planes], pad=pad)
    db = Buf(dwhere, depths, pad=depths[0].itemsize * 3)
    try:
        fe.frame_rgbd_async(ib.ptrs, ib.pitch, db.ptrs, db.pitch, dtype, factor, K.BF, to_host=to_host, where=where,
                            depth_where=dwhere)
        feats, st = fe.frame_rgbd_wait()
        for s, nm in enumerate(names):
            wk, wdesc, _ = K.oracle(nm)
            if to_host:
                assert _same_kps(feats[s][0], wk) and np.array_equal(feats[s][1], wdesc), (names, s)
            else:
                assert feats[s][0] == len(wk)
            uk = wk
            if cam is not None:
                uk = U.undistort_keypoints(wk, *cam)
                assert _same_kps(fe.ukeypoints(s), uk)
            wu, wd = R.stereo_from_rgbd(wk, uk, R.depth_to_float(depths[s], dtype, factor), K.BF)
            assert np.array_equal(_bits(st[s][0]), _bits(wu)), (names, kind, factor, where, dwhere, s)
            assert np.array_equal(_bits(st[s][1]), _bits(wd)), (names, kind, factor, where, dwhere, s)
            if nm != "black":
                assert 0.1 * len(wk) <= (wd > 0).sum() <= 0.9 * len(wk)
    finally:
        ib.close()
        db.close()


@pytest.mark.parametrize("kind,factor", [("u16", F5000), ("f32", 1.0), ("f32", float(np.float32(1.0 + 5e-6))), ("f32", 0.5)])
def test_rgbd_equals_reference(fe8, fe2, kind, factor):
    fe8.set_pixel_format(V.PIX_RGB8)
    fe2.set_pixel_format(V.PIX_BGRA8)
    for i, dwhere in enumerate((V.IMGS_HOST, V.IMGS_PINNED, V.IMGS_DEVICE)):
        where = (V.IMGS_PINNED, V.IMGS_DEVICE, V.IMGS_HOST)[i]
        _rgbd(fe8, ["hut1", "black", "lenna"], V.PIX_RGB8, kind, factor, where, dwhere)                    # partial
        _rgbd(fe8, ["hut1", "hut2", "black", "lenna", "hut3", "lenna2", "hut1", "black"], V.PIX_RGB8, kind, factor, where,
              dwhere)                                                                                         # full
        _rgbd(fe2, ["hut2"], V.PIX_BGRA8, kind, factor, where, dwhere)
        _rgbd(fe2, ["black", "hut3"], V.PIX_BGRA8, kind, factor, where, dwhere)


@pytest.mark.parametrize("to_host", [False, True, "deferred"])
def test_rgbd_want_host_forms(fe8, to_host):
    fe8.set_pixel_format(V.PIX_BGR8)
    full = ["hut1", "hut2", "hut3", "lenna", "lenna2", "hut1", "hut2", "hut3"]
    for names in (full, full[:3]):
        for rep in range(2):
            _rgbd(fe8, names, V.PIX_BGR8, "u16", F5000, V.IMGS_HOST, V.IMGS_DEVICE, to_host=to_host)


def test_rgbd_gray_input_and_distorted_camera():
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2)
    try:
        _rgbd(fe, ["hut1", "lenna"], V.PIX_GRAY8, "f32", 1.0, V.IMGS_DEVICE, V.IMGS_DEVICE)
        fe.set_camera(*CAM[0], dist=CAM[1])
        _rgbd(fe, ["hut1", "lenna"], V.PIX_GRAY8, "f32", 1.0, V.IMGS_HOST, V.IMGS_PINNED, cam=CAM)
        fe.set_pixel_format(V.PIX_RGB8)
        _rgbd(fe, ["hut2"], V.PIX_RGB8, "u16", F5000, V.IMGS_PINNED, V.IMGS_HOST, cam=CAM)
        wk = K.oracle("hut1")[0]
        assert np.abs(U.undistort_keypoints(wk, *CAM)["x"] - wk["x"]).max() > 0.5  # mvuRight depends on which x is used
    finally:
        fe.close()


def test_rgbd_same_colour_pointers_other_depth_pointers():
    """the extraction of the second call replays the graph captured by the first; the depth gather must read the second
    call's depth images"""
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=2)
    names = ["hut1", "hut3"]
    ib = Buf(V.IMGS_PINNED, [K.interleave(K.scenes()[nm], V.PIX_RGB8) for nm in names])
    d0 = K.depth_u16()
    sets = [[d0, np.roll(d0, 5, axis=1)], [np.roll(d0, 40, axis=1), np.roll(d0, 64, axis=0)], [np.flipud(d0).copy(), d0]]
    dbs = [Buf(V.IMGS_PINNED, s) for s in sets[:2]] + [Buf(V.IMGS_DEVICE, sets[2])]
    try:
        fe.set_pixel_format(V.PIX_RGB8)
        seen = []
        for db, depths in zip(dbs, sets):
            fe.frame_rgbd_async(ib.ptrs, ib.pitch, db.ptrs, db.pitch, V.DEPTH_U16, F5000, K.BF, where=V.IMGS_PINNED,
                                depth_where=db.where)
            feats, st = fe.frame_rgbd_wait()
            for s, nm in enumerate(names):
                wk = K.oracle(nm)[0]
                assert _same_kps(feats[s][0], wk)
                wu, wd = R.stereo_from_rgbd(wk, wk, R.depth_to_float(depths[s], V.DEPTH_U16, F5000), K.BF)
                assert np.array_equal(_bits(st[s][0]), _bits(wu)) and np.array_equal(_bits(st[s][1]), _bits(wd))
            seen.append(st[0][1].copy())
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    finally:
        for b in [ib] + dbs:
            b.close()
        fe.close()


# ---------------------------------------------------------------- 5. chain
def _dev_read(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_rgbd_chain_unproject_and_search_by_projection(fe2):
    """RGB-D pass of two frames -> UnprojectStereo of both -> SearchByProjection(frame 1, frame 0), all enqueued before
    the first wait; hut2 is hut1's crop moved by (3, 1) px"""
    fe2.set_pixel_format(V.PIX_RGB8)
    names = ["hut1", "hut2"]
    depth = np.full((H, W), 10000, np.uint16)  # 2 m everywhere ...
    depth[:, ::37] = 0                         # ... with a few columns without depth
    ib = Buf(V.IMGS_DEVICE, [K.interleave(K.scenes()[nm], V.PIX_RGB8) for nm in names])
    db = Buf(V.IMGS_DEVICE, [depth, depth])
    z = 2.0
    dx, dy = -3.0 / K.FX * z, -1.0 / K.FY * z  # the image content moves by (-3, -1) px from frame 0 to frame 1
    Twc = [np.hstack([np.eye(3), np.array([[-s * dx], [-s * dy], [0.0]])]).astype(np.float32) for s in range(2)]
    Tcw = [np.hstack([np.eye(3), np.array([[s * dx], [s * dy], [0.0]])]).astype(np.float32) for s in range(2)]
    invfx, invfy = np.float32(1.0) / np.float32(K.FX), np.float32(1.0) / np.float32(K.FY)
    cam = (K.FX, K.FY, K.CX, K.CY, K.BF, K.BF / K.FX)
    fe2.frame_rgbd_async(ib.ptrs, ib.pitch, db.ptrs, db.pitch, V.DEPTH_U16, F5000, K.BF)
    fe2.stereo_points_async(Twc, (K.CX, K.CY, float(invfx), float(invfy)), observations=True)
    m = V.FMatcher(fe2, 0.9, True)
    lk, ld, ln = fe2.slot_dev_ptrs(0)
    ck, cd, cn = fe2.slot_dev_ptrs(1)
    x, f, _, _ = fe2.stereo_points_buffers(0)
    _, _, ur, _ = fe2.stereo_points_buffers(1)
    empty = (np.zeros(0, V.KP_DTYPE), np.zeros(0, np.uint8), np.zeros((0, 3), np.float32), np.zeros((0, 32), np.uint8))
    fwd, bwd = orbo.search_by_projection_frame(Tcw[1], Tcw[0], cam, 15, *empty, np.zeros(0, V.KP_DTYPE),
                                               np.zeros((0, 32), np.uint8), np.zeros(0, np.float32),
                                               fe2.GetScaleFactors(), W, H)[2]
    m.search_by_projection_dev_async([dict(Tcw=Tcw[1], cam=cam[:5], th=15, forward=fwd, backward=bwd, img=(W, H), last_kps=lk,
                                           n_last=ln, last_flags=f, last_x3dw=x, mp_desc=ld, cur_kps=ck, cur_desc=cd,
                                           n_cur=cn, cur_u_right=ur)])
    feats, st = fe2.frame_rgbd_wait()
    out = m.search_by_projection_dev_wait([len(feats[1][0])])
    depthf = R.depth_to_float(depth, V.DEPTH_U16, F5000)
    ref = []
    for s, nm in enumerate(names):
        wk, wdesc, _ = K.oracle(nm)
        assert _same_kps(feats[s][0], wk)
        wu, wd = R.stereo_from_rgbd(wk, wk, depthf, K.BF)
        assert np.array_equal(_bits(st[s][0]), _bits(wu)) and np.array_equal(_bits(st[s][1]), _bits(wd))
        wx, wf = orbo.unproject_stereo(wk, wd, Twc[s], K.CX, K.CY, float(invfx), float(invfy))
        xs, fs, us, ds = fe2.stereo_points_buffers(s)
        gx = _dev_read(xs, fe2.cap * 12).view(np.float32).reshape(fe2.cap, 3)[:len(wk)]
        gf = _dev_read(fs, fe2.cap)[:len(wk)]
        assert np.array_equal(gf, wf * 3) and np.array_equal(gx[wf > 0], wx[wf > 0]) and (wf > 0).sum() > 100, s
        assert np.array_equal(_dev_read(us, len(wk) * 4).view(np.uint32), _bits(wu))
        assert np.array_equal(_dev_read(ds, len(wk) * 4).view(np.uint32), _bits(wd))
        ref.append((wk, wdesc, wu, wx, wf))
    wn, wm, _ = orbo.search_by_projection_frame(Tcw[1], Tcw[0], cam, 15, ref[0][0], ref[0][4] * 3, ref[0][3], ref[0][1],
                                                ref[1][0], ref[1][1], ref[1][2], fe2.GetScaleFactors(), W, H)
    assert out[0][0] == wn and np.array_equal(out[0][1], wm) and wn > 30


def test_rgbd_batch_above_the_unprojection_limit():
    """an RGB-D pass may hold more frames than vslam_stereo_points_dev_async takes pairs (16): all frames deliver
    mvuRight / mvDepth, frames 0..15 can be unprojected, a 17th pair is refused"""
    nfr = 18
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, device=0, max_batch=nfr)
    try:
        fe.set_pixel_format(V.PIX_BGR8)
        names = [("hut1", "lenna", "hut3")[s % 3] for s in range(nfr)]
        _rgbd(fe, names, V.PIX_BGR8, "u16", F5000, V.IMGS_DEVICE, V.IMGS_DEVICE)
        Twc = [np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)] * nfr
        cam = (K.CX, K.CY, float(np.float32(1) / np.float32(K.FX)), float(np.float32(1) / np.float32(K.FY)))
        fe.stereo_points_async(Twc[:16], cam)
        wk = K.oracle(names[15])[0]
        depthf = R.depth_to_float(np.roll(K.depth_u16(), 7 * 15, axis=1), V.DEPTH_U16, F5000)
        _, wd = R.stereo_from_rgbd(wk, wk, depthf, K.BF)
        wx, wf = orbo.unproject_stereo(wk, wd, Twc[0], *cam)
        x, f, _, ds = fe.stereo_points_buffers(15)
        torch.cuda.synchronize()  # the unprojection runs on the context's stream: wait for the device
        gx = _dev_read(x, fe.cap * 12).view(np.float32).reshape(fe.cap, 3)[:len(wk)]
        gf = _dev_read(f, fe.cap)[:len(wk)]
        assert np.array_equal(gf, wf * 3) and np.array_equal(gx[wf > 0], wx[wf > 0])
        assert np.array_equal(_dev_read(ds, len(wk) * 4).view(np.uint32), _bits(wd))
        with pytest.raises(V.VslamError):
            fe.stereo_points_async(Twc[:17], cam)
        with pytest.raises(V.VslamError):
            fe.stereo_points_buffers(16)
    finally:
        fe.close()


def test_rgbd_wait_needs_an_rgbd_pass(fe2):
    """a stereo matcher result on extracted slots is not an RGB-D result"""
    L = V.lib()
    fe2.set_pixel_format(V.PIX_GRAY8)
    res = fe2.compute_batch([K.gray_of(K.scenes()["hut1"])])
    V.ComputeStereoMatches(fe2, 0, fe2, 0, 40.0, 400.0)  # stereo_pairs == last_nimg == 1
    n = (C.c_int * 2)()
    assert L.vslam_frame_rgbd_wait(fe2._h, None, None, fe2.cap, n, None, None) == V.ERR_INVALID
    _rgbd(fe2, ["hut1"], V.PIX_GRAY8, "u16", F5000, V.IMGS_HOST, V.IMGS_DEVICE)
    assert len(res[0][0]) == len(K.oracle("hut1")[0])


# ---------------------------------------------------------------- 6. argument checks
def test_argument_checks_enqueue_nothing(fe2):
    L = V.lib()
    fe2.set_pixel_format(V.PIX_GRAY8)
    before = fe2.pixel_format
    for fmt, shift in ((5, 0), (-1, 0), (V.PIX_RGB8, 13), (V.PIX_RGB8, 1)):
        assert L.vslam_fe_set_pixel_format(fe2._h, fmt, shift) == V.ERR_INVALID
    assert fe2.pixel_format == before
    fe2.set_pixel_format(V.PIX_RGB8)
    ib = Buf(V.IMGS_HOST, [K.interleave(K.scenes()["hut1"], V.PIX_RGB8)] * 3)
    db = Buf(V.IMGS_HOST, [K.depth_u16()] * 3)
    ip, dp = (C.c_void_p * 3)(*ib.ptrs), (C.c_void_p * 3)(*db.ptrs)
    _rgbd(fe2, ["hut3", "hut2"], V.PIX_RGB8, "u16", F5000, V.IMGS_HOST, V.IMGS_HOST)  # the last good pass
    fe2.frame_rgbd_async(ib.ptrs[:1], ib.pitch, db.ptrs[:1], db.pitch, V.DEPTH_U16, F5000, K.BF, where=V.IMGS_HOST,
                         depth_where=V.IMGS_HOST)
    stats = fe2.delivery_stats()

    def call(n=1, pitch=ib.pitch, where=V.IMGS_HOST, d=dp, dpitch=db.pitch, dtype=V.DEPTH_U16, dwhere=V.IMGS_HOST, imgs=ip):
        return L.vslam_frame_rgbd_batch_async(fe2._h, n, imgs, pitch, where, d, dpitch, dtype, dwhere, F5000, K.BF, 1)

    assert call(dtype=2) == V.ERR_INVALID and call(dtype=-1) == V.ERR_INVALID         # depth type
    assert call(pitch=W * 3 - 1) == V.ERR_INVALID and call(pitch=W) == V.ERR_INVALID   # pitch below width * bpp
    assert call(d=None) == V.ERR_INVALID                                               # no depth table
    assert call(n=2, d=(C.c_void_p * 2)(db.ptrs[0], None)) == V.ERR_INVALID            # null depth pointer
    assert call(n=3) == V.ERR_INVALID                                                  # nframes > max_batch
    assert call(dpitch=W * 2 - 2) == V.ERR_INVALID and call(dwhere=V.IMGS_STAGED) == V.ERR_INVALID
    assert L.vslam_fe_extract_batch_async(fe2._h, 1, ip, W * 3 - 1, V.IMGS_HOST, 0, 0, 1) == V.ERR_INVALID
    assert L.vslam_fe_stage_images_async(fe2._h, 1, ip, W * 3 - 1, V.IMGS_HOST) == V.ERR_INVALID
    assert L.vslam_frame_stereo_batch_async(fe2._h, 1, ip, W * 3 - 1, V.IMGS_HOST, 40.0, 400.0, 1) == V.ERR_INVALID
    assert fe2.delivery_stats() == stats                                               # nothing was enqueued
    feats, st = fe2.frame_rgbd_wait()                                                  # the pass enqueued before still stands
    assert _same_kps(feats[0][0], K.oracle("hut1")[0])
