"""Pyramid, blurred level and FAST candidate list of every level and every used slot against the CPU oracle, byte for byte and
entry for entry, on the small frames of tests/stage_cases.py, which jointly hit every strip, tail, row-chunk, cell and band
edge of k_blur7_v2, k_fast_cells_v3 and k_fast_bands (asserted on the CPU by tests/test_stage_cases_cpu.py, which also shows
why: most candidates and most blurred bytes reach no keypoint or descriptor).  The oracle's blur is pinned there to a plain
numpy restatement, so the blurred bytes rest on two independent statements of the operation.

Which kernels a context variant reaches (vslam_fe.hip:100, vslam_context.hip:246-247):
  max_batch 1 or 2, no tuning   k_fast_cells_v3, k_blur7_v2 with 8-row chunks, k_pyramid_group (16-row tiles), slots 0 (and 1)
  max_batch 3                   k_fast_bands, k_blur7_v2 with 32-row chunks, k_pyramid_group(_fit), slots 0-2, then 0-1
  max_batch 9                   the same kernels on slots 0-8, k_fast_bands in its image-major order of eight slots and more
  fast_kernel = 4, max_batch 1  k_fast_bands in a context that would take k_fast_cells_v3
  fast_kernel = 3, max_batch 3  k_fast_cells_v3 on slots 0-2 (the context accepts the switch: it is read at launch only)
  blur_rows = R                 k_blur7_v2 with a last chunk of one row, of five rows, and with one chunk on the deep levels
  gauss_taps                    the blur with taps that are not mirror images, in both chunk heights
  FLAG_HOST_OCTREE              the candidate list after it was fetched to the host for DistributeOctTree
  device-resident level 0       blur, FAST and pyramid read level 0 in place through the caller's pitch (not a multiple of 4)
  dense patterns                both FAST kernels with full survivor lists; the ramp overflows k_fast_bands' list, in the first
                                chunk at thresholds 20 / 7 and first at minThFAST at 30 / 10 (446 x 201 and 160 x 69: the case
                                in which the retry once counted on from a stale counter)

Every frame is a geometry that vslam_fe_create accepts (asserted on the CPU), so no combination is expected to be refused; a
refusal is counted, the combination skipped, and the module's last test asserts that no test lost more than a quarter."""
import collections

import numpy as np
import pytest

import vi_slam_amd as V
from oracle import orbo

import stage_cases as S
from stage_compare import Reference, compare_stages

pytestmark = pytest.mark.gpu

ASYM_TAPS = [10, 30, 50, 60, 52, 36, 18]

_refs = {}
_tried = collections.Counter()
_refused = collections.Counter()


def _oracle(f, taps=None):
    return orbo.Extractor(f[4], scale=f[3], nlevels=f[2], ini_th=f[5], min_th=f[6], taps=taps)


def _ref(f, k, taps=None):
    """the oracle's stages of image k of a frame, computed once for all tests"""
    key = (f, k, tuple(taps) if taps else None)
    if key not in _refs:
        _refs[key] = (S.frame_image(f, k), Reference(_oracle(f, taps), S.frame_image(f, k), taps))
    return _refs[key]


def _context(test, f, **kw):
    _tried[test] += 1
    try:
        return V.FExtractor(f[4], f[3], f[2], f[5], f[6], f[0], f[1], **kw)
    except V.VslamError as e:
        if e.code != -5:  # VSLAM_ERR_UNSUPPORTED: the geometry; anything else is a failure
            raise
        _refused[test] += 1
        pytest.skip("vslam_fe_create refuses %s: %s" % (S.frame_id(f), e))


def _run(fe, f, ks, taps=None, tag=""):
    pairs = [_ref(f, k, taps) for k in ks]
    compare_stages(fe, [im for im, _ in pairs], None, taps, refs=[r for _, r in pairs], tag="%s %s" % (S.frame_id(f), tag))


frames = pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)


@frames
def test_one_image_context(f):
    """k_fast_cells_v3 and 8-row blur chunks, which a context of one or two images runs"""
    fe = _context("one", f, max_batch=1)
    try:
        _run(fe, f, [0])
        _run(fe, f, [3], tag="second image")  # nothing of the image before
    finally:
        fe.close()


@frames
def test_batch_of_three_then_a_partial_batch(f):
    """k_fast_bands and 32-row blur chunks on slots 0-2; then two other images on the same context: slots 0 and 1 show
    nothing of the pass before"""
    fe = _context("batch", f, max_batch=3)
    try:
        _run(fe, f, [0, 1, 2], tag="full batch")
        _run(fe, f, [3, 4], tag="partial batch")
    finally:
        fe.close()


@frames
def test_batch_of_nine(f):
    """eight slots and more: k_fast_bands takes its image-major workgroup order (vk_fast_bands: nslots >= 8) and the
    blur's work list wraps around the eight XCD parts with nine slots; every slot is compared"""
    fe = _context("nine", f, max_batch=9)
    try:
        _run(fe, f, list(range(9)), tag="batch of nine")
    finally:
        fe.close()


@pytest.mark.parametrize("batch", [1, 3])
@frames
def test_dense_patterns(f, batch):
    """a wrapping diagonal ramp (nearly every pixel passes the compass pre-test in both polarities: the survivor list of a
    wide band overflows and k_fast_bands sweeps the rows again in halves; asserted on the CPU), three-level noise and a
    3-px checkerboard at the frames' sizes, through k_fast_cells_v3 one after the other and through k_fast_bands as a batch"""
    fe = _context("dense", f, max_batch=batch)
    try:
        if batch == 1:
            for name in S.DENSE:
                _run(fe, f, [name], tag=name)
        else:
            _run(fe, f, S.DENSE, tag="dense batch")
    finally:
        fe.close()


@frames
def test_bands_kernel_in_a_one_image_context(f):
    fe = _context("bands1", f, max_batch=1, tuning=dict(fast_kernel=4))
    try:
        _run(fe, f, [1])
    finally:
        fe.close()


@frames
def test_cells_kernel_in_a_batch_context(f):
    """fast_kernel = 3 with max_batch = 3: the context accepts it (the switch only picks the launch), so k_fast_cells_v3
    fills slots 1 and 2, which no default context makes it do"""
    fe = _context("cells3", f, max_batch=3, tuning=dict(fast_kernel=3))
    try:
        _run(fe, f, [2, 0, 1])
        _run(fe, f, [4], tag="partial batch")
    finally:
        fe.close()


@frames
def test_blur_rows_overrides(f):
    """a last chunk of one row and of five rows on some level, and levels of one chunk (tests/stage_cases.py picks the
    values); two images, so that slot 1 is blurred with them too"""
    for R in sorted(set(S.blur_rows_overrides(f))):
        fe = _context("rows", f, max_batch=2, tuning=dict(blur_rows=R))
        try:
            _run(fe, f, [0, 1], tag="blur_rows=%d" % R)
        finally:
            fe.close()


@pytest.mark.parametrize("batch", [1, 3])
@frames
def test_asymmetric_gauss_taps(f, batch):
    fe = _context("taps", f, max_batch=batch, gauss_taps=ASYM_TAPS)
    try:
        _run(fe, f, list(range(batch)), taps=ASYM_TAPS, tag="asymmetric taps")
    finally:
        fe.close()


@pytest.mark.parametrize("batch", [1, 3])
@frames
def test_host_quadtree_candidates(f, batch):
    """VSLAM_FLAG_HOST_OCTREE: vslam_fe_candidates reads the list that was fetched to the host for the quadtree"""
    fe = _context("host", f, max_batch=batch, flags=V.FLAG_HOST_OCTREE)
    try:
        _run(fe, f, list(range(batch)), tag="host quadtree")
        if batch > 1:
            _run(fe, f, [4, 3], tag="host quadtree, partial batch")
    finally:
        fe.close()


@pytest.mark.parametrize("batch", [2, 3])
@frames
def test_device_resident_level0_with_an_odd_pitch(f, batch):
    """level 0 stays in the caller's buffer: rows w + 1 .. w + 3 bytes apart, whichever is no multiple of 4 and odd or even
    by the frame, with 255 in the padding.  The entry takes any pitch of at least a row (vslam_fe.hip:454), so nothing is
    refused here; a pitch below the row is."""
    import torch
    w, h = f[0], f[1]
    pitch = w + 1 if (w + 1) % 4 else w + 2
    assert pitch % 4 != 0
    pairs = [_ref(f, k) for k in range(batch)]
    dev = torch.full((batch, h, pitch), 255, dtype=torch.uint8, device="cuda")
    for s, (im, _) in enumerate(pairs):
        dev[s, :, :w] = torch.from_numpy(im).cuda()
    torch.cuda.synchronize()
    fe = _context("pitch", f, max_batch=batch)
    try:
        compare_stages(fe, None, None, refs=[r for _, r in pairs], tag="%s pitch %d" % (S.frame_id(f), pitch),
                       device_ptrs=[dev[s].data_ptr() for s in range(batch)], pitch=pitch)
        assert bool((dev[:, :, w:] == 255).all()), "the padding of the caller's buffer was written"
        with pytest.raises(V.VslamError):
            fe.compute_batch(None, device_ptrs=[dev[s].data_ptr() for s in range(batch)], pitch=w - 1)
    finally:
        fe.close()


def test_few_combinations_were_refused():
    """runs last: of the combinations each test above tried, at most a quarter were geometries vslam_fe_create refuses"""
    for test, n in _tried.items():
        assert 4 * _refused[test] <= n, (test, _refused[test], n)
