"""The frames of tests/stage_cases.py, on the CPU: they jointly hit every edge class of the blur and FAST kernels (asserted
class by class, so that an edit of the list cannot lose one silently), the oracle's blur equals a plain numpy restatement on
every one of their levels, and the figures that are the reason for the stage-wise GPU tests: how much of what the image
kernels compute never reaches the keypoints and descriptors that the other tests compare.  No GPU.

Run with -s to see which frame and level carries each class, and the blindness figures."""
import os
import re

import numpy as np
import pytest

import stage_cases as S
from oracle import orbo

ASYM_TAPS = [10, 30, 50, 60, 52, 36, 18]  # sum 256, as tests/test_gpu_extract.py has them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ref = {}


def _oracle(f):
    """the oracle after compute() of the frame's image 0 -> (Extractor, keypoints, descriptors)"""
    if f not in _ref:
        e = orbo.Extractor(f[4], scale=f[3], nlevels=f[2], ini_th=f[5], min_th=f[6])
        k, d, _ = e.compute(S.frame_image(f))
        _ref[f] = (e, k, d)
    return _ref[f]


def _levels(f):
    return list(enumerate(S.level_sizes(*f[:4])))


# ---------------------------------------------------------------------------------------------------------------------------
# the restated geometry


@pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)
def test_level_sizes_are_the_extractors(f):
    e = _oracle(f)[0]
    assert [e.level(l).shape[::-1] for l in range(f[2])] == S.level_sizes(*f[:4])
    assert f[0] <= S.MAX_W and f[1] <= S.MAX_H


@pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)
def test_every_frame_is_a_geometry_a_context_accepts_and_has_a_band_plan(f):
    """no combination of tests/test_gpu_stages.py is lost to a refused geometry, and k_fast_bands runs where it is chosen"""
    assert S.accepted(*f[:4])
    assert S.band_plan_ok(S.level_sizes(*f[:4]))


@pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)
def test_every_frame_gets_a_fused_pyramid_plan(f):
    """vslam_fe_create falls back to one launch per level when a group has no plan; the stage-wise tests are meant to see
    k_pyramid_group (contexts of one or two images: every level resident, 16-row tiles) and k_pyramid_group_fit (batches:
    ping-pong tiles of 32 rows)"""
    from test_pyramid_plan_cpu import _plan
    for batch, want in ((1, (16, 0)), (2, (16, 0)), (3, (32, 1)), (9, (32, 1))):
        ng, _, _, shape, _, _, _, _ = _plan(f[0], f[1], batch, -1, -1, nlevels=f[2], scale=f[3])
        assert ng >= 1 and shape[:2] == want, (batch, ng, shape)


def test_accepted_restates_the_known_refusals():
    assert not S.accepted(64, 48, 8, 1.2)     # levels below 40 px
    assert not S.accepted(58, 58, 1, 1.2)     # 40 px and more, but no 30-px cell
    assert not S.accepted(100, 200, 1, 1.2)   # portrait
    assert S.accepted(69, 69, 4, 1.2)


# ---------------------------------------------------------------------------------------------------------------------------
# coverage, class by class


def _where(pred):
    return ["%s level %d (%dx%d)" % (S.frame_id(f), l, lw, lh) for f in S.FRAMES for l, (lw, lh) in _levels(f) if pred(f, l, lw, lh)]


@pytest.mark.parametrize("cls", S.BLUR_WIDTH_CLASSES)
def test_blur_width_class_is_covered(cls):
    hit = _where(lambda f, l, lw, lh: cls in S.blur_width_classes(lw))
    print("blur %-16s %s" % (cls, hit[:3]))
    assert hit, cls


@pytest.mark.parametrize("R", [8, 32])
@pytest.mark.parametrize("cls", S.BLUR_HEIGHT_CLASSES)
def test_blur_height_class_is_covered_for_both_default_chunk_heights(cls, R):
    hit = _where(lambda f, l, lw, lh: cls in S.blur_height_classes(lh, R))
    print("blur R=%-2d %-12s %s" % (R, cls, hit[:3]))
    assert hit, (cls, R)
    assert not _where(lambda f, l, lw, lh: S.BLUR_ONE_CHUNK in S.blur_height_classes(lh, R))  # h >= 40 > R: overrides only


@pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)
def test_blur_rows_overrides_give_one_row_five_rows_and_one_chunk(f):
    r1, r5, rall = S.blur_rows_overrides(f)
    hs = [lh for _, lh in S.level_sizes(*f[:4])]
    assert 8 <= r1 <= 512 and 8 <= r5 <= 512 and 8 <= rall <= 512  # what vslam_fe_create clamps blur_rows to
    assert any(S.last_chunk_rows(h, r1) == 1 and h > r1 for h in hs)
    assert any(S.last_chunk_rows(h, r5) == 5 and h > r5 for h in hs)
    assert any(S.BLUR_ONE_CHUNK in S.blur_height_classes(h, rall) for h in hs)
    print("blur_rows overrides %s: %d (1-row last chunk), %d (5-row), %d (one chunk)" % (S.frame_id(f), r1, r5, rall))


@pytest.mark.parametrize("cls", S.FAST_PLAN_CLASSES)
def test_fast_plan_class_is_covered(cls):
    hit = _where(lambda f, l, lw, lh: cls in S.fast_plan_classes(l, lw, lh))
    print("FAST %-20s %s" % (cls, hit[:3]))
    assert hit, cls


@pytest.mark.parametrize("cls", S.FAST_PATH_CLASSES)
def test_fast_kernel_path_is_covered(cls):
    hit = [S.frame_id(f) for f in S.FRAMES if cls in S.fast_path_classes(f)]
    print("FAST %-46s %s" % (cls, hit[:3]))
    assert hit, cls


def test_the_ramp_overflows_a_band_list_and_the_scenes_do_not():
    """k_fast_bands sweeps a row chunk again, half as many rows at a time, when its survivor list overflows: the dense
    patterns of tests/stage_cases.py are there for that path, which no synthetic scene of the frames takes"""
    hit, scenes = [], 0
    for f in S.FRAMES:
        lds = S.band_lds(S.frame_max_band_rows(f))
        e = orbo.Extractor(f[4], scale=f[3], nlevels=f[2], ini_th=f[5], min_th=f[6])
        e.pyramid_only(S.frame_image(f, "ramp"))
        for l in range(f[2]):
            over = S.band_list_overflows(e.level(l), l, f[5], lds)
            if over:
                hit.append("%s level %d: %d bands, e.g. %d entries for %d" % (S.frame_id(f), l, len(over), over[0][1], over[0][2]))
        ex = _oracle(f)[0]
        scenes += sum(len(S.band_list_overflows(ex.level(l), l, f[5], lds)) for l in range(f[2]))
    print("FAST %s: %s" % (S.FAST_OVERFLOW_CLASS, hit[:4]))
    assert len(hit) >= 3 and scenes == 0


@pytest.mark.parametrize("cls", S.FAST_OVERFLOW_CLASSES)
def test_where_the_first_overflow_of_a_band_list_falls(cls):
    hit = []
    for f in S.FRAMES:
        lds = S.band_lds(S.frame_max_band_rows(f))
        e = orbo.Extractor(f[4], scale=f[3], nlevels=f[2], ini_th=f[5], min_th=f[6])
        e.pyramid_only(S.frame_image(f, "ramp"))
        hit += ["%s level %d" % (S.frame_id(f), l) for l in range(f[2])
                if cls in S.band_overflow_classes(e.level(l), l, f[5], f[6], lds)]
    print("FAST %s: %s" % (cls, hit[:4]))
    assert hit, cls


def test_smallest_segment_is_what_the_search_finds():
    assert S.smallest_segment() == 5 * 9  # interiors of 10 x 18 px: a level of 513 x 273
    cl = S.cells(0, 513, 273)
    assert ((cl[:, 3] - cl[:, 1] - 6).min(), (cl[:, 4] - cl[:, 2] - 6).min()) == (10, 18)


def test_a_min_threshold_cell_lies_beside_an_ini_threshold_cell():
    hit = []
    for f in S.FRAMES:
        e = _oracle(f)[0]
        for l in range(f[2]):
            if S.fast_image_classes(e.level(l), l, f[5]):
                low = S.min_threshold_cells(e.level(l), l, f[5])
                hit.append("%s level %d (%d of %d cells at minThFAST)" % (S.frame_id(f), l, low.sum(), len(low)))
    print("FAST %s: %s" % (S.FAST_IMAGE_CLASS, hit[:4]))
    assert hit


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's blur against plain numpy


def blur7_numpy(img, taps):
    """reflect-101 border, integer row sums with the taps, integer column sums, round half up at 16 fractional bits"""
    h, w = img.shape
    p = np.pad(img.astype(np.int64), 3, mode="reflect")
    rows = sum(int(taps[k]) * p[:, k:k + w] for k in range(7))
    acc = sum(int(taps[k]) * rows[k:k + h, :] for k in range(7))
    return ((acc + 32768) >> 16).astype(np.uint8)


@pytest.mark.parametrize("taps", [None, ASYM_TAPS], ids=["default", "asymmetric"])
@pytest.mark.parametrize("f", S.FRAMES, ids=S.frame_id)
def test_oracle_blur_equals_numpy(f, taps):
    e = _oracle(f)[0]
    t = taps or [18, 34, 48, 56, 48, 34, 18]
    assert sum(t) == 256  # no sum passes 16 bits, no result passes 255: neither of the oracle's clamps acts
    for l in range(f[2]):
        lv = e.level(l)
        want = blur7_numpy(lv, t)
        got = orbo.blur7(lv, taps)
        assert np.array_equal(got, want), (S.frame_id(f), l, np.argwhere(got != want)[:1])
        own = e.level(l, blurred=True)  # only levels with a keypoint are blurred by compute()
        if own is not None and taps is None:
            assert np.array_equal(own, want), (S.frame_id(f), l)


# ---------------------------------------------------------------------------------------------------------------------------
# what the keypoints and descriptors cannot see


def _blindness(f):
    """(candidates, kept, share dropped by the quadtree, share of blurred bytes within 19 px of no kept keypoint)"""
    e = _oracle(f)[0]
    ncand = nkept = nbytes = nseen = 0
    for l in range(f[2]):
        keys = e.level_keys(l)
        ncand += len(e.candidates(l))
        nkept += len(keys)
        lh, lw = e.level(l).shape
        seen = np.zeros((lh, lw), bool)
        for k in keys:
            x, y = int(round(float(k["x"]))), int(round(float(k["y"])))
            seen[max(y - 19, 0):y + 20, max(x - 19, 0):x + 20] = True
        nbytes += lh * lw
        nseen += int(seen.sum())
    return ncand, nkept, 1.0 - nkept / max(ncand, 1), 1.0 - nseen / nbytes


def test_blindness_figures():
    """Most FAST candidates and most blurred bytes of a frame reach no compared output: the reason for comparing stages"""
    rows = [(S.frame_id(f),) + _blindness(f) for f in S.FRAMES]
    for r in rows:
        print("blindness %-30s candidates %5d kept %4d dropped %4.1f %%  blurred bytes read by no descriptor %4.1f %%"
              % (r[0], r[1], r[2], 100 * r[3], 100 * r[4]))
    assert any(r[3] > 0.5 and r[4] > 0.5 for r in rows)  # both on one frame


def _pattern():
    txt = open(os.path.join(ROOT, "include", "vslam_orb_pattern.h")).read()
    body = txt[txt.index("VSLAM_ORB_PATTERN[1024]"):]
    v = [int(t) for t in re.findall(r"-?\d+", body[body.index("{"):body.index("}")])]
    assert len(v) == 1024
    return np.array(v, np.int32).reshape(512, 2)


def _describe(blurred, keys):
    """computeOrbDescriptor (fextractor.cpp:98-138) over level keypoints, with the oracle's own cosf / sinf / cvRound"""
    L = orbo.lib()
    pat = _pattern()
    out = np.zeros((len(keys), 32), np.uint8)
    fpi = np.float32(np.pi / np.float32(180.0))
    for i, k in enumerate(keys):
        ang = np.float32(k["angle"]) * fpi
        a, b = np.float32(L.orbo_cosf(float(ang))), np.float32(L.orbo_sinf(float(ang)))
        cx, cy = L.orbo_cv_round_f(float(k["x"])), L.orbo_cv_round_f(float(k["y"]))
        px, py = pat[:, 0].astype(np.float32), pat[:, 1].astype(np.float32)
        yy = [cy + L.orbo_cv_round_f(float(v)) for v in (px * b + py * a)]
        xx = [cx + L.orbo_cv_round_f(float(v)) for v in (px * a - py * b)]
        v = blurred[yy, xx].astype(np.int32).reshape(256, 2)
        out[i] = np.packbits((v[:, 0] < v[:, 1]).astype(np.uint8).reshape(32, 8), axis=1, bitorder="little")[:, 0]
    return out


def test_a_wrong_byte_in_the_blurred_border_ring_changes_no_descriptor():
    """sensitivity, on the CPU: one corrupted byte in each corner and edge of the outermost ring of a blurred level leaves
    every descriptor as it was, while the stage array differs -- only a comparison of the blurred level itself sees it"""
    f = S.FRAMES[0]
    e, kps, desc = _oracle(f)
    o = 0
    checked = 0
    for l in range(f[2]):
        keys = e.level_keys(l)
        n = len(keys)
        if n == 0:
            continue
        bl = e.level(l, blurred=True)
        assert np.array_equal(_describe(bl, keys), desc[o:o + n]), "the restated descriptor is not the oracle's"
        bad = bl.copy()
        lh, lw = bl.shape
        for y, x in ((0, 0), (0, lw - 1), (lh - 1, 0), (lh - 1, lw - 1), (0, lw // 2), (lh - 1, lw // 2), (lh // 2, 0), (lh // 2, lw - 1)):
            bad[y, x] ^= 0x80
        assert not np.array_equal(bad, bl)
        assert np.array_equal(_describe(bad, keys), desc[o:o + n]), l
        o += n
        checked += 1
    assert o == len(kps) and checked >= 2


def test_dropping_the_weakest_candidate_of_a_cell_changes_no_keypoint():
    """sensitivity, on the CPU: the quadtree keeps the best candidate of a node, so the candidate list without the weakest
    candidate of a crowded cell gives the same keypoints -- only a comparison of the candidate list itself sees it"""
    f = S.FRAMES[0]
    e = _oracle(f)[0]
    quota = e.tables()["quota"]
    shown = 0
    for l in range(f[2]):
        cand, keys = e.candidates(l), e.level_keys(l)
        lh, lw = e.level(l).shape
        if len(cand) < 4 * max(len(keys), 1):
            continue
        args = (S.FAST_BORDER, lw - S.FAST_BORDER, S.FAST_BORDER, lh - S.FAST_BORDER, int(quota[l]))
        base = orbo.distribute_octree(cand, *args)
        # the oracle's own keypoints of the level are this selection, shifted by the border
        assert np.array_equal(base["x"] + S.FAST_BORDER, keys["x"]) and np.array_equal(base["y"] + S.FAST_BORDER, keys["y"])
        assert np.array_equal(base["response"], keys["response"])
        weakest = int(np.argmin(cand["response"]))  # of the level, so of its cell too
        fewer = np.delete(cand, weakest)
        again = orbo.distribute_octree(fewer, *args)
        same = np.array_equal(again, base)
        print("level %d: %d candidates, %d kept; without the weakest candidate the selection is %s"
              % (l, len(cand), len(keys), "the same" if same else "another"))
        shown += same
    assert shown >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison itself: what tests/test_gpu_stages.py relies on to fail


class _OracleBackedContext:
    """stands in for a context: serves the stages of the given References, writable so that a test can spoil one"""

    def __init__(self, refs, nlevels):
        self.nlevels = nlevels
        self.pyr = [[a.copy() for a in r.pyramid] for r in refs]
        self.blur = [[a.copy() for a in r.blurred] for r in refs]
        self.cand = [[a.copy() for a in r.candidates] for r in refs]

    def mvImagePyramid(self, level, slot=0, blurred=False):
        return (self.blur if blurred else self.pyr)[slot][level]

    def candidates(self, level, slot=0):
        return self.cand[slot][level]


def test_the_stage_comparison_names_slot_level_stage_and_position():
    from stage_compare import Reference, stage_differences
    f = S.FRAMES[0]
    e = orbo.Extractor(f[4], scale=f[3], nlevels=f[2], ini_th=f[5], min_th=f[6])
    refs = [Reference(e, S.frame_image(f, k)) for k in range(2)]
    results = [r.result for r in refs]
    assert stage_differences(_OracleBackedContext(refs, f[2]), results, refs) == []

    fe = _OracleBackedContext(refs, f[2])
    lh, lw = fe.blur[1][2].shape
    fe.blur[1][2][lh - 1, lw - 2] ^= 1          # one bit of one byte of the border ring
    fe.pyr[0][7][3, 0] ^= 1
    fe.cand[0][1] = np.delete(fe.cand[0][1], len(fe.cand[0][1]) - 1)   # the last candidate of the last cell is missing
    c = fe.cand[1][0]
    same_y = np.nonzero((c["y"][1:] == c["y"][:-1]) & (c["response"][1:] != c["response"][:-1]))[0]
    i = int(same_y[0])
    c[[i, i + 1]] = c[[i + 1, i]]                # two neighbours in another order
    fe.cand[1][3]["response"][0] += 1            # one response off by one
    d = stage_differences(fe, results, refs, tag="t")
    print("\n".join(d))
    assert len(d) == 5
    assert any(m.startswith("t slot 1 level 2 blur") and "(row %d, column %d)" % (lh - 1, lw - 2) in m for m in d)
    assert any(m.startswith("t slot 0 level 7 pyramid") and "(row 3, column 0)" in m for m in d)
    assert any(m.startswith("t slot 0 level 1 candidates: %d instead of %d" % (len(fe.cand[0][1]), len(refs[0].candidates[1]))) for m in d)
    assert any(m.startswith("t slot 1 level 0 candidates: x differs from entry %d on" % i) for m in d)
    assert any(m.startswith("t slot 1 level 3 candidates: response differs from entry 0 on (1 of") for m in d)
    # ... and the end of the pipeline: a keypoint field, a descriptor bit, the mono index
    k, dd, m = refs[0].result
    k2, d2 = k.copy(), dd.copy()
    k2["angle"][5] += 1
    d2[7, 31] ^= 0x80
    d = stage_differences(_OracleBackedContext(refs, f[2]), [(k2, d2, m + 1), results[1]], refs)
    assert len(d) == 3 and all(x.startswith("slot 0 ") for x in d), d
