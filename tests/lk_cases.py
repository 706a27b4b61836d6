"""Inputs and cases shared by tests/test_lk_cpu.py, tests/test_gpu_featuretracker.py and tests/golden/make_lk_golden.py:
the 384x256 crops of frames 01-05 of the reference's smooth `hut_long` sequence, the two detector set-ups of the reference's
tracker test (test/src/high_level/test_featuretracker.cpp:53-75) and the tracker cases, each run once through tests/lk_ref.py."""
import functools
import os

import numpy as np

import harris_ref as hr
import lk_ref as lk
from oracle import orbo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CELL, BORDER, DET_MAX_LEVEL = 32, 8, 2
FAST = dict(threshold=10.0, min_arc_length=10, score=1)                                   # :69-71, SUM_OF_ABS_DIFF_ON_ARC
HARRIS = dict(filter_border_type=hr.BORDER_SKIP, use_harris=True, harris_k=0.04, quality_level=0.1)  # :73-75
# the reference's test (:97-102) on the options' defaults: levels 0-4, patches {16,16,16,8,8}, first observation as template
TEST_OPTS = dict(reset_before_detection=False, use_best_n_features=50, min_tracks_to_detect_new_features=15)


@functools.lru_cache(None)
def frames():
    """[5, 256, 384] uint8"""
    return np.load(os.path.join(GOLD, "lk_hut_long.npz"))["frames"]


def dimmed(img):
    """pixels * 0.8 + 10, rounded to nearest and clipped"""
    return np.clip(np.floor(img.astype(np.float64) * 0.8 + 10.5), 0, 255).astype(np.uint8)


def grid(img):
    h, w = img.shape
    return (w + CELL - 1) // CELL, (h + CELL - 1) // CELL


def ref_detector(kind, border=BORDER):
    """the bound detector's raw grid (the callback overload of detect: no threshold step)"""
    if kind == "fast":
        return lambda img: orbo.fg_detect(img, (CELL, CELL), 0, DET_MAX_LEVEL, (border, border), FAST["threshold"], FAST["min_arc_length"],
                                          FAST["score"], 0)
    return lambda img: hr.detect(img, (CELL, CELL), 0, DET_MAX_LEVEL, (border, border), HARRIS["filter_border_type"], HARRIS["use_harris"],
                                 HARRIS["harris_k"], HARRIS["quality_level"], 0)[:3]


def _seq(idx, last=None):
    f = frames()
    out = [f[i] for i in idx]
    if last is not None:
        out[-1] = last(out[-1])
    return out


# name -> (detector, options, the frames)
def cases():
    c = {
        "precompute": ("fast", dict(TEST_OPTS, use_best_n_features=-1), lambda: _seq([0])),
        "step": ("fast", TEST_OPTS, lambda: _seq([0, 1])),
        "seq_harris": ("harris", dict(TEST_OPTS, min_tracks_to_detect_new_features=45), lambda: _seq(range(5))),
        "seq_last_template": ("fast", dict(TEST_OPTS, min_tracks_to_detect_new_features=45, klt_template_is_first_observation=False),
                              lambda: _seq(range(5))),
        "seq_reset": ("fast", dict(TEST_OPTS, min_tracks_to_detect_new_features=45, reset_before_detection=True), lambda: _seq(range(5))),
        "patch32_odd": ("fast", dict(TEST_OPTS, use_best_n_features=49, klt_patch_sizes=(32, 16, 16, 8, 8)), lambda: _seq([0, 2])),
    }
    for off in (False, True):
        for gain in (False, True):
            c["affine_%d%d" % (off, gain)] = ("fast", dict(TEST_OPTS, affine_est_offset=off, affine_est_gain=gain), lambda: _seq([0, 1], dimmed))
    return c


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def summary(tracker, counts):
    """what a case leaves behind, as the integer arrays that go into the golden file"""
    t, f = tracker.track_table(), tracker.feature_table()
    return dict(counts=np.array(counts, np.int32).reshape(-1, 2), first_pos=u32(t["first_pos"]), cur_pos=u32(t["cur_pos"]),
                cur_disparity=u32(t["cur_disparity"]), life=t["life"], track_id=t["track_id"], buffer_id=t["buffer_id"],
                f_px=u32(f["px"]), f_score=u32(f["score"]), f_level=f["level"], f_track_id=f["track_id"],
                disparity=u32(np.array([tracker.book.disparity(0.5)], np.float32)))


def run_case(kind, opts, seq, border=BORDER):
    """one case (detector, options, frames) through the yardstick -> (the lk_ref.Tracker after the last frame, summary,
    per-frame summaries); tests/lk_edge_cases.py runs its table through this too"""
    nc, nr = grid(seq[0])
    T = lk.Tracker(lk.Options(**opts), ref_detector(kind, border), nc, nr, CELL, CELL)
    counts, per_frame = [], []
    for img in seq:
        counts.append(T.track(img))
        per_frame.append(summary(T, counts))
    return T, per_frame[-1], per_frame


@functools.lru_cache(None)
def run_ref(name):
    """-> (the lk_ref.Tracker after the case's last frame, summary, per-frame summaries)"""
    kind, opts, get = cases()[name]
    return run_case(kind, opts, get())


def templates(T):
    """every live track's templates as they lie in the buffers: patches [n, L, max_area] int32, invH [n, L, 10] as words"""
    b = [t.buffer_id for t in T.book.tracks]
    return T.patches[b].copy(), u32(T.invh[b])
