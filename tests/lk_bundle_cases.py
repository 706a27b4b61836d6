"""Cases shared by tests/test_lk_bundle_cpu.py, tests/test_gpu_featuretracker_bundle.py and tests/test_cpp_lk_bundle.py:
several cameras per tracker object on the 384x256 hut_long crops of tests/lk_cases.py, each run once through
tests/lk_bundle_ref.py.  The properties that make these inputs reach every way a bundle can go wrong are asserted here,
on the yardstick, so that a change of inputs that loses one fails on the CPU."""
import functools

import numpy as np

import lk_bundle_ref as lb
import lk_cases as LC
import lk_ref as lk

# name -> (detector, options, per camera the frame indices of every call; None: a constant image of 128)
CASES = {
    # fwd | blank | rev | hold
    "four": ("harris", dict(LC.TEST_OPTS, min_tracks_to_detect_new_features=45), ([0, 1, 2, 3, 4], None, [4, 3, 2, 1, 0], [1, 1, 2, 3, 3])),
    # fwd | rev, every live track through k_ft_update in every call.  With camera 1 on [4, 3, 2, 1, 0] both cameras detect
    # in the same calls under FAST (calls 0, 2 and 4), so its order is shifted by one: then only camera 1 detects in
    # calls 1 and 3 and only camera 0 in call 2.
    "two_last": ("fast", dict(LC.TEST_OPTS, min_tracks_to_detect_new_features=45, klt_template_is_first_observation=False),
                 ([0, 1, 2, 3, 4], [3, 2, 1, 0, 4])),
}
N_CALLS = 5


def images(name):
    """[call][camera] -> image"""
    f = LC.frames()
    blank = np.full(f[0].shape, 128, np.uint8)
    return [[blank if idx is None else f[idx[k]] for idx in CASES[name][2]] for k in range(N_CALLS)]


def camera_frames(name, camera):
    return [call[camera] for call in images(name)]


@functools.lru_cache(None)
def run_ref(name):
    """-> (the BundleTracker after the last call, per call the list of per-camera summaries, per call [(tracked, detected)])"""
    kind, opts, _ = CASES[name]
    seq = images(name)
    nc, nr = LC.grid(seq[0][0])
    B = lb.BundleTracker(lk.Options(**opts), LC.ref_detector(kind), len(seq[0]), nc, nr, LC.CELL, LC.CELL)
    counts, per_call = [], []
    live_before = []
    for imgs in seq:
        live_before.append([len(T.book.tracks) for T in B.T])
        counts.append(B.track(imgs))
        per_call.append([LC.summary(T, [c[i] for c in counts]) for i, T in enumerate(B.T)])
    _check(name, B, counts, live_before)
    return B, per_call, counts


def _check(name, B, counts, live_before):
    det = [[d > 0 for _, d in call] for call in counts]
    if name == "four":
        # cross-camera wave: camera 0 enters a call with an odd number of live tracks and a later camera has some
        assert any(lb_[0] % 2 == 1 and sum(lb_[1:]) > 0 for lb_ in live_before)
        # empty segment in the middle: camera 1 never has a track, its neighbours do
        assert all(lb_[1] == 0 for lb_ in live_before) and all(c[1] == (0, 0) for c in counts)
        assert any(lb_[0] > 0 and lb_[2] > 0 for lb_ in live_before)
        # partial detection: only camera 2 of the image cameras; cameras 0 and 3 but not 2; none of the image cameras
        # (the blank camera always asks, so hi = 2 then)
        assert any(d == [False, False, True, False] for d in det)
        assert any(d == [True, False, False, True] for d in det)
        assert any(d == [False, False, False, False] for d in det[1:])
        # k_ft_update gets new tracks from some cameras and none from others
        assert sum(1 for d in det[1:] if any(d) and not all(d[i] for i in (0, 2, 3))) >= 3
    else:
        # detection in exactly one of the two cameras in at least one call
        assert any(d[0] != d[1] for d in det)
        # every live track goes through k_ft_update next to new ones
        assert any(t > 0 and d > 0 for call in counts[1:] for t, d in call)
