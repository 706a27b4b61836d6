#!/usr/bin/env python3
"""The Lucas-Kanade feature tracker (vilib::FeatureTrackerGPU's job) on the GPU box: parity with tests/lk_ref.py first,
then vslam_ft_track per call on 752x480 frames resident in HBM with about 50, about 300 and as many live tracks as the grid holds,
the two kernels alone by HIP events, and the bound detector's own detect call on the same frames in the same run as the
yardstick (the CUDA reference cannot run here).  The frames are the fixture's 384x256 crops tiled to 752x480; the camera
swings by (+-2, +-1) px per frame: whole-pixel shifts, so the tracks live on and every call tracks about as many.
Writes profiles/featuretracker_timing.txt.      python tests/tools/time_featuretracker.py [out.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import lk_cases as LC  # noqa: E402
import lk_ref as lk  # noqa: E402
from vi_slam_amd.fastgrid import FASTGPU  # noqa: E402
from vi_slam_amd.featuretracker import FeatureTrackerGPU  # noqa: E402
from vi_slam_amd.harrisgrid import HarrisGPU  # noqa: E402

W, H, PITCH, NF, CALLS, ROUNDS, EVENT_CALLS = 752, 480, 768, 8, 1500, 3, 300
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "featuretracker_timing.txt")

if torch.cuda.device_count() == 0:
    sys.exit("time_featuretracker.py: no GPU; nothing is measured without one")

base = np.tile(LC.frames()[0], (2, 2))
# a swing: offsets 0, 1, 2, 3, 4, 3, 2, 1 steps of (2, 1) px, cut from a margin so that no pixel wraps
frames = [np.ascontiguousarray(base[8 + s:8 + s + H, 8 + 2 * s:8 + 2 * s + W]) for s in (0, 1, 2, 3, 4, 3, 2, 1)]
dev = torch.zeros((NF, H, PITCH), dtype=torch.uint8, device="cuda")
for s in range(NF):
    dev[s, :, :W] = torch.from_numpy(frames[s]).cuda()
torch.cuda.synchronize()
ptrs = [dev[s].data_ptr() for s in range(NF)]
CELLS = ((W + 31) // 32) * ((H + 31) // 32)


def detector(kind):
    if kind == "fast":
        return FASTGPU(W, H, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, **LC.FAST)
    return HarrisGPU(W, H, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, **LC.HARRIS)


def parity(kind, opts, n_frames):
    """the device's track and feature lists against the yardstick's after every frame"""
    det = detector(kind)
    ft = FeatureTrackerGPU(det, **opts)
    T = lk.Tracker(lk.Options(**opts), LC.ref_detector(kind), (W + 31) // 32, (H + 31) // 32)
    try:
        for k in range(n_frames):
            got, want = ft.track(dev_ptr=ptrs[k % NF], pitch=PITCH), T.track(frames[k % NF])
            t, f, rt, rf = ft.tracks(), ft.features(), T.track_table(), T.feature_table()
            same = tuple(got) == tuple(want) and all(np.array_equal(LC.u32(t[a]), LC.u32(rt[a])) for a in ("first_pos", "cur_pos", "cur_disparity")) \
                and all(np.array_equal(t[a], rt[a]) for a in ("life", "track_id", "buffer_id")) \
                and np.array_equal(LC.u32(f["px"]), LC.u32(rf["px"])) and np.array_equal(f["track_id"], rf["track_id"])
            if not same:
                sys.exit("time_featuretracker.py: %s, frame %d: the device's lists differ from tests/lk_ref.py" % (kind, k))
    finally:
        ft.close()
        det.close()


def measure(kind, label, opts):
    det = detector(kind)
    ft = FeatureTrackerGPU(det, **opts)
    try:
        k = 0
        for _ in range(3 * NF):  # warm up: the track count settles
            ft.track(dev_ptr=ptrs[k % NF], pitch=PITCH)
            k += 1
        best, live, tracked, detected = float("inf"), 0, 0, 0
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                a, b = ft.track(dev_ptr=ptrs[k % NF], pitch=PITCH)
                k += 1
                tracked += a
                detected += b
            best = min(best, (time.perf_counter() - t0) / CALLS * 1e3)
        live = len(ft.tracks())
        ft.profile(True)
        ev = np.zeros((EVENT_CALLS, 2))
        for i in range(EVENT_CALLS):
            ft.track(dev_ptr=ptrs[k % NF], pitch=PITCH)
            k += 1
            ev[i] = ft.kernel_ms()
        ft.profile(False)
        t_det = float("inf")
        for _ in range(ROUNDS):  # the bound detector's own call on the same frames: pyramid (2 levels), detect, grid copy
            t0 = time.perf_counter()
            for i in range(CALLS):
                det.detect_batch(dev_ptrs=[ptrs[i % NF]], pitch=PITCH)
            t_det = min(t_det, (time.perf_counter() - t0) / CALLS * 1e3)
        n = ROUNDS * CALLS
        return {"detector": kind, "tracks": label, "capacity": ft.capacity, "live_tracks_at_end": live, "tracked_per_call": round(tracked / n, 1),
                "detected_per_call": round(detected / n, 2), "track_ms_per_call": round(best, 4),
                "k_ft_track_ms": round(float(np.median(ev[:, 0])), 4), "k_ft_update_ms_when_run": round(float(np.median(ev[ev[:, 1] > 0, 1])) if (ev[:, 1] > 0).any() else 0.0, 4),
                "update_runs_per_call": round(float((ev[:, 1] > 0).mean()), 3), "detector_detect_ms_per_call": round(t_det, 4),
                "track_over_detect": round(best / t_det, 3)}
    finally:
        ft.close()
        det.close()


rows = []
for kind in ("fast", "harris"):
    parity(kind, dict(LC.TEST_OPTS), 6)
    rows.append({"parity": kind, "frames": 6, "equal_to_restatement": True})
parity("fast", dict(LC.TEST_OPTS, use_best_n_features=-1, min_tracks_to_detect_new_features=CELLS, klt_template_is_first_observation=False), 4)
rows.append({"parity": "fast, every cell, last observation as template", "frames": 4, "equal_to_restatement": True})
CONFIGS = [("about 50", dict(LC.TEST_OPTS)),                                                           # the reference's test
           ("about 300", dict(LC.TEST_OPTS, use_best_n_features=300, min_tracks_to_detect_new_features=280)),
           # every call updates every track's template (k_ft_update on all of them)
           ("about 300, last observation as template",
            dict(LC.TEST_OPTS, use_best_n_features=300, min_tracks_to_detect_new_features=280, klt_template_is_first_observation=False)),
           # below 2 * cells tracks the detector runs in every call and fills the cells that hold no track
           ("max_ftr_count, detection in every call", dict(LC.TEST_OPTS, use_best_n_features=-1, min_tracks_to_detect_new_features=2 * CELLS))]
for kind in ("harris", "fast"):
    for label, opts in CONFIGS:
        rows.append(measure(kind, label, opts))

with open(OUT, "w") as f:
    f.write("# tests/tools/time_featuretracker.py, 1 x MI355X: vslam_ft_track on device-resident %dx%d frames, one frame per call, host\n"
            "# clock around calls that end in a stream synchronise, best of %d windows of %d calls; kernels alone: median of %d calls\n"
            "# bracketed by HIP events; the detector's own detect call (2 levels) on the same frames in the same run\n"
            % (W, H, ROUNDS, CALLS, EVENT_CALLS))
    for r in rows:
        f.write(json.dumps(r) + "\n")
for r in rows:
    print(json.dumps(r))
