#!/usr/bin/env python3
"""The feature tracker over a bundle of C cameras (vslam_ft_track_bundle) on the GPU box: parity with tests/lk_bundle_ref.py
first, then for C = 1, 2, 4, 8, 32 one bundle call against C single-camera trackers called in turn on the same 752x480
device-resident frames in the same run -- the two take turns window by window --, with about 50 and about 300 live tracks
per camera, and the two kernels of the bundle call alone by HIP events.  Frames as in time_featuretracker.py (the fixture
crop tiled, the camera swinging by whole pixels); camera c is c frames ahead of camera 0.
Writes profiles/featuretracker_bundle_timing.txt.      python tests/tools/time_featuretracker_bundle.py [out.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import lk_bundle_ref as lb  # noqa: E402
import lk_cases as LC  # noqa: E402
import lk_ref as lk  # noqa: E402
from vi_slam_amd.featuretracker import FeatureTrackerGPU  # noqa: E402
from vi_slam_amd.harrisgrid import HarrisGPU  # noqa: E402

W, H, PITCH, NF, CALLS, ROUNDS, EVENT_CALLS = 752, 480, 768, 8, 1500, 3, 300
CAMERAS = (1, 2, 4, 8, 32)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "featuretracker_bundle_timing.txt")

if torch.cuda.device_count() == 0:
    sys.exit("time_featuretracker_bundle.py: no GPU; nothing is measured without one")

base = np.tile(LC.frames()[0], (2, 2))
frames = [np.ascontiguousarray(base[8 + s:8 + s + H, 8 + 2 * s:8 + 2 * s + W]) for s in (0, 1, 2, 3, 4, 3, 2, 1)]
dev = torch.zeros((NF, H, PITCH), dtype=torch.uint8, device="cuda")
for s in range(NF):
    dev[s, :, :W] = torch.from_numpy(frames[s]).cuda()
torch.cuda.synchronize()
ptrs = [dev[s].data_ptr() for s in range(NF)]


def detector(max_batch):
    return HarrisGPU(W, H, LC.CELL, LC.CELL, 0, LC.DET_MAX_LEVEL, LC.BORDER, LC.BORDER, max_batch=max_batch, **LC.HARRIS)


def parity(n_cam, opts, n_calls):
    det = detector(n_cam)
    ft = FeatureTrackerGPU(det, cameras=n_cam, **opts)
    B = lb.BundleTracker(lk.Options(**opts), LC.ref_detector("harris"), n_cam, (W + 31) // 32, (H + 31) // 32)
    try:
        for k in range(n_calls):
            got = ft.track_bundle(dev_ptrs=[ptrs[(k + c) % NF] for c in range(n_cam)], pitch=PITCH)
            want = B.track([frames[(k + c) % NF] for c in range(n_cam)])
            same = got == [tuple(x) for x in want]
            for c, T in enumerate(B.T):
                t, f, rt, rf = ft.tracks(c), ft.features(c), T.track_table(), T.feature_table()
                same = same and all(np.array_equal(LC.u32(t[a]), LC.u32(rt[a])) for a in ("first_pos", "cur_pos", "cur_disparity")) \
                    and all(np.array_equal(t[a], rt[a]) for a in ("life", "track_id", "buffer_id")) \
                    and np.array_equal(LC.u32(f["px"]), LC.u32(rf["px"])) and np.array_equal(f["track_id"], rf["track_id"])
            if not same:
                sys.exit("time_featuretracker_bundle.py: %d cameras, call %d: the device's lists differ from tests/lk_bundle_ref.py" % (n_cam, k))
    finally:
        ft.close()
        det.close()


def measure(n_cam, label, opts):
    det = detector(n_cam)
    ft = FeatureTrackerGPU(det, cameras=n_cam, **opts)
    lone_det = [detector(1) for _ in range(n_cam)]
    lone = [FeatureTrackerGPU(d, **opts) for d in lone_det]
    try:
        args = [[ptrs[(k + c) % NF] for c in range(n_cam)] for k in range(NF)]
        k = 0
        for _ in range(3 * NF):  # warm up: the track counts settle
            ft.track_bundle(dev_ptrs=args[k % NF], pitch=PITCH)
            for c in range(n_cam):
                lone[c].track(dev_ptr=args[k % NF][c], pitch=PITCH)
            k += 1
        t_bundle = t_lone = float("inf")
        tracked = 0
        for _ in range(ROUNDS):  # the two take turns window by window
            t0 = time.perf_counter()
            for i in range(CALLS):
                r = ft.track_bundle(dev_ptrs=args[(k + i) % NF], pitch=PITCH)
                tracked += sum(a for a, _ in r)
            t_bundle = min(t_bundle, (time.perf_counter() - t0) / CALLS * 1e3)
            t0 = time.perf_counter()
            for i in range(CALLS):
                a = args[(k + i) % NF]
                for c in range(n_cam):
                    lone[c].track(dev_ptr=a[c], pitch=PITCH)
            t_lone = min(t_lone, (time.perf_counter() - t0) / CALLS * 1e3)
            k += CALLS
        same = all(np.array_equal(LC.u32(ft.tracks(c)["cur_pos"]), LC.u32(lone[c].tracks()["cur_pos"])) for c in range(n_cam))
        ft.profile(True)
        ev = np.zeros((EVENT_CALLS, 2))
        for i in range(EVENT_CALLS):
            ft.track_bundle(dev_ptrs=args[k % NF], pitch=PITCH)
            k += 1
            ev[i] = ft.kernel_ms()
        ft.profile(False)
        return {"cameras": n_cam, "tracks_per_camera": label, "tracked_per_call": round(tracked / (ROUNDS * CALLS), 1),
                "bundle_equals_lone_trackers_at_end": bool(same), "bundle_ms_per_call": round(t_bundle, 4),
                "lone_trackers_ms_per_call": round(t_lone, 4), "bundle_over_lone": round(t_bundle / t_lone, 3),
                "bundle_ms_per_camera": round(t_bundle / n_cam, 4), "k_ft_track_ms": round(float(np.median(ev[:, 0])), 4),
                "k_ft_update_ms_when_run": round(float(np.median(ev[ev[:, 1] > 0, 1])) if (ev[:, 1] > 0).any() else 0.0, 4),
                "update_runs_per_call": round(float((ev[:, 1] > 0).mean()), 3)}
    finally:
        for t in lone + [ft]:
            t.close()
        for d in lone_det + [det]:
            d.close()


rows = []
parity(4, dict(LC.TEST_OPTS, min_tracks_to_detect_new_features=45), 4)
rows.append({"parity": "harris, 4 cameras", "calls": 4, "equal_to_restatement": True})
CONFIGS = [("about 50", dict(LC.TEST_OPTS)),
           ("about 300", dict(LC.TEST_OPTS, use_best_n_features=300, min_tracks_to_detect_new_features=280))]
for label, opts in CONFIGS:
    for n_cam in CAMERAS:
        rows.append(measure(n_cam, label, opts))
        print(json.dumps(rows[-1]), flush=True)

with open(OUT, "w") as f:
    f.write("# tests/tools/time_featuretracker_bundle.py, 1 x MI355X: vslam_ft_track_bundle over C cameras against C single-camera\n"
            "# trackers (vslam_ft_track) called in turn, device-resident %dx%d frames, Harris detector, host clock around calls that\n"
            "# end in a stream synchronise, best of %d windows of %d calls, the two taking turns window by window; kernels of the\n"
            "# bundle call alone: median of %d calls bracketed by HIP events\n" % (W, H, ROUNDS, CALLS, EVENT_CALLS))
    for r in rows:
        f.write(json.dumps(r) + "\n")
