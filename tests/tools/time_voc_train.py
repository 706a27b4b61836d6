#!/usr/bin/env python3
"""Vocabulary::create on the GPU box.  Checks parity with the yardstick tests/voc_train_ref.py on clu3000 first, then trains
clustered sets of N = 100 k, 500 k and 2.27 M descriptors (4541 x 500: the job of the reference's tools/createVoc) at
k = 10, L = 5 and at k = 35, L = 5 (the tool's setting).  Reports the per-phase HIP-event times of
vslam_voc_train_stats, the whole call (host clock around the synchronous call, upload of the descriptors included) and,
for the two smaller N, vslamh_voc_train on one core in the same run.  Every device figure is the second of two calls.
Writes profiles/voc_train_timing.txt (or the path given as the first argument); --quick stops after N = 100 k."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voc_train_cases as cases
import voc_train_ref as ref
import vi_slam_amd as V

args = [a for a in sys.argv[1:] if not a.startswith("--")]
quick = "--quick" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "voc_train_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush():
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


desc, off, kw = cases.inputs("clu3000")
ref.assert_same(V.train_vocabulary(desc, off, **kw), cases.expected("clu3000"), "clu3000")
say("parity with tests/voc_train_ref.py on clu3000: ok")
say("clustered descriptors (N / 50 centres, 24 bit flips each), 500 per document, TF_IDF, seed 1, default rand_mask")
say("ms: seed / assign / mean / partition / weights are HIP-event times of the phases; call = host clock around vslam_voc_train")
H = V.host_lib()
rng = np.random.default_rng(77)
for n in (100000,) if quick else (100000, 500000, 4541 * 500):
    d = cases.clustered_desc(rng, n, n // 50, 24)
    docs = np.arange(0, n + 1, 500, dtype=np.int64)
    if docs[-1] != n:
        docs = np.append(docs, n)
    for k, L in ((10, 5), (35, 5)):
        for rep in range(2):
            t0 = time.perf_counter()
            voc = V.train_vocabulary(d, docs, k=k, L=L, seed=1)
            call = (time.perf_counter() - t0) * 1e3
        s = voc["stats"]
        say("N %8d k %2d L %d: nodes %7d words %7d | passes max %3d total %7d | seed %8.1f assign %8.1f mean %8.1f "
            "partition %8.1f weights %6.1f | call %9.1f ms" % (
                n, k, L, s["nodes"], s["words"], s["max_passes"], s["total_passes"], s["ms_seed"], s["ms_assign"],
                s["ms_mean"], s["ms_partition"], s["ms_weights"], call))
        flush()
        if n <= 500000:
            t0 = time.perf_counter()
            hv = V.train_vocabulary(d, docs, k=k, L=L, seed=1, library=H)
            host = (time.perf_counter() - t0) * 1e3
            same = all(np.array_equal(hv[key], voc[key]) for key in ref.TABLE_KEYS) and \
                np.array_equal(hv["weight"].view(np.uint64), voc["weight"].view(np.uint64))
            say("                      host twin, one core: %10.1f ms (x%.1f of the device call), same vocabulary: %s" % (
                host, host / call, "yes" if same else "NO"))
            flush()
            if not same:
                raise SystemExit("the device and the host twin disagree")
flush()
