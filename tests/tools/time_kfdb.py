#!/usr/bin/env python3
"""KeyFrameDatabase query on the GPU box: K = 1000 / 4000 / 16000 keyframes x 1 and 32 queries of about 1000 words out of
a vocabulary of 100 000.  Checks the hit lists of the smallest database against tests/kfdb_ref.py bit for bit first, then
times query (upload, kernel, dense result download, host ordering) as wall time per call and the stream part
(vslam_kfdb_query_async until its event) alone.
Writes profiles/kfdb_query_timing.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kfdb_ref as R
import vi_slam_amd as V

NW, WORDS, HOT = 100000, 1000, 30000
WARM, REPS = 3, 20
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kfdb_query_timing.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


rng = np.random.default_rng(5)
fe = V.FExtractor(1000, 1.2, 8, 20, 7, 640, 480)
queries = [R.random_bow(rng, NW, WORDS + int(rng.integers(-100, 100)), hi=HOT) for _ in range(32)]
db = V.KeyFrameDatabase(NW)
ref = R.RefDatabase(NW)
n_added = 0
say("KeyFrameDatabase query, %d-word vocabulary, about %d words per BowVector" % (NW, WORDS))
for K in (1000, 4000, 16000):
    while n_added < K:
        v = R.random_bow(rng, NW, WORDS + int(rng.integers(-300, 300)), hi=HOT)
        db.add(n_added, n_added % 4, v)
        if K == 1000:
            ref.add(n_added, n_added % 4, *v)
        n_added += 1
    if K == 1000:  # parity before any number
        for q, g in zip(queries[:4], db.query(fe, queries[:4])):
            w = ref.hits(q)
            ok = (g["kf"].tolist() == w["kf"].tolist() and np.array_equal(g["words"], w["words"]) and
                  np.array_equal(g["score"].view(np.uint64), w["score"].view(np.uint64)))
            if not ok:
                raise SystemExit("query differs from the reference: nothing timed")
        say("parity with tests/kfdb_ref.py at K = 1000: ok")
    for nq in (1, 32):
        for _ in range(WARM):
            db.query(fe, queries[:nq])
        t = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            db.query(fe, queries[:nq])
            t.append(time.perf_counter() - t0)
        t.sort()
        say("K = %5d  nq = %2d  query wall: median %.3f ms  min %.3f ms  (%.2f us per pair)" % (
            K, nq, 1e3 * t[len(t) // 2], 1e3 * t[0], 1e6 * t[len(t) // 2] / (K * nq)))
db.close()
fe.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
