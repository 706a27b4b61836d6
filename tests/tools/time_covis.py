"""Times the covisibility queries at the workload's own shape -- about 500 keyframes of 2000 features, about 60k MapPoints --
after checking parity with tests/covis_ref.py on that scene: UpdateConnections with 1 and with 30 jobs, the vote with 1 job,
KeyFrameCulling with 100 jobs.  Two figures per query, on the same box: the HIP-event spans of the kernels, and the wall
time of the enqueue / wait pair with the upload of a typical dirty set (one new keyframe with 200 observations) against
the host twin on the same data: mean of the rounds with the least and the greatest.
    python tests/tools/time_covis.py [--rounds 20] [--out profiles/covis_timing.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import covis_cases as CC  # noqa: E402
import covis_ref as CR  # noqa: E402
import vi_slam_amd as V  # noqa: E402

N_KF, N_FEAT, N_MP = 500, 2000, 60000


def scene(seed=1):
    """points seen by runs of consecutive keyframes, as along a trajectory; every keyframe ends with about N_FEAT of them"""
    rng = np.random.RandomState(seed)
    run = np.clip(rng.geometric(N_MP / float(N_KF * N_FEAT), size=N_MP), 2, 60)
    first = rng.randint(0, N_KF, size=N_MP)
    ops = [("add_keyframes", np.arange(N_KF), np.zeros(N_KF, np.int32), np.array([CC.key_of(k) for k in range(N_KF)], np.uint64))]
    lists = [[] for _ in range(N_KF)]
    for mp in range(N_MP):
        ops.append(("add_point", mp))
        for k in range(first[mp], min(first[mp] + run[mp], N_KF)):
            if len(lists[k]) < N_FEAT:
                ops.append(("add_observation", mp, k, len(lists[k]), False, int(rng.randint(0, 8)), False))
                lists[k].append(mp)
    return ops, lists


def spread(ts):
    ts = np.array(ts) * 1e3
    return "%.3f ms (%.3f .. %.3f)" % (ts.mean(), ts.min(), ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops, lists = scene()
    t0 = time.perf_counter()
    g, twin, cov = CC.build(ops), CC.build(ops, V.CovisibilityMapHost()), CC.build(ops, V.CovisibilityMap())
    fe = V.FExtractor(500, 1.2, 8, 20, 7, 320, 240, max_batch=1)
    rng = np.random.RandomState(2)
    lines = ["covisibility queries: %d keyframes, %d MapPoints, %d observation entries (built three times in %.1f s)"
             % (cov.size() + (time.perf_counter() - t0,)), "pool: %r" % (cov.stats(),)]
    kfs = [int(k) for k in rng.choice(N_KF, 100, replace=False)]
    conn = lambda ks, mode=CC.CONN: [dict(mode=mode, self_kf=k, map_id=0, min_obs=3, mp_ids=lists[k]) for k in ks]
    cull = [dict(kf_id=k, mp_ids=lists[k], levels=[int(v) for v in rng.randint(0, 8, size=len(lists[k]))]) for k in kfs]
    cases = [("connections, 1 job", "connections", conn(kfs[:1])), ("connections, 30 jobs", "connections", conn(kfs[:30])),
             ("vote, 1 job", "connections", conn(kfs[:1], CC.VOTE)), ("culling, 100 jobs", "culling", cull)]
    # parity first
    for name, kind, jobs in cases:
        if kind == "connections":
            for r, h, j in zip(cov.connections(fe, jobs), twin.connections(jobs), jobs):
                want = g.connections(j)
                CC.same_connections(r, want)
                CC.same_connections(h, want)
        else:
            want = [g.culling(j) for j in jobs]
            assert cov.culling(fe, jobs) == want and twin.culling(jobs) == want
    lines.append("parity with covis_ref on every job of every case: ok")
    next_kf = N_KF
    for name, kind, jobs in cases:
        n = len(jobs)
        arr, keep = (cov._jobs(jobs) if kind == "connections" else cov._cull_jobs(jobs))
        res = ((V._CovisResult if kind == "connections" else V._CovisCullResult) * n)()
        L, H = V.lib(), V.host_lib()
        dev, host = [], []
        fe.set_profiling(True)
        p0 = cov.profile()
        for rnd in range(a.rounds + 2):
            dirty = [("add_keyframe", next_kf, 0, CC.key_of(next_kf))]
            dirty += [("add_observation", int(m), next_kf, i, False, 2, False) for i, m in enumerate(rng.choice(N_MP, 200, replace=False))]
            next_kf += 1
            CC.apply(cov, dirty)
            CC.apply(twin, dirty)
            t = time.perf_counter()
            if kind == "connections":
                rc = L.vslam_covis_connections_async(cov._h, fe._h, n, arr) or L.vslam_covis_connections_wait(cov._h, fe._h, res)
            else:
                rc = L.vslam_covis_culling_async(cov._h, fe._h, n, arr, 3) or L.vslam_covis_culling_wait(cov._h, fe._h, res)
            t1 = time.perf_counter()
            if kind == "connections":
                rh = H.vslamh_covis_connections(twin._h, n, arr, res)
            else:
                rh = H.vslamh_covis_culling(twin._h, n, arr, 3, res)
            t2 = time.perf_counter()
            assert rc == 0 and rh == 0
            if rnd >= 2:  # two warm-up rounds
                dev.append(t1 - t)
                host.append(t2 - t1)
        fe.set_profiling(False)
        p1 = cov.profile()
        k = p1["passes"] - p0["passes"]
        lines.append("%-22s device enqueue+wait %s | host twin %s | kernels: scatter %.1f us, query %.1f us, %.1f KB up per query"
                     % (name, spread(dev), spread(host), (p1["apply_ms"] - p0["apply_ms"]) / k * 1e3,
                        (p1["query_ms"] - p0["query_ms"]) / k * 1e3, (p1["upload_bytes"] - p0["upload_bytes"]) / k / 1024.0))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
