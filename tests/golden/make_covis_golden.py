"""Writes tests/golden/covis_small.npz from tests/covis_ref.py: the restatement's outputs on the census scenes and on one
small random scene, so that a change of the yardstick itself shows.   python tests/golden/make_covis_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import covis_cases as CC  # noqa: E402


def arrays():
    out = {}

    def put_conn(tag, g, jobs):
        res = [g.connections(j) for j in jobs]
        out[tag + "_head"] = np.array([[r["error"], len(r["counter_kf"]), len(r["ordered_kf"]), r["n_max"], r["kf_max"],
                                        r["n_tracked"]] for r in res], np.int64)
        for f in ("counter_kf", "counter_n", "ordered_kf", "ordered_w"):
            out[tag + "_" + f] = np.array([v for r in res for v in r[f]], np.int64)

    def put_cull(tag, g, jobs):
        out[tag] = np.array([[r["error"], r["n_mps"], r["n_redundant"]] for r in (g.culling(j) for j in jobs)], np.int64)
    ops, jobs = CC.connections_scene()
    put_conn("conn", CC.build(ops), jobs)
    ops, jobs = CC.culling_scene()
    put_cull("cull", CC.build(ops), jobs)
    g = CC.build(CC.random_scene(20, 60, 6, seed=5, n_maps=2))
    g.set_keyframe_bad(7)
    rng = np.random.RandomState(5)
    lists = [[None if v < 0 else int(v) for v in rng.randint(-10, 60, size=40)] for _ in range(6)]
    put_conn("rand_conn", g, [dict(mode=j % 2, self_kf=j, map_id=j % 2, min_obs=j % 4, mp_ids=lists[j]) for j in range(6)])
    put_cull("rand_cull", g, [dict(kf_id=j, mp_ids=lists[j], levels=[(i + j) % 8 for i in range(40)]) for j in range(6)])
    pts = [g.get_point(m) for m in sorted(g.mps)]
    out["rand_points"] = np.array([[m, p[0], int(p[1]), len(p[2])] for m, p in zip(sorted(g.mps), pts)], np.int64)
    out["rand_obs"] = np.array([row for p in pts for row in p[2]], np.int64).reshape(-1, 6)
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "covis_small.npz")
    np.savez_compressed(path, **arrays())
    print("wrote", path)
