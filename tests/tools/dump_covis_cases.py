"""Dumps the covisibility cases as text for tests/tools/covis_host_check.cpp: the mutation sequence with the result of every
call and the points as tests/covis_ref.py has them, and the query cases with the restatement's answers.
    python tests/tools/dump_covis_cases.py OUT_DIR"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import covis_cases as CC  # noqa: E402
import covis_ref as CR  # noqa: E402


def op_line(op, ok):
    args = [int(a) for a in op[1:]]
    return "op %s %d %s" % (op[0], 0 if ok else -1, " ".join(str(a) for a in args))


def point_line(g, m):
    nobs, bad, obs = g.get_point(m)
    return "point %d %d %d %d %s" % (m, nobs, int(bad), len(obs), " ".join(str(v) for row in obs for v in row))


def ids(v):
    return " ".join(str(-1 if m is None else int(m)) for m in v)


def conn_line(g, j):
    r = g.connections(j)
    return "conn %d %d %d %d %d %s | %d %d %d %d %d %s %s %d %s %s" % (
        j["mode"], j["self_kf"], j["map_id"], j["min_obs"], len(j["mp_ids"]), ids(j["mp_ids"]), r["error"], r["kf_max"], r["n_max"],
        r["n_tracked"], len(r["counter_kf"]), ids(r["counter_kf"]), ids(r["counter_n"]), len(r["ordered_kf"]), ids(r["ordered_kf"]),
        ids(r["ordered_w"]))


def cull_line(g, j, th=3):
    r = g.culling(j, th)
    return "cull %d %d %d %s %s | %d %d %d" % (j["kf_id"], th, len(j["mp_ids"]), ids(j["mp_ids"]), ids(j["levels"]), r["error"],
                                               r["n_mps"], r["n_redundant"])


def scene_lines(g, ops):
    lines = []
    for op in ops:
        if op[0] == "add_keyframes":
            for k, m, o in zip(*op[1:]):
                lines.append(op_line(("add_keyframe", k, m, o), True))
        else:
            lines.append(op_line(op, True))
    CC.apply(g, ops)
    return lines


def main(out):
    os.makedirs(out, exist_ok=True)
    g, lines = CR.Graph(), ["create 8"]
    for step, (op, ok) in enumerate(CC.random_mutations(3000, seed=21)):
        lines.append(op_line(op, ok))
        if ok:
            getattr(g, op[0])(*op[1:])
            if op[0] in ("add_observation", "erase_observation", "clear_point") and op[1] in g.mps:
                lines.append(point_line(g, op[1]))
        if step % 50 == 0:
            lines += [point_line(g, m) for m in sorted(g.mps)] + ["size %d %d %d" % g.size()]
    lines.append("stats 1 1")
    open(os.path.join(out, "mutations.txt"), "w").write("\n".join(lines) + "\n")

    ops, jobs = CC.connections_scene()
    g = CR.Graph()
    lines = ["create 16"] + scene_lines(g, ops) + [conn_line(g, j) for j in jobs]
    open(os.path.join(out, "connections.txt"), "w").write("\n".join(lines) + "\n")

    ops, jobs = CC.culling_scene()
    g = CR.Graph()
    lines = ["create 16"] + scene_lines(g, ops) + [cull_line(g, j) for j in jobs] + [cull_line(g, j, 2) for j in jobs]
    open(os.path.join(out, "culling.txt"), "w").write("\n".join(lines) + "\n")

    g = CR.Graph()
    ops = CC.random_scene(70, 400, 9, seed=8, n_maps=2)
    lines = ["create 0"] + scene_lines(g, ops)
    for j in range(12):
        lst = [(j * 31 + i * 7) % 430 - 15 for i in range(150)]
        lst = [None if v < 0 or v >= 400 else v for v in lst]
        lines.append(conn_line(g, dict(mode=j % 2, self_kf=j, map_id=j % 2, min_obs=j % 4, mp_ids=lst)))
        lines.append(cull_line(g, dict(kf_id=j, mp_ids=lst, levels=[(i + j) % 8 for i in range(150)])))
    open(os.path.join(out, "random.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
