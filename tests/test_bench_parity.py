"""Oracle parity of bench.Pipeline at the bench's own geometry: four contexts in flight, 32 image slots each, stream
priority 2, the FAST gate (mono), the carry buffer, one deferred result transfer per step, and on the pinned route the
chained upload, the staged images and captured-graph replay.  Every workload of bench.WORKLOADS, both input routes,
every step of a run, every slot: keypoints, descriptors and matcher results bit-equal to the CPU oracle.

The Pipeline is driven in-process with a Namespace that carries the defaults of bench.py's parser; the CPU test at the
top reads those defaults out of bench.py's source, so a changed bench default fails here instead of silently moving the
parity test away from the geometry that is benchmarked.

What the ORACLE gives for the frames of each workload (rank 0 of 1, computed on the CPU; asserted below before any GPU
result is looked at):
  workload                                keypoints/slot   per-step total                    smallest job / pair
  kitti00_mono_1241x376_n1000             1003 .. 1004     4425 init matches                 83 matches
  kitti00_mono_1241x376_n2000             2009 .. 2014     8314 init matches                 172 matches
  kitti00_stereo_1241x376_n2000           2009 .. 2014     15167 with u_right >= 0           906 of a pair
  synthetic_stereo_1920x1080_n4000        4006             33716 with u_right >= 0           2071 of a pair
  hut_stereo_752x480_n1200_real           1182 .. 1211     2222 with u_right >= 0            27 of a pair
  kitti00_stereo_track_1241x376_n2000     2009 .. 2014     15167 stereo, 11021 tracked       125 tracked of a job
The first four totals are the figures a reviewer recomputed by hand from bench.py's matches_last_step_rank0; the hut pairs
are (01,02) (03,04) (04,05) cycled over 16 pairs, and (04,05) is the pair with 27.
"""
import argparse
import ast
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import vi_slam_amd as V  # noqa: F401  (the package must import without a GPU)
from oracle import orbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: bench.py's parser defaults for everything Pipeline reads from `args`
BENCH_DEFAULTS = dict(batch=32, inflight=4, stream_priority=2, fast_chain="auto", delivery="single", upload_chain=1,
                      upload_split=0, exchange_chain=True, fast_kernel=-1, wave_prio=-1, force_collective=False, gc=False,
                      stamp_dump="")
ALL_WORKLOADS = ["kitti00_mono_1241x376_n1000", "kitti00_mono_1241x376_n2000", "kitti00_stereo_1241x376_n2000",
                 "synthetic_stereo_1920x1080_n4000", "hut_stereo_752x480_n1200_real", "kitti00_stereo_track_1241x376_n2000"]
#: matches_last_step_rank0 of the four workloads whose figure was recomputed by hand in review (mono: sum of nmatches,
#: stereo: keypoints with u_right >= 0); the other two are this file's own CPU runs of the oracle
STEP_TOTALS = {"kitti00_mono_1241x376_n1000": 4425, "kitti00_mono_1241x376_n2000": 8314,
               "kitti00_stereo_1241x376_n2000": 15167, "synthetic_stereo_1920x1080_n4000": 33716,
               "hut_stereo_752x480_n1200_real": 2222, "kitti00_stereo_track_1241x376_n2000": 15167}
TRACK_TOTAL = 11021  # tracking workload: sum of SearchByProjection's nmatches over the 16 jobs of a step
ORACLE_THREADS = min(16, os.cpu_count() or 1)


# ------------------------------------------------------------------------------------------------ bench defaults (CPU)
def _parser_defaults(path):
    """{dest: default} of every add_argument call in bench.py (the parser is built inside main(), so it is read from
    the source): default= if given, else what argparse itself gives a store_true / store_false / plain option."""
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"):
            continue
        kw = {k.arg: k.value for k in node.keywords}
        flags = [ast.literal_eval(a) for a in node.args]
        dest = ast.literal_eval(kw["dest"]) if "dest" in kw else \
            [f for f in flags if f.startswith("--")][0][2:].replace("-", "_")
        action = ast.literal_eval(kw["action"]) if "action" in kw else "store"
        if "default" in kw:
            out[dest] = ast.literal_eval(kw["default"])
        else:
            out[dest] = {"store_true": False, "store_false": True}.get(action)
    return out


def test_parity_namespace_carries_the_bench_parsers_defaults():
    """every attribute the parity test hands to Pipeline equals bench.py's own default for that option, and Pipeline
    reads no option the Namespace lacks"""
    defaults = _parser_defaults(os.path.join(ROOT, "bench.py"))
    for k, v in BENCH_DEFAULTS.items():
        assert k in defaults, "bench.py has no option %r any more" % k
        assert defaults[k] == v and type(defaults[k]) is type(v), (k, defaults[k], v)
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Pipeline"][0]
    read = {n.attr for n in ast.walk(cls) if isinstance(n, ast.Attribute) and isinstance(n.value, (ast.Name, ast.Attribute))
            and ast.unparse(n.value) in ("args", "self.args")}
    assert read and read <= set(BENCH_DEFAULTS), read - set(BENCH_DEFAULTS)
    import bench
    assert sorted(bench.WORKLOADS) == sorted(ALL_WORKLOADS)
    assert bench.HEADLINE == ALL_WORKLOADS[0]


# ------------------------------------------------------------------------------------------------ the oracle's side
def _kp32(k):
    return np.stack([k[f].astype(np.float32) for f in k.dtype.names], 1)


def _stereo_pair(args):
    L, R, nf, bf, fx = args
    eL, eR = orbo.Extractor(nf), orbo.Extractor(nf)
    kL, dL, _ = eL.compute(L)
    kR, dR, _ = eR.compute(R)
    u, dep = orbo.stereo(eL, eR, kL, dL, kR, dR, bf, fx)[:2]
    return (kL, dL), (kR, dR), u, dep, eL.tables()["scale"]


def oracle_expectation(name, frames):
    """What one step of workload `name` over `frames` (the B host images of the Pipeline, slot order) must deliver, in the
    layout of Pipeline.last_outputs(): {"first": step 0 of a run, "later": every other step}.  Equal frames (the 1080p
    and hut workloads cycle theirs) are extracted once."""
    import bench
    cfg = bench.WORKLOADS[name]
    w, h, nf, B = cfg["w"], cfg["h"], cfg["nf"], len(frames)
    f32 = lambda a: np.asarray(a, np.float32)
    # the first slot that holds the same image (stereo: the same pair of images; hut4 is the right image of one pair and
    # the left one of the next)
    step = 2 if cfg["stereo"] else 1
    key = lambda s: tuple(id(f) for f in frames[s - s % step:s - s % step + step])
    distinct = {}
    for s in range(0, B, step):
        distinct.setdefault(key(s), s)
    first_of = [distinct[key(s)] + s % step for s in range(B)]
    pool = ThreadPoolExecutor(ORACLE_THREADS)
    exp = {}
    try:
        if not cfg["stereo"]:
            def one(s):
                return orbo.Extractor(nf).compute(frames[s], lap=(0, 1000))
            got = dict(zip(distinct.values(), pool.map(one, distinct.values())))
            feats = [got[first_of[s]] for s in range(B)]

            def job(s):
                p, q = feats[(s - 1) % B], feats[s]
                return orbo.search_for_initialization(p[0], p[1], q[0], q[1], w, h, window=100, nnratio=0.9)[:2]
            jobs = list(pool.map(job, range(B)))
            exp["mono_index"] = f32([f[2] for f in feats])
            exp["init_nmatches"] = f32([j[0] for j in jobs])
            exp["init_matches12"] = [f32(j[1]) for j in jobs]
            for s in range(B):
                assert len(jobs[s][1]) == len(feats[(s - 1) % B][0])
        else:
            bf, fx = cfg.get("bf", bench.BF), cfg.get("fx", bench.FX)
            pairs_distinct = sorted(distinct.values())
            got = dict(zip(pairs_distinct, pool.map(_stereo_pair, [(frames[s], frames[s + 1], nf, bf, fx) for s in pairs_distinct])))
            pairs = [got[first_of[2 * j]] for j in range(B // 2)]
            feats = [pairs[s // 2][s & 1] for s in range(B)]
            exp["u_right"] = np.concatenate([f32(p[2]) for p in pairs])
            exp["depth"] = np.concatenate([f32(p[3]) for p in pairs])
            exp["stereo_matched"] = [int((p[2] >= 0).sum()) for p in pairs]
            if cfg.get("track"):
                FX, FY, CX, CY, BF = bench.FX, bench.FY, bench.CX, bench.CY, bench.BF
                T0 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
                Tcw = np.hstack([np.eye(3), np.array([[3.0 / FX * bench.TRACK_Z], [1.0 / FY * bench.TRACK_Z], [0.0]])]).astype(np.float32)
                invfx, invfy = float(np.float32(1.0) / np.float32(FX)), float(np.float32(1.0) / np.float32(FY))
                pts = [orbo.unproject_stereo(p[0][0], p[3], T0, CX, CY, invfx, invfy) for p in pairs]

                def tjob(j):
                    (pk, pd), _, _, _, _ = pairs[j - 1]
                    (ck, cd), _, cu, _, scale = pairs[j]
                    px, pf = pts[j - 1]
                    return orbo.search_by_projection_frame(Tcw, T0, (FX, FY, CX, CY, BF, BF / FX), 15, pk, pf * 3, px, pd,
                                                           ck, cd, cu, scale, w, h)[:2]
                tj = list(pool.map(tjob, range(B // 2)))
                exp["track_nmatches"] = f32([t[0] for t in tj])
                exp["track_matches"] = [f32(t[1]) for t in tj]
                for j in range(B // 2):
                    assert len(tj[j][1]) == len(pairs[j][0][0])
    finally:
        pool.shutdown()
    exp["keypoint_counts"] = f32([len(f[0]) for f in feats])
    exp["keypoints"] = np.concatenate([_kp32(f[0]) for f in feats])
    exp["descriptors"] = np.concatenate([f32(f[1]).reshape(-1, 32) for f in feats])
    # ---- the oracle's own output must make the comparison worth something
    counts = exp["keypoint_counts"]
    assert len(counts) == B and counts.min() >= nf / 2, (name, counts.min())
    if not cfg["stereo"]:
        assert exp["init_nmatches"].min() > 0
        assert int(exp["init_nmatches"].sum()) == STEP_TOTALS[name], (name, int(exp["init_nmatches"].sum()))
    else:
        assert min(exp["stereo_matched"]) > 0
        assert int((exp["u_right"] >= 0).sum()) == sum(exp["stereo_matched"]) == STEP_TOTALS[name], \
            (name, int((exp["u_right"] >= 0).sum()))
        if cfg.get("track"):
            assert exp["track_nmatches"].min() > 0
            assert int(exp["track_nmatches"].sum()) == TRACK_TOTAL, int(exp["track_nmatches"].sum())
    # ---- step 0 of a run has no job for slot 0 / pair 0 (no previous step); every later step has all of them
    later = {k: (np.concatenate(v) if isinstance(v, list) else v) for k, v in exp.items() if k != "stereo_matched"}
    first = dict(later)
    for nk, mk in (("init_nmatches", "init_matches12"), ("track_nmatches", "track_matches")):
        if nk in exp:
            first[nk] = exp[nk][1:]
            first[mk] = np.concatenate(exp[mk][1:])
    return {"first": first, "later": later, "counts": counts.astype(int)}


_EXPECTED = {}


def expectation_for(name, frames):
    """the oracle runs once per workload and module (a Pipeline's frames are the same at every step and for both routes)"""
    if name not in _EXPECTED:
        _EXPECTED[name] = oracle_expectation(name, frames)
    return _EXPECTED[name]


def workload_frames(name, B=32):
    """the host frames bench.Pipeline gives rank 0 of 1 for `name`, made here without a GPU"""
    import bench
    from vi_slam_amd import synth
    cfg = bench.WORKLOADS[name]
    w, h = cfg["w"], cfg["h"]
    if cfg.get("real"):
        fr = bench.real_frames(cfg)
    elif cfg["stereo"]:
        fr = [synth.make_frame(w, h, step=s // 2, right=bool(s & 1)) for s in range(B if w * h < 1000000 else min(B, 16))]
    else:
        fr = [synth.make_frame(w, h, step=s) for s in range(B)]
    return [fr[s % len(fr)] for s in range(B)]


@pytest.mark.parametrize("name", ALL_WORKLOADS)
def test_oracle_side_of_the_parity_test_is_not_vacuous(name):
    """Without a GPU: for the frames of every workload the oracle finds at least nf / 2 keypoints in every slot, matches in
    every matcher job, stereo pair and tracking job, and the per-step totals of the table at the top (the assertions of
    oracle_expectation).  Step 0 of a run lacks the job of slot 0 / pair 0 only."""
    exp = oracle_expectation(name, workload_frames(name))
    first, later = exp["first"], exp["later"]
    assert sorted(first) == sorted(later) and len(exp["counts"]) == 32
    for nk in ("init_nmatches", "track_nmatches"):
        if nk in later:
            assert len(first[nk]) == len(later[nk]) - 1 == (31 if nk == "init_nmatches" else 15)


# ------------------------------------------------------------------------------------------------ the GPU's side
def _explain(key, got, want, exp):
    """where two arrays that should be equal differ: the slot (or matcher job) of the first difference"""
    if got.shape != want.shape:
        return "%s: shape %s, oracle %s" % (key, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1))
    if key in ("keypoints", "descriptors"):
        off = np.concatenate([[0], np.cumsum(exp["counts"])])
        slots = sorted({int(np.searchsorted(off, b, "right") - 1) for b in bad})
        return "%s: %d rows differ, slots %s" % (key, len(bad), slots[:40])
    return "%s: %d of %d entries differ, first at %d (got %s, oracle %s)" % (key, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


def run_and_compare(name, routes, nsteps=None, **overrides):
    """One Pipeline of workload `name` at the bench's defaults (+ overrides): for each input route a run of nsteps steps,
    every collected step's last_outputs() against the oracle.  -> (list of differences, number of (route, step, slot)
    combinations compared)"""
    import bench

    class Checked(bench.Pipeline):
        def collect(self, t):
            super().collect(t)
            # float32 COPIES: the views in self.last die at this context's next wait
            self.delivered.append((t, self.last_outputs()))

    args = argparse.Namespace(**dict(BENCH_DEFAULTS, **overrides))
    env = {"rank": 0, "world": 1, "local_rank": 0, "barrier": lambda: None, "max_over_ranks": lambda x: x}
    pl = Checked(name, args, env)
    errors, compared = [], 0
    try:
        assert pl.B == 32 and pl.NCTX == 4 and len(pl.ctxs) == 4 and all(c.max_batch == 32 for c in pl.ctxs)
        n = nsteps or 2 * pl.NCTX + 2
        exp = expectation_for(name, pl.frames)
        for route in routes:
            pl.use_inputs(route)
            pl.delivered = []
            pl.run(n)
            assert [t for t, _ in pl.delivered] == list(range(n)), "steps collected out of order or not at all"
            for t, out in pl.delivered:
                want = exp["first" if t == 0 else "later"]
                if sorted(out) != sorted(want):
                    errors.append("%s step %d: outputs %s, expected %s" % (route, t, sorted(out), sorted(want)))
                    continue
                for key in sorted(want):
                    assert out[key].dtype == np.float32
                    if not np.array_equal(out[key], want[key]):
                        errors.append("%s step %d (context %d): %s" % (route, t, t % pl.NCTX, _explain(key, out[key], want[key], exp)))
                compared += pl.B
            pl.delivered = []
    finally:
        pl.close()
    return errors, compared


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_WORKLOADS)
def test_every_step_and_slot_of_a_bench_pipeline_equals_the_oracle(name):
    """Both input routes of one workload, 10 steps each (every context delivers at least twice; on the pinned route every
    un-gated context has replayed its captured graph), all 32 slots of every step: keypoint counts, keypoints, descriptors,
    mono: monoIndex and SearchForInitialization of every job; stereo: mvuRight / mvDepth of all 16 pairs; tracking:
    SearchByProjection of every job.  No tolerance."""
    errors, compared = run_and_compare(name, ("device", "pinned"))
    print("%s: %d (route, step, slot) combinations compared" % (name, compared))
    assert compared == 2 * 10 * 32
    assert not errors, "\n".join(errors[:30])


@pytest.mark.gpu
def test_ungated_mono_pipeline_replays_a_pass_without_its_own_delivery():
    """fast_chain off, pinned inputs: un-gated mono contexts are the only ones that replay a CAPTURED pass whose delivery is
    deferred to the matcher (want_host = 2); the default mono run is gated and never graphed."""
    errors, compared = run_and_compare(ALL_WORKLOADS[0], ("pinned",), fast_chain="off")
    assert compared == 10 * 32
    assert not errors, "\n".join(errors[:30])
