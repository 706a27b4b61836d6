#!/usr/bin/env python3
"""bench.py -- frames/sec of the ORB extract + match front-end on N MI355X (one process per GPU).

    python bench.py --gpus 1 --steps K --warmup W     # the headline figure only: set up, warm up, K timed steps
    python bench.py --full                            # N=1, every workload, host inputs, roofline, CPU baseline: minutes
    python bench.py --gpus N --steps K --warmup W     # N>1 without a launcher: spawns torch.distributed.run itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W     # the driver's form
    python bench.py --steps K --dump-outputs DIR      # + what the last timed step delivered, as DIR/<name>.npy

A "step" = one pass of the hot path over one batch of synthetic frames per rank: `--batch` images go through
extraction (pyramid, FAST+NMS per cell, quadtree, orientation, blur, rBRIEF) and every frame is matched (mono:
FMatcher::SearchForInitialization against its predecessor in video order, window 100; stereo:
Frame::ComputeStereoMatches L<->R).  Keypoints, descriptors and matches are delivered to pinned host memory inside
the step.  Frames are dealt round-robin over ranks; the only collective is one ring shift of packed result slots per
step (mono workload, N>1: vslam_exchange_ring = ncclSend/ncclRecv on the extractor's stream, inside the library).

Rank 0 prints ONE JSON line on stdout:
  value                = headline workload (BASELINE configs[1], KITTI-00 mono 1241x376, 1000 features), input frames
                         resident in HBM when the timed region starts (the contract's definition of `value`)
  ms_per_step          = milliseconds of one timed step; the timed region is exactly K = --steps steps, after at least
                         W = --warmup untimed steps that last 0.5 s or more (Pipeline.warm_up)
With --full, beside it:
  value_host_inputs    = the same workload with the frames in pinned HOST memory: H2D over PCIe inside the timed
                         region (the span frame.cpp:103-116 + :124-132 starts from a host cv::Mat)
  extra_workloads[]    = KITTI-00 stereo N=2000 (north_star's >=5x target) and 1920x1080 stereo N=4000, each with its
                         own value / value_host_inputs / roofline / cpu_baseline
  roofline, roofline_pcie, cpu_baseline, and for N>1 the exchange alone and its GPU-side proof
and every timed region is K steps repeated R times back to back (R chosen so that it lasts >= --min-seconds;
`timed_repeats`).  A second JSON line with per-stage details goes to STDERR.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# Several extractor contexts (HIP streams) are kept in flight; with the runtime's default of 4 hardware
# queues two of them end up behind each other on one queue (measured: 29k -> 38k frames/s with 8).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# RCCL / cross-process device memory need dmabuf IPC on this stack; must be in the environment of EVERY rank process before
# the HIP runtime loads (torch import), whoever launched it (the driver's torch.distributed.run or self_launch below)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

# issue time of a wave64 VALU instruction of the classes the FAST kernel is made of (packed 16-bit, v_perm, v_alignbyte, v_cmp,
# v_mbcnt, DPP/SDWA forms: 4 cycles per SIMD at ~2.26 GHz; profiles/r03_issue_rate_probe.txt, unchanged in round 4); 256 CUs x 4 SIMDs
VALU_NS_PER_WAVE_INST, NUM_SIMDS = 1.77, 1024
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md

WORKLOADS = {
    # BASELINE.json configs[1]: KITTI-00 mono, 8-level pyramid, 1000 features/frame
    "kitti00_mono_1241x376_n1000": dict(w=1241, h=376, nf=1000, stereo=False),
    # config/KITTI00-Mono.yaml:20 says 2000 (config discrepancy)
    "kitti00_mono_1241x376_n2000": dict(w=1241, h=376, nf=2000, stereo=False),
    # configs[2]: KITTI-00 stereo (YAML: 2000 features), L<->R Hamming match -- north_star's target workload
    "kitti00_stereo_1241x376_n2000": dict(w=1241, h=376, nf=2000, stereo=True),
    # configs[4]: synthetic 1920x1080 stream, 4000 features/frame
    "synthetic_stereo_1920x1080_n4000": dict(w=1920, h=1080, nf=4000, stereo=True),
    # SURVEY.md 8(d) "real-image sanity point": the reference's own hut_stereo PNGs (752x480; tests/golden/real_images*.npz),
    # pairs (01,02) (03,04) (04,05) cycled; fx from hut_stereo.json, the baseline is a bench parameter
    "hut_stereo_752x480_n1200_real": dict(w=752, h=480, nf=1200, stereo=True, real="hut", bf=822.5 * 0.4, fx=822.5),
    # SURVEY.md 8(f) rank 1, the per-frame tracking front-end of TrackWithMotionModel: stereo frame construction +
    # UnprojectStereo + SearchByProjection(frame, previous frame); every rank follows its own sequence
    "kitti00_stereo_track_1241x376_n2000": dict(w=1241, h=376, nf=2000, stereo=True, track=True),
}
HEADLINE = "kitti00_mono_1241x376_n1000"
# config/KITTI00-Mono.yaml:20 (2000 features) rides on the driver's line next to BASELINE's configs[1] (1000)
EXTRAS = ["kitti00_mono_1241x376_n2000", "kitti00_stereo_1241x376_n2000", "synthetic_stereo_1920x1080_n4000",
          "hut_stereo_752x480_n1200_real"]
BF, FX = 386.1448, 718.856  # config/KITTI00-Stereo.yaml Camera.bf, Camera.fx
FY, CX, CY = 718.856, 607.1928, 185.2157
TRACK_Z = 12.0  # the synthetic scene moves (+3,+1) px per frame; as a camera translation at this depth
WARMUP_SECONDS = 0.5  # shortest warm-up before an exactly --steps long region (Pipeline.warm_up)
KERNEL_OF = {"pyramid": "k_pyramid", "fast": "k_fast_cells_v3", "blur": "k_blur7_v2", "describe": "k_orient_describe_dev"}
PROF_KEY = {"pyramid": "pyramid_ms", "fast": "fast_ms", "blur": "blur_ms", "describe": "describe_ms"}


def sig(x, n=5):
    """round to n significant digits (keeps the one JSON line short enough for the driver's stdout tail)"""
    if x is None or isinstance(x, (str, bool)) or x == 0 or not isinstance(x, (int, float)):
        return x
    if isinstance(x, int):
        return x
    return float("%.*g" % (n, x))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N worker processes through torch.distributed.run as a CHILD
    process (nothing in this process has touched the GPU -- torch is not even imported yet) and exit with its code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    if args.print_launch:
        print(" ".join(cmd))
        return 0
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL / cross-process device memory)
    return subprocess.call(cmd, env=env)


def real_frames(cfg):
    """the hut_stereo frames as L,R,L,R,... (three pairs; the generator of the fixtures is tests/golden/make_golden.py)"""
    import numpy as np
    z = {}
    for f in ("real_images.npz", "real_images_hut4_5.npz"):
        z.update(np.load(os.path.join(ROOT, "tests", "golden", f)))
    out = []
    for a, b in (("hut1", "hut2"), ("hut3", "hut4"), ("hut4", "hut5")):
        out += [np.ascontiguousarray(z[a]), np.ascontiguousarray(z[b])]
    return out


def level_pixels(fe):
    return [fe.level_size(l)[0] * fe.level_size(l)[1] for l in range(fe.nlevels)]


def algorithmic_bytes(fe, nf):
    """SURVEY.md 8(d) per-image algorithmic bytes of each kernel stage."""
    px = level_pixels(fe)
    P = sum(px)
    return dict(pyramid=(P - px[-1]) + (P - px[0]), fast=P, blur=2 * P, describe=2 * P + 60 * nf, total_px=P)


def pmc_traffic(kernel, cfg, batch):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc summary (tools/collect_pmc.sh: separate
    FETCH_SIZE / WRITE_SIZE passes).  gfx950's FETCH_SIZE counts 64 B per 128-B request, i.e. half of a coalesced
    stream (MI355X_MICROARCH.md 'HBM'); the factor 2 is applied here.  Only valid for the geometry / batch /
    feature count the profile was taken with; otherwise None."""
    for rnd in ("r04", "r03", "r02"):  # the newest committed summary for this geometry
        name = "%s_pmc_traffic_%dx%d_n%d_b%d.json" % (rnd, cfg["w"], cfg["h"], cfg["nf"], batch)
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            break
    else:
        return None
    k = json.load(open(path))["kernels"].get(kernel.split("(")[0])
    if not k or "fetch_bytes_raw" not in k or "write_bytes" not in k:
        return None
    return {"bytes": 2 * k["fetch_bytes_raw"] + k["write_bytes"], "fetch_size_raw_bytes": k["fetch_bytes_raw"],
            "write_size_bytes": k["write_bytes"], "valu_insts": k.get("SQ_INSTS_VALU"), "source": "profiles/" + name}


# ------------------------------------------------------------------------------------------------ CPU baseline
def cpu_baseline(cfg, seconds=12.0, all_seconds=8.0):
    """The oracle (a port of the reference's CPU path, oracle/) timed on this box's host cores: the same
    workload on a bounded sample of frames, reference-faithful threading (1 thread per image; the two
    images of a stereo frame on 2 threads, frame.cpp:107-108).  Test infrastructure used as the CHECKER/baseline
    only, after the timed GPU region."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from oracle import orbo
    from vi_slam_amd import synth
    w, h, nf, stereo = cfg["w"], cfg["h"], cfg["nf"], cfg["stereo"]
    bf, fx = cfg.get("bf", BF), cfg.get("fx", FX)
    nsample = 6 if w * h < 1000000 else 3
    frames = 0
    if stereo:
        if cfg.get("real"):
            rf = real_frames(cfg)
            pairs = [(rf[2 * j], rf[2 * j + 1]) for j in range(len(rf) // 2)]
            nsample = len(pairs)
        else:
            pairs = [synth.make_stereo_pair(w, h, step=s) for s in range(nsample)]
        eL, eR = orbo.Extractor(nf), orbo.Extractor(nf)
        pool = ThreadPoolExecutor(2)
        prev_track = None
        t0 = time.time()
        t_end = t0 + seconds
        while time.time() < t_end:
            L, R = pairs[frames % nsample]
            fl = pool.submit(eL.compute, L)
            fr = pool.submit(eR.compute, R)
            (kL, dL, _), (kR, dR, _) = fl.result(), fr.result()
            uR, depth = orbo.stereo(eL, eR, kL, dL, kR, dR, bf, fx)[:2]
            if cfg.get("track"):
                T0 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
                x3, has = orbo.unproject_stereo(kL, depth, T0, CX, CY, 1.0 / FX, 1.0 / FY)
                if prev_track is not None:
                    pk, pd, px, pf = prev_track
                    Tcw = np.hstack([np.eye(3), np.array([[3.0 / FX * TRACK_Z], [1.0 / FY * TRACK_Z], [0.0]])])
                    orbo.search_by_projection_frame(Tcw, T0, (FX, FY, CX, CY, BF, BF / FX), 15, pk, pf * 3, px, pd, kL, dL,
                                                    uR, eL.tables()["scale"], w, h)
                prev_track = (kL.copy(), dL.copy(), x3, has)
            frames += 1
        cores = 2
        sample = "%d %s stereo frames %dx%d, %d features: 2 threads extract L/R + ComputeStereoMatches%s" % (
            frames, "real (hut_stereo)" if cfg.get("real") else "synthetic", w, h, nf, " + UnprojectStereo + SearchByProjection(prev frame)" if cfg.get("track") else "")
    else:
        imgs = [synth.make_frame(w, h, step=s) for s in range(nsample)]
        e = orbo.Extractor(nf)
        prev = None
        t0 = time.time()
        t_end = t0 + seconds
        while time.time() < t_end:
            k, d, _ = e.compute(imgs[frames % nsample], lap=(0, 1000))
            if prev is not None:
                orbo.search_for_initialization(prev[0], prev[1], k, d, w, h, window=100, nnratio=0.9)
            prev = (k, d)
            frames += 1
        cores = 1
        sample = "%d synthetic mono frames %dx%d, %d features: extract + SearchForInitialization(prev)" % (
            frames, w, h, nf)
    dt = time.time() - t0
    out = {"value": frames / dt, "unit": "frames/s", "cores": cores, "kind": "port", "sample": sample}
    if all_seconds > 0:
        out["all_cores"] = cpu_baseline_all_cores(cfg, all_seconds)
    return out


def cpu_baseline_all_cores(cfg, seconds=8.0):
    """SURVEY.md 8(d) variant (ii): every host core of the box, frame-parallel (one oracle extractor per thread,
    each thread following its own frame sequence; ctypes releases the GIL).  Reported beside the
    reference-faithful figure, never as the headline."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import orbo
    from vi_slam_amd import synth
    w, h, nf, stereo = cfg["w"], cfg["h"], cfg["nf"], cfg["stereo"]
    bf, fx = cfg.get("bf", BF), cfg.get("fx", FX)
    ncores = max(1, min(os.cpu_count() or 1, 64))
    nsample = 3
    if stereo and cfg.get("real"):
        rf = real_frames(cfg)
        data = [(rf[2 * j], rf[2 * j + 1]) for j in range(len(rf) // 2)]
        nsample = len(data)
    elif stereo:
        data = [synth.make_stereo_pair(w, h, step=s) for s in range(nsample)]
    else:
        data = [synth.make_frame(w, h, step=s) for s in range(nsample)]
    t_end = time.time() + seconds

    def worker(_):
        e, e2 = orbo.Extractor(nf), orbo.Extractor(nf)
        prev, n = None, 0
        while time.time() < t_end:
            if stereo:
                L, R = data[n % nsample]
                kL, dL, _ = e.compute(L)
                kR, dR, _ = e2.compute(R)
                orbo.stereo(e, e2, kL, dL, kR, dR, bf, fx)
            else:
                k, d, _ = e.compute(data[n % nsample], lap=(0, 1000))
                if prev is not None:
                    orbo.search_for_initialization(prev[0], prev[1], k, d, w, h, window=100, nnratio=0.9)
                prev = (k, d)
            n += 1
        return n

    t0 = time.time()
    with ThreadPoolExecutor(ncores) as pool:
        total = sum(pool.map(worker, range(ncores)))
    dt = time.time() - t0
    return {"value": total / dt, "unit": "frames/s", "cores": ncores,
            "sample": "%d frames on %d threads, one sequence per thread" % (total, ncores)}


# ------------------------------------------------------------------------------------------------ one workload
class Pipeline:
    """NCTX extractor contexts (HIP streams) kept in flight on one GPU; step t runs on context t % NCTX.  A step is
    enqueued completely (H2D pull if the frames are in host memory, extraction, [N>1: pack + ring exchange],
    matcher, D2H of results) with GPU-side events between contexts and collected by ONE host wait."""

    def __init__(self, name, args, env):
        import ctypes
        import numpy as np
        import torch
        import vi_slam_amd as V
        from vi_slam_amd import dist as vd
        from vi_slam_amd import synth
        self.np, self.torch, self.V, self.vd = np, torch, V, vd
        self.name, self.args, self.env = name, args, env
        rank, world = env["rank"], env["world"]
        cfg = self.cfg = WORKLOADS[name]
        w, h, nf = cfg["w"], cfg["h"], cfg["nf"]
        self.stereo, self.track = cfg["stereo"], bool(cfg.get("track"))
        B = args.batch
        if self.stereo and B % 2:
            B += 1
        if self.track:
            B = min(B, 32)  # one SearchByProjection pass takes up to 16 frame pairs
        self.B = B
        self.NCTX = max(3, args.inflight)
        self.multi = (world > 1 or args.force_collective) and not self.stereo
        # a stream priority of its own keeps the four contexts off the hardware queues torch's and RCCL's streams use
        # (DESIGN section 6); the library's default is the normal pool, a pipelined caller opts in
        tuning = dict(stream_priority=args.stream_priority)
        if args.upload_split:
            tuning["stage_split_event"] = 2
        if args.fast_kernel >= 0:
            tuning["fast_kernel"] = args.fast_kernel
        if args.wave_prio >= 0:
            tuning["wave_prio"] = args.wave_prio
        self.ctxs = [V.FExtractor(nf, 1.2, 8, 20, 7, w, h, device=env["local_rank"], max_batch=B, tuning=tuning)
                     for _ in range(self.NCTX)]
        self.fe = self.ctxs[0]
        # FAST(t) starts when FAST(t-1) has finished: never two FAST launches resident at once.  FAST takes every CU's whole LDS;
        # with two of them in flight the pipeline flips between a smooth state (mono 187 k frames/s) and one that runs like three
        # contexts (172 k, a 400-us delivery gap every ~10 steps) for hundreds of steps at a time; chained it stays at 186 k
        # (+6 %, HBM-resident and host inputs alike).  The stereo workloads' contexts are independent of each other -- no
        # cross-frame matcher -- and a chain is the only coupling they would have: it buys them nothing (-0.5 %) and lets one late
        # context hold up the other three (blocks at 60-75 % of the rate in two of four runs): auto = mono only
        self.fast_chain = args.fast_chain == "on" or (args.fast_chain == "auto" and not self.stereo)
        if self.fast_chain:
            for k, c in enumerate(self.ctxs):
                c.set_fast_gate(self.ctxs[(k - 1) % self.NCTX])
        self.matchers = [V.FMatcher(c, 0.9, True) for c in self.ctxs]
        self.lap = (0, 0) if self.stereo else (0, 1000)  # frame.cpp:107-108 vs :289
        # ---- synthetic frames (host copies kept for the pinned-input mode)
        ndistinct = B if w * h < 1000000 else min(B, 16)  # 1080p frames are slow to synthesise; cycled
        self.ndistinct = ndistinct
        frames = []
        self.bf, self.fx = cfg.get("bf", BF), cfg.get("fx", FX)
        if cfg.get("real"):
            frames = real_frames(cfg)
            ndistinct = self.ndistinct = len(frames)
        for s in range(0 if cfg.get("real") else ndistinct):
            if self.track:  # one contiguous sequence per rank
                fr = synth.make_frame(w, h, seed=20250215 + rank, step=s // 2, right=bool(s & 1))
            elif self.stereo:
                fr = synth.make_frame(w, h, step=(s // 2) * world + rank, right=bool(s & 1))
            else:
                fr = synth.make_frame(w, h, step=vd.global_frame(rank, s, world, B))
            frames.append(fr)
        self.frames = [frames[s % ndistinct] for s in range(B)]
        self.pitch = (w + 127) & ~127
        self.dev_frames = torch.zeros((B, h, self.pitch), dtype=torch.uint8, device="cuda")
        for s in range(B):
            self.dev_frames[s, :, :w] = torch.from_numpy(self.frames[s]).cuda()
        self.dev_ptrs = (ctypes.c_void_p * B)(*[self.dev_frames[s].data_ptr() for s in range(B)])
        self.pinned = None
        self.where = V.IMGS_DEVICE
        self.slot_bytes = self.fe.slot_bytes
        self.desc_off = 16 + self.fe.cap * 28
        nb = self.NCTX if self.multi else 0
        self.packed = [torch.zeros(self.slot_bytes, dtype=torch.uint8, device="cuda") for _ in range(nb)]  # the rank's LAST frame
        self.xchg = env.get("xchg")
        recv_n = (world if (self.xchg and self.xchg.mode == "allgather") else 1) * self.slot_bytes
        self.recv = [torch.zeros(recv_n, dtype=torch.uint8, device="cuda") for _ in range(nb)]
        # single GPU: the last frame of a step, which the NEXT step's first matcher job reads, is copied into a carry
        # buffer of its own, so that a context may start its next extraction without waiting for that matcher
        self.carry = [torch.zeros(self.slot_bytes, dtype=torch.uint8, device="cuda") for _ in range(0 if self.multi else self.NCTX)]
        self.state = {"matches": 0}
        self.stamps = None  # timed(): host time at which every step's results were delivered
        self.step_trace = None
        self.last = None  # collect(): (step, features, stereo, matcher outputs) of the last step delivered
        self.job_cache = {}
        self.track_Twc = [np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)] * (B // 2)
        self.track_cam = (CX, CY, float(np.float32(1.0) / np.float32(FX)), float(np.float32(1.0) / np.float32(FY)))
        self.track_Tcw = np.hstack([np.eye(3), np.array([[3.0 / FX * TRACK_Z], [1.0 / FY * TRACK_Z], [0.0]])]).astype(np.float32)
        torch.cuda.synchronize()

    # -------------------------------------------------------------------------------------------- inputs
    def use_inputs(self, mode):
        """'device': frames resident in HBM, zero-copy level 0.  'pinned': frames in pinned host memory (one ring of B
        buffers per context, as a capture driver's DMA ring): every pass pulls them over PCIe itself."""
        V = self.V
        self.torch.cuda.synchronize()
        if mode == "pinned":
            if self.pinned is None:
                self.pinned = []
                for _ in range(self.NCTX):
                    p = V.PinnedImages(self.B, self.cfg["h"], self.cfg["w"], self.cfg["w"])  # rows packed like cv::Mat
                    for s in range(self.B):
                        p.array[s][:] = self.frames[s]
                    self.pinned.append(p)
            self.where = V.IMGS_PINNED
        else:
            self.where = V.IMGS_DEVICE
        self.job_cache = {}

    def _imgs(self, k):
        if self.where == self.V.IMGS_PINNED:
            return self.pinned[k].ptrs, self.pinned[k].pitch
        return self.dev_ptrs, self.pitch

    # -------------------------------------------------------------------------------------------- one step
    def _slot_ptrs_in(self, buf, s):
        """(kps, desc, count) device addresses of slot s inside a packed buffer."""
        base = buf.data_ptr() + s * self.slot_bytes
        return base + 16, base + self.desc_off, base

    def enqueue(self, t):
        """Enqueue step t completely without waiting for anything on the host: every pointer is a fixed address and
        the keypoint counts stay in HBM."""
        V, vd = self.V, self.vd
        NCTX, B, st = self.NCTX, self.B, self.state
        rank, world = self.env["rank"], self.env["world"]
        w, h = self.cfg["w"], self.cfg["h"]
        c, k = self.ctxs[t % NCTX], t % NCTX
        nxt, prv = self.ctxs[(t + 1) % NCTX], self.ctxs[(t - 1) % NCTX]
        ptrs, pitch = self._imgs(k)
        where = self.where
        if where == V.IMGS_PINNED:
            # The PCIe upload of step t is enqueued at the head of the step, on the context's own stream, and the uploads are
            # paced by an event chain of lag L (--upload-chain L): upload t starts when upload t-L has landed, so at most L
            # are in flight.  Without any chain several contexts that happen to upload at the same time share the link,
            # finish together, compute together and come back to the link together -- a phase the pipeline stayed locked
            # in for whole runs in round 2 (79 k vs 106 k mono frames/s between runs); a strict chain (L = 1) is stable but
            # leaves the link idle for the hand-over between two transfers (94.7 k, every run); L = 2 keeps a second
            # transfer queued behind the running one.
            lag = self.args.upload_chain
            if lag > 0 and t >= lag:
                c.event_wait(self.ctxs[(t - lag) % NCTX], 2)
            c.stage_images_async(ptrs, pitch, V.IMGS_PINNED)
            if not self.args.upload_split:
                c.event_record(2)  # (with --upload-split the library records event 2 between the two halves of the upload)
            where = V.IMGS_STAGED
        if self.track:
            npairs = B // 2
            c.event_wait(nxt, 1)  # nxt's matcher (step t-NCTX+1) read our last frame: it must finish first
            c.frame_stereo_async(ptrs, pitch, self.bf, self.fx, where=where)
            c.stereo_points_async(self.track_Twc, self.track_cam)  # UnprojectStereo of every left keypoint
            c.event_record(0)
            ck = (k, t == 0)
            if ck not in self.job_cache:
                jobs = []
                for j in range(npairs):
                    if j == 0 and t == 0:
                        continue
                    lc, lj = (c, j - 1) if j else (prv, npairs - 1)
                    lk, ld, ln = lc.slot_dev_ptrs(2 * lj)
                    x3, fl, _, _ = lc.stereo_points_buffers(lj, with_stereo=False)
                    ckp, cd, cn = c.slot_dev_ptrs(2 * j)
                    ur = c.stereo_points_buffers(j)[2]
                    jobs.append(dict(Tcw=self.track_Tcw, cam=(FX, FY, CX, CY, BF), th=15, forward=0, backward=0, img=(w, h),
                                     last_kps=lk, n_last=ln, last_flags=fl, last_x3dw=x3, mp_desc=ld, cur_kps=ckp,
                                     cur_desc=cd, n_cur=cn, cur_u_right=ur))
                self.job_cache[ck] = (V.FMatcher.make_sbp_jobs(jobs, True), len(jobs))
            arr, njobs = self.job_cache[ck]
            if t > 0:
                c.event_wait(prv, 0)
            self.matchers[k].search_by_projection_dev_async(arr)
            c.event_record(1)
            st.setdefault("njobs", {})[t] = njobs
            return
        if self.stereo:
            c.frame_stereo_async(ptrs, pitch, self.bf, self.fx, where=where)
            return
        # The extraction overwrites only this context's own result slots, which nobody else reads: what the matcher of
        # the NEXT step (context nxt, step t-NCTX+1) read from us is the carry / exchange buffer, so only the copy into
        # that buffer has to wait for it -- not the extraction.  (With the wait in front of the extraction a context sat
        # idle for a whole step between two of its passes: 353 us per 1140-us cycle in the kernel trace.)
        # ONE result transfer per step: the extraction's delivery is deferred to the matcher call below (want_host = 2) --
        # counts, keypoints, descriptors and vnMatches12 of the step are one block (--delivery separate for A/B)
        c.compute_batch_async(ptrs, pitch, self.lap, where=where,
                              to_host="with_matcher" if self.args.delivery == "single" else True)
        c.event_wait(nxt, 1)
        if self.multi:  # the right neighbour needs this rank's last frame: pack it and shift it round the ring
            c.pack_slots(1, self.packed[k].data_ptr(), self.slot_bytes, first=B - 1, sync=False)
            # One exchange at a time per rank, in step order on every rank: step t's shift starts when step t-1's has
            # finished (a GPU-side event between the two contexts' streams).  Each lane has its own communicator so that
            # RCCL does not serialise whole streams, but operations of SEVERAL communicators in flight at once are only
            # safe if every rank can run them all concurrently; the chain removes the question (the matcher of step t
            # waits for step t-1's results anyway).
            if t > 0 and self.args.exchange_chain:
                c.event_wait(prv, 3)
            self.xchg.exchange(c, self.packed[k], self.recv[k], lane=k)  # RCCL: enqueued on c's own stream (no host sync)
            c.event_record(3)
        else:
            c.pack_slots(1, self.carry[k].data_ptr(), self.slot_bytes, first=B - 1, sync=False)
        c.event_record(0)  # step t's results (own, and the left neighbour's / the carried last frame) are complete
        # the device addresses are fixed per context, so the job array is built once (t == 0 has no predecessor
        # for slot 0 and is built separately)
        ck = (k, t == 0)
        if ck not in self.job_cache:
            jobs = []
            uses_prev_step = False
            for s in range(B):
                pr, ps, prev_step = vd.predecessor(rank, s, world, B)
                if s > 0:
                    p = c.slot_dev_ptrs(ps)  # the rank's own previous slot
                else:  # the left neighbour's last frame: out of the exchange buffer (single GPU: the carry buffer)
                    if prev_step:
                        if t == 0:
                            continue
                        uses_prev_step = True
                    kk = (t - 1) % NCTX if prev_step else k
                    p = (self._slot_ptrs_in(self.xchg.left_block(self.recv[kk]), 0) if self.multi
                         else self._slot_ptrs_in(self.carry[kk], 0))
                q = c.slot_dev_ptrs(s)
                jobs.append((p[0], p[1], p[2], q[0], q[1], q[2], 0))
            self.job_cache[ck] = (V.FMatcher.make_init_jobs(jobs) if jobs else None, len(jobs), uses_prev_step)
        arr, njobs, uses_prev_step = self.job_cache[ck]
        if uses_prev_step:
            c.event_wait(prv, 0)  # the previous step's results (not its matcher)
        if njobs:
            self.matchers[k].search_init_dev_async(arr, 100, (w, h))
        c.event_record(1)  # matcher(t) complete
        st.setdefault("njobs", {})[t] = njobs

    def collect(self, t):
        """One host wait per step delivers keypoints, descriptors and the matches."""
        st, B = self.state, self.B
        c = self.ctxs[t % self.NCTX]
        t_a = time.perf_counter()
        out = []
        if self.stereo:
            feats, stv = c.frame_stereo_wait()
            st["matches"] = sum(int((u >= 0).sum()) for u, _ in stv)
            t_b = time.perf_counter()
            if self.track:
                nj = st["njobs"].pop(t)
                ncur = [len(feats[2 * j][0]) for j in range(B // 2 - nj, B // 2)]
                out = self.matchers[t % self.NCTX].search_by_projection_dev_wait(ncur)
                st["track_matches"] = sum(o[0] for o in out)
        else:
            feats, stv = c.wait(), None
            t_b = time.perf_counter()
            nj = st["njobs"].pop(t)
            if nj:
                out = self.matchers[t % self.NCTX].search_init_dev_wait([self.fe.cap] * nj)
                st["matches"] = sum(o[0] for o in out)
        # what the step delivered (views into the context's staging, valid until its next wait): --dump-outputs
        self.last = (t, feats, stv, out)
        hs = st.setdefault("host_s", [0.0, 0.0])
        hs[0] += t_b - t_a
        hs[1] += time.perf_counter() - t_b

    def run(self, nsteps):
        NCTX = self.NCTX
        trace = self.step_trace  # --stamp-dump: (enqueue start, enqueue end, wait start, wait end) of every step, host clock
        for t in range(nsteps + NCTX - 1):
            if t < nsteps:
                t_e = time.perf_counter()
                self.enqueue(t)
                t_f = time.perf_counter()
                self.state["enq_s"] = self.state.get("enq_s", 0.0) + t_f - t_e
                if trace is not None:
                    trace.append(("e", t, t_e, t_f))
            if 0 <= t - (NCTX - 1) < nsteps:
                t_w = time.perf_counter()
                self.collect(t - (NCTX - 1))
                t_d = time.perf_counter()
                if self.stamps is not None:
                    self.stamps.append(t_d)  # step t - (NCTX - 1) delivered
                if trace is not None:
                    trace.append(("w", t - (NCTX - 1), t_w, t_d))

    # -------------------------------------------------------------------------------------------- exchange proof
    def verify_exchange(self, xchg):
        """One UNTIMED step that proves the exchange on the GPU, without the oracle: this rank extracts its own batch,
        packs its last frame and sends it round `xchg`; then it extracts the LEFT neighbour's last frame ITSELF (frames are
        synthesised from their global index, so every rank can make any frame) and compares the packed slot that arrived
        with the one it packed locally -- count, monoIndex, keypoints, descriptors, byte for byte -- and the matcher output
        of its own slot 0 against the arrived predecessor with the one against the local copy.
        -> dict(ok, n, reason, matcher_ok, matches, us)"""
        import ctypes
        torch, V, vd, np = self.torch, self.V, self.vd, self.np
        from vi_slam_amd import synth
        rank, world, B = self.env["rank"], self.env["world"], self.B
        w, h = self.cfg["w"], self.cfg["h"]
        c, c2 = self.ctxs[0], self.ctxs[1]
        sb = self.slot_bytes
        torch.cuda.synchronize()
        self.env["barrier"]()
        # 1. own step on context 0: extract, pack the last frame, exchange
        c.compute_batch_async(self.dev_ptrs, self.pitch, self.lap, where=V.IMGS_DEVICE, to_host=False)
        send = torch.zeros(sb, dtype=torch.uint8, device="cuda")
        recv = torch.zeros(sb * (world if xchg.mode == "allgather" else 1), dtype=torch.uint8, device="cuda")
        c.pack_slots(1, send.data_ptr(), sb, first=B - 1, sync=False)
        t0 = time.perf_counter()
        xchg.exchange(c, send, recv, lane=0)
        c.wait()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6
        got = xchg.left_block(recv)[:sb]
        # 2. the left neighbour's last frame, extracted HERE (every slot of context 1 gets the same image; slot B-1 is packed)
        lr, ls, _ = vd.left_last_frame(rank, world, B)
        fr = synth.make_frame(w, h, step=vd.global_frame(lr, ls % self.ndistinct, world, B))
        dev = torch.zeros((h, self.pitch), dtype=torch.uint8, device="cuda")
        dev[:, :w] = torch.from_numpy(fr).cuda()
        ptrs2 = (ctypes.c_void_p * B)(*[dev.data_ptr()] * B)
        c2.compute_batch_async(ptrs2, self.pitch, self.lap, where=V.IMGS_DEVICE, to_host=False)
        local = torch.zeros(sb, dtype=torch.uint8, device="cuda")
        c2.pack_slots(1, local.data_ptr(), sb, first=B - 1, sync=False)
        c2.wait()
        torch.cuda.synchronize()
        res = vd.compare_packed_slots(got.cpu().numpy(), local.cpu().numpy())
        # 3. the matcher on slot 0 with the arrived predecessor and with the local copy
        q = c.slot_dev_ptrs(0)
        m = []
        for buf in (got, local):
            p0 = self._slot_ptrs_in(buf, 0)
            self.matchers[0].search_init_dev_async([(p0[0], p0[1], p0[2], q[0], q[1], q[2], 0)], 100, (w, h))
            m.append(self.matchers[0].search_init_dev_wait([self.fe.cap])[0])
        res["matcher_ok"] = bool(m[0][0] == m[1][0] and np.array_equal(m[0][1], m[1][1]))
        res["matches"] = int(m[1][0])
        res["us"] = us
        res["ok"] = bool(res["ok"])
        if not (res["ok"] and res["matcher_ok"]):
            print("rank %d: exchange verification FAILED (%s): %s; matcher %s" % (rank, xchg.mode, res["reason"], res["matcher_ok"]),
                  file=sys.stderr, flush=True)
        return res

    # -------------------------------------------------------------------------------------------- timing
    def warm_up(self, warmup):
        """At least `warmup` untimed steps, then more in blocks until the warm-up has lasted WARMUP_SECONDS: a GPU that comes
        out of the set-up idle runs its first steps slowly (5 warmup steps alone left 20 timed mono steps at 0.92 instead of
        0.16 ms each; 20 left 4 ms of 495 in a region of 3000 steps).  All ranks agree on every further block (exchanges)."""
        t_end = time.perf_counter() + WARMUP_SECONDS
        self.run(max(warmup, 1))
        while self.env["max_over_ranks"](1.0 if time.perf_counter() < t_end else 0.0) > 0:
            self.run(50)

    def timed(self, steps, warmup, min_seconds, profile=False, outputs=False):
        """W warmup steps, then the timed region bracketed by barrier + synchronize; max over ranks.  min_seconds = 0: the
        region is exactly K = `steps` steps.  min_seconds > 0 (--full): R x K steps, R measured on calibration blocks and
        agreed by all ranks BEFORE the region (every rank must issue the same number of exchanges).  profile: per-stage
        event spans from a run of their own after the region.  outputs: what the region's last step delivered
        (last_outputs)."""
        env = self.env
        import gc
        gc_was = gc.isenabled()
        reps = 1
        if min_seconds > 0:
            self.run(max(warmup, 1))
            self.run(steps)  # first calibration block: still warming up (first DMA copies, clocks) -- not used
            self.torch.cuda.synchronize()
            env["barrier"]()
            t0 = time.perf_counter()
            self.run(steps)  # second calibration block, untimed but clocked: how many repeats make min_seconds
            self.torch.cuda.synchronize()
            block = env["max_over_ranks"](time.perf_counter() - t0)
            reps = max(1, min(int(math.ceil(1.25 * min_seconds / max(block, 1e-6))), 100000 // max(steps, 1) + 1))
        # The harness is Python; the product's host side is C++.  A collection of the cyclic garbage collector inside the
        # timed region stalls the one host thread for a few hundred microseconds -- two or three steps' worth -- which is what
        # the blocks well below the median were; the collector is switched off for the region (--gc keeps it)
        if not self.args.gc:
            gc.collect()
            gc.disable()
        # the collection above left the GPU idle for tens of milliseconds; the first blocks of the region then ran 10-13 %
        # below the rest (profiles/r04_slow_blocks.txt): fill the pipeline, untimed, before the bracket (the warmup steps
        # themselves when there is no calibration)
        if min_seconds > 0:
            self.run(steps)
        else:
            self.warm_up(warmup)
        for k in ("host_s", "enq_s"):
            self.state.pop(k, None)
        env["barrier"]()
        self.stamps = []
        self.step_trace = [] if self.args.stamp_dump else None
        sent0 = [c.delivery_stats() for c in self.ctxs]
        t0 = time.perf_counter()
        self.run(steps * reps)  # the timed region: the product path as a caller runs it (no per-stage events)
        env["barrier"]()
        dt = env["max_over_ranks"](time.perf_counter() - t0)
        if gc_was:
            gc.enable()
        delivered = self.last_outputs() if outputs else None
        if self.step_trace is not None:
            with open("%s.%s.%s.json" % (self.args.stamp_dump, self.name, "pinned" if self.where == self.V.IMGS_PINNED else "device"), "w") as f:
                json.dump({"workload": self.name, "steps": steps, "reps": reps, "t0": t0, "dt": dt, "gc": bool(self.args.gc),
                           "events": self.step_trace}, f)
            self.step_trace = None
        sent = [tuple(b - a for a, b in zip(s0, c.delivery_stats())) for s0, c in zip(sent0, self.ctxs)]
        stamps, self.stamps = self.stamps, None
        host_times = {k: self.state.get(k) for k in ("host_s", "enq_s")}
        # per-stage event spans inside the pipeline: a short run of its own with the contexts' stage events switched on
        # (they cost launches of their own and keep the pass out of its captured graph), after the timed region
        prof = {}
        if profile:
            for c in self.ctxs:
                c.set_profiling(True)
            self.run(steps * min(reps, 10))
            self.torch.cuda.synchronize()
            for c in self.ctxs:
                for k, v in c.get_profile().items():
                    prof[k] = prof.get(k, 0) + v
                c.set_profiling(False)
        for k, v in host_times.items():
            if v is not None:
                self.state[k] = v
        frames_per_step = (self.B // 2 if self.stereo else self.B) * env["world"]
        n = steps * reps
        # spread over the region: the rate of every block of `bs` consecutive steps (delivery time stamps of this rank; the
        # first block also carries the pipeline's fill).  The contexts in flight finish their steps in BURSTS -- three short
        # delivery gaps, then a long one, up to 8 x the mean at 1080p (profiles/r04_slow_blocks.txt) -- so the rate of a block
        # is quantised by (one between-burst gap / block length): +-10-16 % for blocks of 20 steps whatever the GPU does.
        # Blocks of 25 bursts bound that at +-2 %; what is left is the pipeline's own variation.
        bs = max(steps, 25 * self.NCTX)
        nblk = len(stamps) // bs
        blocks = [frames_per_step * bs / (stamps[(r + 1) * bs - 1] - stamps[r * bs - 1]) for r in range(1, nblk)
                  if stamps[(r + 1) * bs - 1] > stamps[r * bs - 1]]
        blocks.sort()
        spread = ({"min": blocks[0], "median": blocks[len(blocks) // 2], "max": blocks[-1], "blocks": len(blocks), "block_steps": bs}
                  if blocks else None)
        return {"value": frames_per_step * n / dt, "ms_per_step": dt / n * 1e3, "reps": reps, "seconds": dt, "prof": prof,
                "spread": spread, "outputs": delivered,
                # result deliveries of this rank's contexts: copy operations towards the host per step, and their bytes
                "result_transfers_per_step": sum(a for a, _ in sent) / n, "result_bytes_per_step": sum(b for _, b in sent) / n,
                "host_ms_per_step": {k: v / n * 1e3 for k, v in zip(("enqueue", "wait_step", "fetch_matches"),
                                                                   [self.state.get("enq_s", 0.0)] + self.state.get("host_s", [0, 0]))}}

    def last_outputs(self):
        """What the last collected step delivered to its caller, as float32 arrays (--dump-outputs): every image's keypoints
        (x, y, size, angle, response, octave, class_id) and descriptors, concatenated in slot order, with the per-image counts;
        mono: monoIndex and, per matcher job, SearchForInitialization's nmatches and vnMatches12 (over the predecessor's
        keypoints); stereo: mvuRight / mvDepth of every left image; tracking: SearchByProjection's nmatches and matches."""
        np, B = self.np, self.B
        t, feats, stv, out = self.last
        f32 = lambda a: np.asarray(a, np.float32)
        counts = [len(f[0]) for f in feats]
        res = {"keypoint_counts": f32(counts),
               "keypoints": np.concatenate([np.stack([f[0][n].astype(np.float32) for n in f[0].dtype.names], 1) for f in feats]),
               "descriptors": np.concatenate([f32(f[1]).reshape(-1, 32) for f in feats])}
        if self.stereo:
            res["u_right"] = np.concatenate([f32(u) for u, _ in stv])
            res["depth"] = np.concatenate([f32(d) for _, d in stv])
            if self.track:
                res["track_nmatches"] = f32([o[0] for o in out])
                res["track_matches"] = np.concatenate([f32(o[1]) for o in out] or [f32([])])
            return res
        res["mono_index"] = f32([f[2] for f in feats])
        # job j matched query slot B - njobs + j (slot 0 has no job in a run's first step) against its predecessor
        rank, world = self.env["rank"], self.env["world"]
        m12 = []
        for j, (_, m, _) in enumerate(out):
            s = B - len(out) + j
            _, ps, prev_step = self.vd.predecessor(rank, s, world, B)
            if s > 0:
                n1 = counts[ps]
            else:  # the left neighbour's last frame, carried or exchanged: its count heads the packed slot
                kk = (t - 1) % self.NCTX if prev_step else t % self.NCTX
                buf = self.xchg.left_block(self.recv[kk]) if self.multi else self.carry[kk]
                n1 = int(buf[:4].cpu().numpy().view(np.int32)[0])
            m12.append(f32(m[:n1]))
        res["init_nmatches"] = f32([o[0] for o in out])
        res["init_matches12"] = np.concatenate(m12 or [f32([])])
        return res

    def single_context_stage_ms(self, passes=30):
        """The extraction pass alone on the GPU (one context, device-resident frames, no matcher, nothing else in flight):
        per-stage HIP-event times whose spans contain no other stream's workgroups.  `passes` warm passes first so the
        clocks are where a busy GPU holds them, then `passes` measured ones."""
        self.torch.cuda.synchronize()
        c0 = self.ctxs[0]
        for i in range(2 * passes):
            if i == passes:
                c0.set_profiling(True)
            if self.stereo:
                c0.frame_stereo_async(self.dev_ptrs, self.pitch, self.bf, self.fx)
                c0.frame_stereo_wait()
            else:
                c0.compute_batch_async(self.dev_ptrs, self.pitch, self.lap)
                c0.wait()
        alone = c0.get_profile()
        c0.set_profiling(False)
        nb = max(alone.get("batches", 0), 1)
        return {k: alone[v] / nb for k, v in PROF_KEY.items()} | {"octree": alone["octree_ms"] / nb}

    def close(self):
        self.torch.cuda.synchronize()
        for c in self.ctxs:
            c.close()
        for p in self.pinned or []:
            p.close()
        self.dev_frames = None
        self.packed = self.recv = self.carry = None


def roofline_of(pl, stage_alone, stage_pipe, res_dev):
    """roofline object of one workload: the dominant image-streaming KERNEL (by its single-context launch time), its
    algorithmic bytes per launch (SURVEY.md 8(d) x images per launch) over that time."""
    ab = algorithmic_bytes(pl.fe, pl.cfg["nf"])
    nlaunch = pl.fe.pyramid_launches() if hasattr(pl.fe, "pyramid_launches") else 7
    per_launch = {k: (v / nlaunch if k == "pyramid" else v) for k, v in stage_alone.items() if k != "octree"}
    dom = max(per_launch, key=per_launch.get)
    kof = dict(KERNEL_OF)
    if pl.args.fast_kernel != 3 and pl.B > 2:  # the library's default for batches (vslam_tuning.fast_kernel)
        kof["fast"] = "k_fast_bands"
    kernel = kof[dom] if dom != "pyramid" else ("k_resize_level_v2(x%d)" % nlaunch if nlaunch > 2 else "k_pyramid")
    bytes_per_launch = ab[dom] * pl.B / (nlaunch if dom == "pyramid" else 1.0)
    ms = per_launch[dom]
    achieved = bytes_per_launch / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    tr = pmc_traffic(kernel, pl.cfg, pl.B)
    pipe_bytes = ab["pyramid"] + ab["fast"] + ab["blur"] + ab["describe"]
    images_per_s = res_dev["value"] / pl.env["world"] * (2 if pl.stereo else 1)  # this rank's images per second
    pipe_ms = stage_pipe.get(dom, 0.0) / (nlaunch if dom == "pyramid" else 1.0)
    rl = {"bound": "hbm", "kernel": kernel, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
          "frac": achieved / HBM_PEAK_GBS, "traffic": tr["bytes"] if tr else None,
          "algorithmic_bytes_per_launch": bytes_per_launch, "avg_launch_ms": ms, "avg_launch_ms_pipelined": pipe_ms,
          # all extraction stages together, algorithmic bytes per image x images/s (per rank)
          "pipeline_gbps_per_rank": pipe_bytes * images_per_s / 1e9,
          "pipeline_frac": pipe_bytes * images_per_s / 1e9 / HBM_PEAK_GBS}
    if tr and tr.get("valu_insts") and ms > 0:
        # what actually bounds the kernel: wave64 VALU instructions per launch (committed SQ_INSTS_VALU) x 1.77 ns per
        # instruction and SIMD (tools/issue_rate_probe.hip, 8 waves per SIMD) over 1024 SIMDs, against the launch time
        rl["valu_issue_frac"] = tr["valu_insts"] * VALU_NS_PER_WAVE_INST / NUM_SIMDS / (ms * 1e6)
    detail = {"traffic_detail": tr, "stage_ms_single_context": stage_alone, "stage_ms_pipelined_event_spans": stage_pipe,
              "avg_launch_ms_note": "avg_launch_ms: HIP events on the kernel's own stream, single context (nothing else on the "
                                    "GPU); avg_launch_ms_pipelined: event span inside the timed region, other streams' workgroups included",
              "pipelined_event_span_ms_of_kernel": pipe_ms, "algorithmic_bytes_per_image": pipe_bytes}
    return rl, detail


def host_cpu_description():
    """'<model name>, <n> hardware threads' of the box the CPU baseline ran on"""
    model = "unknown CPU"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return "%s, %d hardware threads" % (model, os.cpu_count() or 0)


def link_probe(nbytes):
    """Host-to-device rate of the link as this process sees it: one asynchronous copy of a pinned block of a step's size on
    an otherwise idle GPU (the DMA engines), from memory allocated the way the pipeline's pinned images are
    (vslam_host_alloc: on the CPUs next to the device).  A peak is the BEST of the 9 timed copies.  The denominator of
    roofline_pcie."""
    import torch
    import vi_slam_amd as V
    pin = V.PinnedImages(1, 1, nbytes)
    try:
        a = torch.from_numpy(pin._flat)  # torch sees hipHostMalloc memory as pinned: copy_ is one hipMemcpyAsync
        b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for i in range(12):
            e0.record()
            b.copy_(a, non_blocking=True)
            e1.record()
            e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        del a
    finally:
        torch.cuda.synchronize()
        pin.close()
    return nbytes / (min(ts) * 1e-3) / 1e9


def run_workload(name, args, env, want_cpu, cpu_seconds, headline):
    """headline: the workload of the line's `value`; --dump-outputs writes what its main region (device inputs, unless
    --inputs pinned) delivered last."""
    pl = Pipeline(name, args, env)
    try:
        inputs = args.inputs
        res = {}
        main_mode = "device" if inputs in ("device", "both") else "pinned"
        for mode in ("device", "pinned"):
            if inputs in (mode, "both"):
                pl.use_inputs(mode)
                res[mode] = pl.timed(args.steps, args.warmup, args.min_seconds if args.full else 0.0,
                                     profile=args.full and mode == main_mode,
                                     outputs=headline and mode == main_mode and bool(args.dump_outputs))
        pl.use_inputs("device")
        main = res[main_mode]
        if main["outputs"] is not None and env["rank"] == 0:
            dump_outputs(args.dump_outputs, main["outputs"])
        out = {"workload": name, "value": main["value"] if "device" in res else None,
               "value_host_inputs": res["pinned"]["value"] if "pinned" in res else None,
               "ms_per_step": main["ms_per_step"], "timed_repeats": main["reps"], "timed_seconds": main["seconds"],
               "result_transfers_per_step": main["result_transfers_per_step"], "result_bytes_per_step": main["result_bytes_per_step"],
               "spread": main.get("spread"), "spread_host_inputs": res["pinned"].get("spread") if "pinned" in res else None}
        if args.full and "pinned" in res and env["rank"] == 0:
            # the PCIe roofline of the host-input figure: image bytes that cross the link per second against what one
            # hipMemcpyAsync of a step's images achieves alone on this box, measured here
            img_bytes = pl.cfg["w"] * pl.cfg["h"] * (2 if pl.stereo else 1)
            step_bytes = pl.cfg["w"] * pl.cfg["h"] * pl.B
            peak = link_probe(step_bytes)
            ach = res["pinned"]["value"] / env["world"] * img_bytes / 1e9
            out["roofline_pcie"] = {"bound": "pcie_h2d", "achieved": ach, "peak": peak, "unit": "GB/s", "frac": ach / peak,
                                    "bytes_per_frame": img_bytes, "peak_source": "best of 9 hipMemcpyAsync of one step's images from vslam_host_alloc memory, idle GPU, this run"}
        if args.full and pl.multi:  # the exchange step alone: every rank enqueues the same 50 shifts of its last packed slot and waits once
            pl.torch.cuda.synchronize()
            env["barrier"]()
            t0 = time.perf_counter()
            for _ in range(50):
                pl.xchg.exchange(pl.ctxs[0], pl.packed[0], pl.recv[0], lane=0)
            pl.torch.cuda.synchronize()
            out["exchange"] = {"us_per_exchange_alone": env["max_over_ranks"]((time.perf_counter() - t0) / 50 * 1e6),
                               "bytes": pl.slot_bytes, "mode": pl.xchg.mode, "transport": pl.xchg.transport,
                               "lanes": len(pl.xchg.comms) if pl.xchg.comms else 0}
            if args.verify_exchange and env.get("exchange_verify") is not None:
                out["exchange"].update(env["exchange_verify"])  # proven once per process, on the first workload that exchanges
            elif args.verify_exchange:
                # the GPU-side proof for the first N > 1 run (no oracle involved), for BOTH exchange forms: the mode of the
                # timed region on its own SlotExchange, the other one on a one-lane SlotExchange built for this check
                ver = {}
                other = "allgather" if pl.xchg.mode == "ring" else "ring"
                for mode in (pl.xchg.mode, other):
                    x = pl.xchg if mode == pl.xchg.mode else pl.vd.SlotExchange.create(
                        env["rank"], env["world"], env["local_rank"], mode=mode, transport=pl.xchg.transport, lanes=1)
                    try:
                        r = pl.verify_exchange(x)
                    finally:
                        if x is not pl.xchg:
                            x.close()
                    bad = env["max_over_ranks"](0.0 if (r["ok"] and r["matcher_ok"]) else 1.0)  # every rank must agree
                    ver[mode] = {"verified": bad == 0.0, "keypoints_compared_rank0": r["n"], "matches_rank0": r["matches"],
                                 "us_first_exchange": env["max_over_ranks"](r["us"])}
                    if r["reason"]:
                        ver[mode]["reason_rank0"] = r["reason"]
                out["exchange"]["exchange_verified"] = all(v["verified"] for v in ver.values())
                out["exchange"]["verify"] = ver
                env["exchange_verify"] = {"exchange_verified": out["exchange"]["exchange_verified"], "verify": ver}
        if pl.cfg.get("real"):
            prob, deep = 0, 0
            for c in pl.ctxs:
                a, b, _ = c.octree_stats()
                prob, deep = prob + a, deep + b
            out["quadtree"] = {"problems": prob, "split_below_grid": deep, "share": deep / max(prob, 1)}
        detail = {"workload": name, "matches_last_step_rank0": pl.state["matches"],
                  "track_matches_last_step_rank0": pl.state.get("track_matches"),
                  "host_ms_per_step": main["host_ms_per_step"],
                  "ms_per_step_host_inputs": res["pinned"]["ms_per_step"] if "pinned" in res else None}
        if args.full and env["rank"] == 0:
            prof = main["prof"]
            nb = max(prof.get("batches", 0), 1)
            stage_pipe = {k: prof[v] / nb for k, v in PROF_KEY.items()} | {"octree": prof["octree_ms"] / nb}
            stage_alone = pl.single_context_stage_ms()
            rl, rd = roofline_of(pl, stage_alone, stage_pipe, main)
            out["roofline"] = rl
            detail.update(rd)
        out["config"] = {"workload": name, "frames_per_step_per_gpu": pl.B // 2 if pl.stereo else pl.B,
                         "images_per_step_per_gpu": pl.B, "nfeatures": pl.cfg["nf"], "nlevels": 8, "scale_factor": 1.2,
                         "contexts_in_flight": pl.NCTX, "distinct_frames": pl.ndistinct,
                         "match": ("ComputeStereoMatches L<->R + UnprojectStereo + SearchByProjection(prev frame) th 15" if pl.track
                                   else "ComputeStereoMatches L<->R") if pl.stereo else "SearchForInitialization(prev frame) window 100",
                         "sharding": ("blocks of consecutive frames per rank; one %s shift of each rank's last packed result slot per step (%s)" %
                                      (env["xchg"].mode if env.get("xchg") else "ring", env["xchg"].transport if env.get("xchg") else "none"))
                         if not pl.stereo else "stereo frames independent per rank, no collective"}
    finally:
        pl.close()
    if want_cpu:
        out["cpu_baseline"] = cpu_baseline(WORKLOADS[name], cpu_seconds, min(cpu_seconds, 8.0))
    return out, detail


def dump_outputs(folder, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (float32), 64 MB at most in all."""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > 64 << 20:
        raise RuntimeError("--dump-outputs: %d bytes of outputs exceed 64 MB" % total)
    os.makedirs(folder, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(folder, name + ".npy"), np.ascontiguousarray(a, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (with --full: steps per block, see --min-seconds)")
    ap.add_argument("--warmup", type=int, default=5,
                    help="untimed steps before the region (without --full: at least that many, and %.1f s of them)" % WARMUP_SECONDS)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: host inputs, the extra workloads, CPU baselines, roofline and per-stage "
                         "figures, the PCIe roofline, and for N>1 the exchange alone and its GPU-side proof; every timed region "
                         "then repeats its --steps steps until it lasts --min-seconds")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the headline region's last step delivered as DIR/<name>.npy (float32)")
    ap.add_argument("--workload", default="all", choices=["all"] + sorted(WORKLOADS),
                    help="'all' = the headline workload (with --full: plus the extra workloads in one line)")
    ap.add_argument("--inputs", default=None, choices=["device", "pinned", "both"],
                    help="where the frames are when the timed region starts: HBM, pinned host memory, or both (two timed regions); "
                         "default device, with --full both")
    ap.add_argument("--min-seconds", type=float, default=1.0,
                    help="with --full: every timed region repeats its --steps steps until it lasts this long (without --full "
                         "the timed region is exactly --steps steps)")
    ap.add_argument("--batch", type=int, default=32, help="images (stereo: L,R,L,R..) per rank per step")
    ap.add_argument("--inflight", type=int, default=4, help="extractor contexts (HIP streams) in flight per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="headline workload only")
    ap.add_argument("--no-exchange-chain", dest="exchange_chain", action="store_false",
                    help="N>1: let the lanes' exchanges overlap instead of ordering them by events (A/B)")
    ap.add_argument("--delivery", default="single", choices=["single", "separate"],
                    help="mono workload: extraction and matcher results in one device-to-host transfer per step, or one each")
    ap.add_argument("--upload-split", type=int, default=0,
                    help="host inputs: 1 = a step's upload goes as two transfers and the chain event sits between them")
    ap.add_argument("--upload-chain", type=int, default=1,
                    help="host inputs: upload of step t waits (GPU-side event) for the upload of step t-L; 0 = no pacing")
    ap.add_argument("--fast-chain", default="auto", choices=["auto", "on", "off"],
                    help="chain the contexts' FAST launches (vslam_fe_set_fast_gate); auto = the workloads whose contexts are coupled "
                         "by a cross-frame matcher anyway (A/B: profiles/r04_fast_chain_ab.txt)")
    ap.add_argument("--gc", action="store_true", help="leave Python's cyclic garbage collector on inside the timed region (A/B)")
    ap.add_argument("--stamp-dump", default="", help="write the host clock of every step's enqueue and wait to PREFIX.<workload>.<inputs>.json")
    ap.add_argument("--stream-priority", type=int, default=2, choices=[0, 1, 2],
                    help="vslam_tuning.stream_priority of the extractor contexts (0 normal, 1 low, 2 high)")
    ap.add_argument("--fast-kernel", type=int, default=-1, help="vslam_tuning.fast_kernel (3 cells, 4 bands; -1 library default)")
    ap.add_argument("--wave-prio", type=int, default=-1, help="vslam_tuning.wave_prio bit mask (-1 library default)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo (slots staged through host memory) only exists to rehearse the N>1 path on one GPU")
    ap.add_argument("--same-gpu", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--exchange", default="ring", choices=["ring", "allgather"],
                    help="N>1 exchange step: ring shift (ncclSend/ncclRecv pair) or the north_star-literal all-gather")
    ap.add_argument("--no-verify-exchange", dest="verify_exchange", action="store_false",
                    help="skip the untimed GPU-side proof of the exchange (on by default whenever the exchange runs)")
    ap.add_argument("--force-collective", action="store_true",
                    help="take the N>1 code path (pack + exchange on the extractor stream) at world size 1")
    ap.add_argument("--print-launch", action="store_true", help="with --gpus N and no launcher: print the launch command, do not run")
    ap.add_argument("--launch-check", action="store_true",
                    help="spawned ranks only rendezvous (gloo, no GPU touched), all-reduce and exit: tests the self-launch")
    args = ap.parse_args()
    if args.inputs is None:
        args.inputs = "both" if args.full else "device"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))  # before anything touches the GPU
    if world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)

    # stdout carries ONE line, the result: whatever libraries print to file descriptor 1 from here on (RCCL's version banner
    # under NCCL_DEBUG=VERSION, for one) goes to stderr; the JSON line is written to the saved descriptor at the end
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist

    if args.launch_check:
        dist.init_process_group("gloo")
        t = torch.tensor([rank + 1.0])
        dist.all_reduce(t)
        dist.barrier()
        if rank == 0:
            os.write(result_fd, (json.dumps({"launch_check": "ok", "world": world, "sum_of_ranks_plus_1": float(t.item())}) + "\n").encode())
        dist.destroy_process_group()
        return

    import vi_slam_amd as V
    from vi_slam_amd import dist as vd

    if args.same_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    need_group = world > 1 or args.force_collective
    if need_group:
        if world == 1:  # --force-collective without a launcher: a one-rank group
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(free_port()))
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")

    ctl_dev = "cuda" if (need_group and args.dist_backend == "nccl") else "cpu"

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=ctl_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    env = {"rank": rank, "world": world, "local_rank": local_rank, "barrier": barrier, "max_over_ranks": max_over_ranks}
    if need_group:
        # the exchange transport and mode are chosen ONCE, before any timed work, by a probe every rank agrees on
        env["xchg"] = vd.SlotExchange.create(rank, world, local_rank, mode=args.exchange,
                                             transport="rccl" if args.dist_backend == "nccl" else "gloo",
                                             lanes=max(3, args.inflight))  # one communicator per context in flight

    names = [HEADLINE] + ([] if args.no_extras or not args.full else EXTRAS) if args.workload == "all" else [args.workload]
    results, details = [], []
    for i, name in enumerate(names):
        want_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
        out, det = run_workload(name, args, env, want_cpu, 12.0 if i == 0 else 6.0, i == 0)  # bounded CPU samples: five workloads in one run
        results.append(out)
        details.append(det)
        barrier()

    if rank == 0:
        head = results[0]
        rl = {k: sig(v) for k, v in head.get("roofline", {}).items()}
        line = {
            "metric": "frames/sec ORB extract+match",
            "value": sig(head["value"] if head["value"] is not None else head["value_host_inputs"], 6),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": sig(head["ms_per_step"]),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "inputs": ("value: frames resident in HBM when the timed region starts (the bench contract's definition); value_host_inputs: "
                       "the SURVEY 8(d) span -- frames in pinned host memory, H2D over PCIe inside the step (roofline_pcie); results D2H in both"),
            "value_device_inputs": sig(head["value"], 6),
            "value_host_inputs": sig(head["value_host_inputs"], 6),
            "spread": {k: sig(v) for k, v in (head.get("spread") or {}).items()},
            "spread_host_inputs": {k: sig(v) for k, v in (head.get("spread_host_inputs") or {}).items()},
            "timed_repeats": head["timed_repeats"],
            "timed_seconds": sig(head["timed_seconds"], 4),
            "result_delivery": {"transfers_per_step": sig(head["result_transfers_per_step"], 3),
                                "bytes_per_step": sig(head["result_bytes_per_step"], 6), "mode": args.delivery},
            "config": head["config"],
            "roofline": rl,
        }
        if "exchange" in head:
            line["exchange"] = {k: sig(v) for k, v in head["exchange"].items()}
            if "exchange_verified" in head["exchange"]:
                line["exchange_verified"] = head["exchange"]["exchange_verified"]
        if "roofline" in head:
            line["hbm_gbps_per_rank"] = sig(head["roofline"].get("pipeline_gbps_per_rank"))
        if "roofline_pcie" in head:
            line["roofline_pcie"] = {k: sig(v) for k, v in head["roofline_pcie"].items()}
        if "cpu_baseline" in head:
            cb = head["cpu_baseline"]
            line["cpu_baseline"] = {"value": sig(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                                    "sample": cb["sample"]}
            if "all_cores" in cb:
                line["cpu_baseline"]["all_cores"] = {"value": sig(cb["all_cores"]["value"]), "cores": cb["all_cores"]["cores"]}
            line["cpu_baseline"]["host"] = host_cpu_description()  # CPU model and thread count beside the number
        extras = []
        for r in results[1:]:
            e = {"workload": r["workload"], "value": sig(r["value"], 6), "value_host_inputs": sig(r["value_host_inputs"], 6),
                 "unit": "frames/s", "ms_per_step": sig(r["ms_per_step"]),
                 "frames_per_step_per_gpu": r["config"]["frames_per_step_per_gpu"]}
            if "roofline" in r:
                e["roofline"] = {k: sig(r["roofline"][k]) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic",
                                                                   "avg_launch_ms", "pipeline_gbps_per_rank")}
            if "roofline_pcie" in r:
                e["roofline_pcie"] = {k: sig(r["roofline_pcie"][k]) for k in ("achieved", "peak", "unit", "frac")}
            if r.get("result_transfers_per_step") is not None:
                e["result_transfers_per_step"] = sig(r["result_transfers_per_step"], 3)
            for k in ("spread", "spread_host_inputs"):
                if r.get(k):
                    e[k] = {a: sig(b, 4) for a, b in r[k].items() if a != "blocks"}
            if "quadtree" in r:
                e["quadtree"] = {k: sig(v, 3) for k, v in r["quadtree"].items()}
            if "cpu_baseline" in r:
                cb = r["cpu_baseline"]
                e["cpu_baseline"] = {"value": sig(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                                     "sample": cb["sample"].split(":")[0]}
                if "all_cores" in cb:
                    e["cpu_baseline"]["all_cores"] = {"value": sig(cb["all_cores"]["value"]), "cores": cb["all_cores"]["cores"]}
                e["speedup_vs_cpu_port"] = sig((r["value_host_inputs"] or r["value"]) / cb["value"], 4)
            extras.append(e)
        if extras:
            line["extra_workloads"] = extras
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(line) + "\n").encode())
        print(json.dumps({"bench_detail": details}), file=sys.stderr)
    if env.get("xchg"):
        env["xchg"].close()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
