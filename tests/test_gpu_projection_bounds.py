"""GPU (-m gpu): the SearchByProjection forms, Fuse and SearchBySim3 over the context's float grid bounds
(vslam_fe_set_grid_bounds) vs tests/projection_bounds_ref.py, bit-exact, on distorted cameras whose undistorted keypoints
and projections leave [0, w] x [0, h] (tests/test_projection_bounds_cpu.py asserts that of the inputs)."""
import numpy as np
import pytest

import projection_bounds_cases as PC
import projection_bounds_ref as R
import undistort_ref as U
import vi_slam_amd as V
from conftest import kp_equal

pytestmark = pytest.mark.gpu

CAMS = sorted(PC.SIZES)


@pytest.fixture(scope="module", params=CAMS)
def ctx(request):
    """one context per camera: both frames extracted with the camera set, slots 0 / 1 hold their ukeypoints_"""
    c = PC.make_case(request.param)
    fe = V.FExtractor(PC.NF, 1.2, 8, 20, 7, c["W"], c["H"], max_batch=2)
    fe.set_camera(*c["K"], dist=c["D"])
    res = fe.compute_batch([c["img0"], c["img1"]])
    assert kp_equal(res[0][0], c["k0"]) and kp_equal(res[1][0], c["k1"])
    assert kp_equal(fe.ukeypoints(0), c["uk0"]) and kp_equal(fe.ukeypoints(1), c["uk1"])
    assert np.array_equal(fe.image_bounds(), c["bounds"])
    dev = [(fe.slot_ukps_ptr(s), fe.slot_dev_ptrs(s)[1], fe.slot_dev_ptrs(s)[2]) for s in (0, 1)]
    yield dict(c=c, fe=fe, dev=dev)
    fe.close()


@pytest.fixture
def with_bounds(ctx):
    ctx["fe"].set_grid_bounds(ctx["c"]["bounds"])
    yield ctx
    ctx["fe"].set_grid_bounds(None)
    ctx["fe"].set_tuning(sbp_sequential=0, sbp_topm=8)


def device(ctx, matcher, s, occupied=None):
    """the run `s` of PC.RUNS on the device, in the shape PC.reference returns it"""
    c, fe = ctx["c"], ctx["fe"]
    fx, fy, cx, cy = c["K"]
    size = (c["W"], c["H"])
    (k0p, d0p, _), (k1p, d1p, _) = ctx["dev"]
    n0, n1 = len(c["uk0"]), len(c["uk1"])
    Tcw = c["shift"]
    Ow = (-Tcw[:, :3].T @ Tcw[:, 3]).astype(np.float32)
    if matcher == "frame":
        m = V.FMatcher(fe, 0.9, s["ori"])
        return m.SearchByProjection(PC.frame_pose(c, s["T"]), PC.pose(), (fx, fy, cx, cy, 0.0, PC.MB), s["th"], c["uk0"],
                                    np.full(n0, 3, np.uint8), c["X"], c["d0"], k1p, d1p, n1, None, s["mono"], size, occupied,
                                    s["gf"])
    if matcher == "keyframe":
        m = V.FMatcher(fe, 0.9, s["ori"])
        return m.SearchByProjectionKeyFrame(Tcw, Ow, (fx, fy, cx, cy), s["th"], s["orb"], PC.LSF, c["uk0"],
                                            np.ones(n0, np.uint8), c["X"], c["mn"], c["mx"], c["d0"], k1p, d1p, n1, occupied,
                                            size, s["gf"])
    pk, pd = PC.kf_points(c, s)  # the MapPoints of the KeyFrame-side forms
    if matcher == "sim3proj":
        m = V.FMatcher(fe, 0.9, True)
        return m.SearchByProjectionSim3(Tcw, Ow, (fx, fy, cx, cy), s["th"], s["ratio"], PC.LSF, np.ones(len(pk), np.uint8),
                                        pk["pos"], pk["normal"], pk["min_distance"], pk["max_distance"], pd, k1p, d1p, n1,
                                        None, size, s["variant"], s["gf"])
    if matcher == "mappoints":
        m = V.FMatcher(fe, s["nnratio"], True)
        return m.SearchByProjectionMapPoints(c["mps"], c["d0"], k1p, d1p, n1, None, s["th"], occupied, size)
    if matcher == "fuse":
        m = V.FMatcher(fe, 0.6, True)
        bi, bd = m.FuseSearch(pk, pd, k1p, d1p, n1, None, Tcw[:, :3], Tcw[:, 3], Ow, (fx, fy, cx, cy, 0.0), s["th"],
                              PC.LSF, size, s["sim3"], s["gf"])
        return bi, bd
    if matcher == "sim3dir":
        m = V.FMatcher(fe, 0.75, True)
        I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        b1, e1 = m.FuseSearch(pk, pd, k1p, d1p, n1, None, I3, z3, z3, (fx, fy, cx, cy, 0.0), s["th"], PC.LSF, size, 2, s["gf"],
                              I3, c["t2w"])
        return (np.where((b1 >= 0) & (e1 <= 100), b1, -1),)
    if matcher == "sim3":
        m = V.FMatcher(fe, 0.75, True)
        I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        R12, t12, sR12, sR21, t21 = PC.sim3_transforms(c["t2w"])
        n, m12, _ = m.SearchBySim3(pk, pd, k0p, d0p, n0, I3, z3, c["pts2"], c["d1"], k1p, d1p, n1, I3, c["t2w"], 1.0,
                                   R12, t12, s["th"], (fx, fy, cx, cy), PC.LSF, size, s["gf"])
        # the two directions themselves (vslam_fuse_search with sim3 = 2), before the agreement check
        camb = (fx, fy, cx, cy, 0.0)
        b1, e1 = m.FuseSearch(pk, pd, k1p, d1p, n1, None, I3, z3, z3, camb, s["th"], PC.LSF, size, 2, s["gf"], sR21,
                              t21)
        b2, e2 = m.FuseSearch(c["pts2"], c["d1"], k0p, d0p, n0, None, I3, c["t2w"], z3, camb, s["th"], PC.LSF, size, 2, s["gf"],
                              sR12, t12)
        return n, m12, np.where((b1 >= 0) & (e1 <= 100), b1, -1), np.where((b2 >= 0) & (e2 <= 100), b2, -1)
    raise KeyError(matcher)


def expect(c, matcher, s, bounds, occupied=None):
    w = PC.reference(c, matcher, s, bounds, occupied=occupied)
    if matcher == "fuse":  # the device clamps a found distance to 255 (its key field); 256 = nothing found
        return w[0], np.minimum(w[1], np.where(w[0] >= 0, 255, 256))
    return w


@pytest.mark.parametrize("run", range(len(PC.RUNS)))
def test_matchers_over_float_bounds_equal_reference(with_bounds, run):
    matcher, s = PC.RUNS[run]
    c = with_bounds["c"]
    got = device(with_bounds, matcher, s)
    want = expect(c, matcher, s, c["bounds"])
    assert PC.same(got, want), (c["name"], matcher, s)


@pytest.mark.parametrize("tune", [dict(sbp_sequential=1), dict(sbp_topm=1), dict(sbp_topm=2)])
def test_sequential_and_short_prefix_paths_over_float_bounds(with_bounds, tune):
    """the replay kernels (k_sbp_replay / k_sbpm_replay) and their full re-scans take the same grid"""
    c, fe = with_bounds["c"], with_bounds["fe"]
    fe.set_tuning(**tune)
    rng = np.random.default_rng(5)
    occ = (rng.random(len(c["uk1"])) < 0.2).astype(np.uint8)
    m = V.FMatcher(fe, 0.9, True)
    m.search_init_fallbacks()
    for matcher, s in (("frame", dict(T="shift", th=30, gf=False, ori=True, mono=False)),
                       ("keyframe", dict(th=20, orb=80, gf=False, ori=True)),
                       ("sim3proj", dict(th=8, ratio=1.5, variant=0, gf=False)),
                       ("mappoints", dict(th=5.0, nnratio=0.8))):
        for occupied in (None, occ) if matcher != "sim3proj" else (None,):
            got = device(with_bounds, matcher, s, occupied)
            assert PC.same(got, expect(c, matcher, s, c["bounds"], occupied)), (c["name"], matcher, tune)
    if "sbp_topm" in tune:
        assert m.search_init_fallbacks() > 0


def test_device_resident_chain_on_a_distorted_camera(ctx):
    """set_camera -> extraction of two frames -> image_bounds -> set_grid_bounds -> SearchByProjection of two jobs in one
    call on the slots' ukeypoints_ and device counts, nothing read back in between"""
    import torch
    c = ctx["c"]
    W, H = c["W"], c["H"]
    fx, fy, cx, cy = c["K"]
    fe = V.FExtractor(PC.NF, 1.2, 8, 20, 7, W, H, max_batch=2)
    try:
        fe.set_camera(fx, fy, cx, cy, dist=c["D"])
        pitch = (W + 127) // 128 * 128
        dev = torch.zeros((2, H, pitch), dtype=torch.uint8, device="cuda")
        dev[0, :, :W] = torch.from_numpy(c["img0"]).cuda()
        dev[1, :, :W] = torch.from_numpy(c["img1"]).cuda()
        torch.cuda.synchronize()
        fe.compute_batch_async([dev[i].data_ptr() for i in range(2)], pitch, to_host=False)
        b = fe.image_bounds()
        fe.set_grid_bounds(b)
        assert fe.grid_bounds()[1] and np.array_equal(fe.grid_bounds()[0], c["bounds"])
        n0 = len(c["uk0"])
        flags = torch.from_numpy(np.full(fe.cap, 3, np.uint8)).cuda()
        Xp = np.zeros((fe.cap, 3), np.float32)
        Xp[:n0] = c["X"]
        X = torch.from_numpy(Xp).cuda()
        (_, d0p, n0p), (_, d1p, n1p) = fe.slot_dev_ptrs(0), fe.slot_dev_ptrs(1)
        k0p, k1p = fe.slot_ukps_ptr(0), fe.slot_ukps_ptr(1)
        runs = [dict(T="shift", th=15, gf=False), dict(T="fwd", th=15, gf=True)]
        jobs = []
        for s in runs:
            T = PC.frame_pose(c, s["T"])
            fwd, bwd = R.projection_direction(T, PC.pose(), PC.MB, False, not s["gf"])
            jobs.append(dict(Tcw=T, cam=(fx, fy, cx, cy, 0.0), th=s["th"], forward=fwd, backward=bwd, img=(W, H),
                             gemm_float=s["gf"], last_kps=k0p, n_last=n0p, last_flags=flags.data_ptr(),
                             last_x3dw=X.data_ptr(), mp_desc=d0p, cur_kps=k1p, cur_desc=d1p, n_cur=n1p))
        m = V.FMatcher(fe, 0.9, True)
        m.search_by_projection_dev_async(jobs)
        counts = fe.wait()  # the extraction results stay on the device
        out = m.search_by_projection_dev_wait([counts[1][0]] * len(runs))
        uk0, uk1 = fe.ukeypoints(0), fe.ukeypoints(1)
        assert kp_equal(uk0, c["uk0"]) and kp_equal(uk1, c["uk1"])
        mono = np.full(len(uk1), -1, np.float32)
        for (nm, mc), s in zip(out, runs):
            wn, wm, _ = R.search_by_projection_frame(PC.frame_pose(c, s["T"]), PC.pose(), (fx, fy, cx, cy, 0.0, PC.MB), s["th"],
                                                     uk0, np.full(n0, 3, np.uint8), c["X"], c["d0"], uk1, c["d1"], mono,
                                                     c["sf"], b, False, True, None, not s["gf"])
            assert nm == wn and np.array_equal(mc, wm), s
            assert wn > 100
            ni = R.search_by_projection_frame(PC.frame_pose(c, s["T"]), PC.pose(), (fx, fy, cx, cy, 0.0, PC.MB), s["th"], uk0,
                                              np.full(n0, 3, np.uint8), c["X"], c["d0"], uk1, c["d1"], mono, c["sf"],
                                              PC.int_bounds(c), False, True, None, not s["gf"])
            if s is runs[0]:  # the run tests/test_projection_bounds_cpu.py::test_the_gpu_inputs_bite vouches for
                assert not np.array_equal(ni[1], wm)
    finally:
        fe.close()


def _all_entry_points(ctx):
    """every affected entry point once, device-resident batch form included -> list of result tuples"""
    c, fe = ctx["c"], ctx["fe"]
    out = [device(ctx, matcher, s) for matcher, s in PC.RUNS]
    import torch
    fx, fy, cx, cy = c["K"]
    n0 = len(c["uk0"])
    flags = torch.from_numpy(np.full(n0, 3, np.uint8)).cuda()
    X = torch.from_numpy(np.ascontiguousarray(c["X"])).cuda()
    kp = torch.from_numpy(c["uk0"].view(np.uint8).reshape(n0, -1).copy()).cuda()
    cnt = torch.tensor([n0], dtype=torch.int32, device="cuda")
    (_, d0p, _), (k1p, d1p, n1p) = ctx["dev"]
    jobs = [dict(Tcw=PC.frame_pose(c, t), cam=(fx, fy, cx, cy, 0.0), th=15, forward=0, backward=0, img=(c["W"], c["H"]),
                 last_kps=kp.data_ptr(), n_last=cnt.data_ptr(), last_flags=flags.data_ptr(), last_x3dw=X.data_ptr(),
                 mp_desc=d0p, cur_kps=k1p, cur_desc=d1p, n_cur=n1p) for t in ("shift", "fwd")]
    m = V.FMatcher(fe, 0.9, True)
    m.search_by_projection_dev_async(jobs)
    out += [(n, mc.copy()) for n, mc in m.search_by_projection_dev_wait([len(c["uk1"])] * 2)]
    return out


def test_identity_bounds_and_reset_are_bit_equal_to_no_bounds(ctx):
    c, fe = ctx["c"], ctx["fe"]
    assert not fe.grid_bounds()[1]
    base = _all_entry_points(ctx)
    try:
        fe.set_grid_bounds(PC.int_bounds(c))
        same = _all_entry_points(ctx)
        fe.set_grid_bounds(c["bounds"])
        other = _all_entry_points(ctx)
        fe.set_grid_bounds(None)
        back = _all_entry_points(ctx)
    finally:
        fe.set_grid_bounds(None)
    assert len(base) == len(PC.RUNS) + 2
    for i, (a, b, o, r) in enumerate(zip(base, same, other, back)):
        assert PC.same(a, b), i
        assert PC.same(a, r), i
    assert not all(PC.same(a, o) for a, o in zip(base, other))
    # the no-bounds results are the integer-image ones
    for (matcher, s), a in list(zip(PC.RUNS, base))[::3]:
        assert PC.same(a, expect(c, matcher, s, PC.int_bounds(c))), (matcher, s)


def test_grid_bounds_arguments(ctx):
    c, fe = ctx["c"], ctx["fe"]
    b, is_set = fe.grid_bounds()
    assert not is_set and np.array_equal(b, np.array([0, c["W"], 0, c["H"]], np.float32))
    good = np.array([-3.5, c["W"] + 2.25, -1.0, c["H"] + 7.0], np.float32)
    try:
        fe.set_grid_bounds(good)
        for bad in ((np.nan, 10, 0, 10), (0, np.inf, 0, 10), (0, 10, -np.inf, 10), (5, 5, 0, 10), (0, 10, 7, 3),
                    (10, 0, 0, 10)):
            with pytest.raises(V.VslamError) as e:
                fe.set_grid_bounds(bad)
            assert e.value.code == V.ERR_INVALID
            b, is_set = fe.grid_bounds()
            assert is_set and np.array_equal(b, good)  # the previous setting stays in force
        fe.set_grid_bounds(None)
        b, is_set = fe.grid_bounds()
        assert not is_set and np.array_equal(b, np.array([0, c["W"], 0, c["H"]], np.float32))
        with pytest.raises(V.VslamError):  # and an invalid one while none is set leaves none set
            fe.set_grid_bounds((0, 0, 0, 0))
        assert not fe.grid_bounds()[1]
    finally:
        fe.set_grid_bounds(None)
