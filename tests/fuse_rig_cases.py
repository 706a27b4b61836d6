"""Deterministic inputs of the rig Fuse tests (the search half of FMatcher::Fuse(pKF, vpMapPoints, th, bRight) for a fisheye
KeyFrame / a two-fisheye rig): tests/test_fuse_rig_cpu.py, tests/test_gpu_fuse_rig.py, tests/test_cpp_fuse_rig.py,
tests/tools/dump_fuse_rig_cases.py, tests/tools/time_fuse_rig.py.

Keypoints and descriptors of the realistic cases are the committed golden's (tests/golden/pipeline_hut_320x240.npz): kL / dL as
the left camera (456 keypoints), kR / dR as the right one (457).  The two KB8 cameras have DIFFERENT calibrations (CAM1 =
kb8_cases.LOCAL_CAM, CAM2) and the rig a real Tlr (kb8_cases.rig(): the right camera 10 cm to the right, looking 50 degrees
away), so that projecting the right job through the left model, or with the left pose, changes results.

A KeyFrame is its left pose; the right camera's pose is Trl * Tcw.  A job is what tests/fuse_rig_ref.py takes:
dict(pose, left_pose, camera, sim3, kps, desc, idx_offset, valid).

cases() -> name -> dict(jobs, pts (FUSE_POINT_DTYPE), desc, th, gf, refuse (None or the error the device entry answers with))
  scene            ~1400 MapPoints against 3 KeyFrames = 6 jobs (left job of a KeyFrame before its right job)
  hand             hand-made keypoints (26 left, 5 right) and 28 MapPoints: every gate on both sides, the image boundary hit
                   exactly, ties across and within cells, the chi2 band between 5.99 and 7.8, a sim3 job with the far rule
  np1 .. np17      the scene's first 1 / 15 / 16 / 17 points against its first KeyFrame (2 jobs)
  jobs1, jobs16    1 job; 16 jobs (the scene's six, cycled, every one with validity bytes of its own)
  empty_job        a job with n_kf == 0 between two ordinary ones
  no_points        n_points == 0
  kf4096           a job with 4096 keypoints (the golden's left ones, tiled: whole windows of equal distances)
  kf4097, jobs17   refused: VSLAM_ERR_UNSUPPORTED / VSLAM_ERR_INVALID
  mono             a monocular fisheye KeyFrame: one job, camera 0, offset 0
  sim3             one sim3 job over the scene's points
  gemm_float       the scene's first KeyFrame with gemm_float
reference(name) evaluates a case with the numpy restatement (cached) -> (best_idx, best_dist, census)."""
import os

import numpy as np

import frustum_cases as FC
import fuse_rig_ref as FR
import kb8_cases as KC
import kb8_ref as KR
from oracle import orbo

F32 = np.float32
BOUNDS = (0.0, float(FC.HUT_W), 0.0, float(FC.HUT_H))
IMG = (FC.HUT_W, FC.HUT_H)
CAM1 = KC.LOCAL_CAM
CAM2 = (121.5, 120.75, 161.25, 118.5, KC.K_STRONG, 0.0)
TH = 3.0
LSF = float(FC.LSF)
_cache = {}


def golden():
    if "g" not in _cache:
        p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
        tab = orbo.Extractor(FC.HUT_NF).tables()
        rig = KC.rig()
        rig["cam2"] = KR.camera(*CAM2)
        _cache["g"] = dict(kl=p["kL"], dl=p["dL"], kr=p["kR"], dr=p["dR"], sf=np.asarray(tab["scale"], F32),
                           is2=np.asarray(tab["inv_sigma2"], F32), cams=(KR.camera(*CAM1), KR.camera(*CAM2)), rig=rig)
    return _cache["g"]


def right_pose(T):
    """(Rcw, tcw, Ow) of the right camera of a KeyFrame whose left pose is T: GetRightRotation / Translation / CameraCenter"""
    Trl = np.asarray(golden()["rig"]["Trl"], np.float64)
    T = np.asarray(T, np.float64)
    R = Trl[:, :3] @ T[:, :3]
    t = Trl[:, :3] @ T[:, 3] + Trl[:, 3]
    return _pose(np.hstack([R, t.reshape(3, 1)]))


def _pose(T):
    T, Ow = FC.pose(np.asarray(T)[:, :3], np.asarray(T)[:, 3])
    return (np.ascontiguousarray(T[:, :3]), np.ascontiguousarray(T[:, 3]), Ow)


def keyframe_jobs(T, kl, dl, kr, dr, valid=(None, None)):
    """the left and the right job of one rig KeyFrame, in the reference's call order"""
    left, right = _pose(T), right_pose(T)
    return [dict(pose=left, left_pose=left, camera=0, sim3=False, kps=kl, desc=dl, idx_offset=0, valid=valid[0]),
            dict(pose=right, left_pose=left, camera=1, sim3=False, kps=kr, desc=dr, idx_offset=0 if kl is None else len(kl),
                 valid=valid[1])]


def world_point(job, px, z):
    """the world point that the job's camera sees at pixel px, the ray scaled by z"""
    cam = golden()["cams"][job["camera"]]
    ray, _, _ = KR.unproject(cam, np.array([px], F32))
    R, t, _ = job["pose"]
    xc = ray[0].astype(np.float64) * z
    return ((xc - t.astype(np.float64)) @ R.astype(np.float64)).astype(F32)


def max_for_level(d, level):
    """a maxDistance for which MapPoint::PredictScale gives `level`, away from its rounding edges"""
    return F32(d) if level == 0 else F32(float(d) * 1.2 ** (level - 0.5))


def fuse_point(job, pos, level, valid=1, away=False, mn=0.6, mx=None):
    """a vslam_fuse_point at pos that looks at the job's camera and predicts `level` there"""
    p = np.zeros((), orbo.FUSE_POINT_DTYPE)
    pos = np.asarray(pos, F32)
    po = pos.astype(np.float64) - job["pose"][2].astype(np.float64)
    d = float(np.linalg.norm(po))
    p["pos"] = pos
    p["normal"] = ((-po if away else po) / max(d, 1e-9)).astype(F32)
    p["min_distance"] = F32(mn * d)
    p["max_distance"] = max_for_level(d, level) if mx is None else F32(mx * d)
    p["valid"] = valid
    return p


def project(job, pos, gemm_double=True):
    """(u, v) of a world point in the job's camera, by the restatement's own arithmetic"""
    from projection_bounds_ref import _gemm_row
    R, t, _ = job["pose"]
    pc = np.array([[_gemm_row(R[r], pos, t[r], gemm_double) for r in range(3)]], F32)
    uv = KR.project(golden()["cams"][job["camera"]], pc)
    return F32(uv[0, 0]), F32(uv[0, 1])


def flip(desc, k, start=0):
    """the descriptor at Hamming distance exactly k: bits [start, start + k) flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + k] ^= 1
    return np.packbits(bits)


# ------------------------------------------------------------------------------------------------ the realistic scene
def scene_poses():
    return [np.asarray(FC.pose(FC.rotation(*r), t)[0], F32) for r, t in (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                                                                        ((0.004, -0.006, 0.003), (0.03, -0.01, 0.04)),
                                                                        ((-0.005, 0.008, -0.002), (-0.04, 0.02, 0.03)))]


def scene():
    """MapPoints on the rays of the keypoints of three KeyFrames' cameras (one descriptor bit off the keypoint's) and 180 points
    scattered around them; one point in 13 is bad, and every KeyFrame already holds some of the points"""
    if "scene" in _cache:
        return _cache["scene"]
    g = golden()
    rng = np.random.default_rng(71)
    jobs = []
    for T in scene_poses():
        jobs += keyframe_jobs(T, g["kl"], g["dl"], g["kr"], g["dr"])
    pts, desc = [], []
    for k, (step, first) in enumerate(((2, 0), (2, 1), (3, 0))):
        for job in jobs[2 * k:2 * k + 2]:
            kps, dd = job["kps"], job["desc"]
            for i in range(first, len(kps), step):
                pos = world_point(job, (kps["x"][i], kps["y"][i]), rng.uniform(2.0, 6.0))
                pts.append(fuse_point(job, pos, int(kps["octave"][i])))
                d = dd[i].copy()
                d[i % 32] ^= np.uint8(1 << (i % 8))
                desc.append(d)
    T0, Ow0 = FC.pose(np.eye(3), np.zeros(3))
    junk = FC.random_points(rng, 180, T0, Ow0, spread=2.6, zr=(-1.5, 9.0))
    for q in junk:
        p = np.zeros((), orbo.FUSE_POINT_DTYPE)
        p["pos"], p["normal"], p["min_distance"], p["max_distance"], p["valid"] = q["pos"], q["normal"], q["min_dist"], \
            q["max_dist"], 1
        pts.append(p)
        desc.append(rng.integers(0, 256, 32).astype(np.uint8))
    order = rng.permutation(len(pts))
    pts = np.array(pts, orbo.FUSE_POINT_DTYPE)[order]
    desc = np.array(desc, np.uint8)[order]
    pts["valid"] = np.where(np.arange(len(pts)) % 13 == 5, 0, pts["valid"])
    for k, job in enumerate(jobs):  # IsInKeyFrame: the left and the right job of a KeyFrame share it; the last KeyFrame has none
        job["valid"] = None if k >= 4 else (rng.random(len(pts)) > 0.1 + 0.1 * (k // 2)).astype(np.uint8)
    jobs[1]["valid"] = jobs[0]["valid"]
    jobs[3]["valid"] = jobs[2]["valid"]
    _cache["scene"] = dict(jobs=jobs, pts=pts, desc=desc, th=TH, gf=False, refuse=None)
    return _cache["scene"]


# ------------------------------------------------------------------------------------------------ the hand-made case
def _solve_u(cam, target, toward):
    """a camera-frame point (x, 0, z) whose KannalaBrandt8 projection has u == target EXACTLY (toward = -1: left of the
    principal point, psi = pi; +1: right of it, psi = 0)"""
    fx, cx, k = float(cam["fx"]), float(cam["cx"]), [float(v) for v in cam["k"]]
    r = abs(float(target) - cx) / fx
    th = r
    for _ in range(50):
        f = th + k[0] * th**3 + k[1] * th**5 + k[2] * th**7 + k[3] * th**9 - r
        th -= f / (1 + 3 * k[0] * th**2 + 5 * k[1] * th**4 + 7 * k[2] * th**6 + 9 * k[3] * th**8)
    for z in (1.0, 0.5, 2.0, 1.5, 0.75, 3.0, 1.25):
        x0 = np.array([toward * np.tan(th) * z], F32)
        xs = (x0.view(np.int32)[0] + np.arange(-20000, 20001, dtype=np.int32)).astype(np.int32).view(F32)
        pc = np.stack([xs, np.zeros_like(xs), np.full_like(xs, z)], 1)
        u = KR.project(cam, pc)[:, 0]
        hit = np.nonzero(u == F32(target))[0]
        if len(hit):
            return pc[hit[len(hit) // 2]]
    raise AssertionError("no camera point projects to u == %r" % (target,))


def hand():
    """-> the case, and `why`: point index -> the census entry (or switch) it is there for"""
    if "hand" in _cache:
        return _cache["hand"]
    g = golden()
    rng = np.random.default_rng(72)
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    jl, jr = keyframe_jobs(I, None, None, None, None)
    sim = dict(jl, sim3=True)
    kps = {0: [], 1: []}   # camera -> [(x, y, octave, descriptor)]
    pts, desc, why = [], [], {}

    def rnd():
        return rng.integers(0, 256, 32).astype(np.uint8)

    def add(job, pos, level, name, d=None, **kw):
        pts.append(fuse_point(job, pos, level, **kw))
        desc.append(rnd() if d is None else d)
        why[len(pts) - 1] = name
        return project(job, pos)

    def key(cam_i, x, y, octave, d):
        kps[cam_i].append((F32(x), F32(y), octave, d))

    def matched(job, px, level, name, dx=0.5, dy=0.5, bits=1, octave=None, z=3.0, **kw):
        """a point at pixel px of the job's camera and ONE keypoint beside its projection"""
        d = rnd()
        u, v = add(job, world_point(job, px, z), level, name, d, **kw)
        key(job["camera"], u + F32(dx), v + F32(dy), level if octave is None else octave, flip(d, bits))
        return u, v

    for job in (jl, jr):  # the gates, on both sides
        c = job["camera"]
        s = "L" if c == 0 else "R"
        matched(job, (40, 40), 0, "match" + s)
        matched(job, (60, 40), 0, "invalid_point" + s, valid=0)
        matched(job, (80, 40), 1, "above_th_low" + s, bits=60)
    # left only from here: 36 px apart and more, so that no window holds another point's keypoints
    add(jl, (0.3, 0.2, -1.0), 0, "z_negative")
    d = rnd()
    u, v = add(jl, (-0.8, -0.6, 0.0), 0, "z_zero_goes_on", d)  # theta = pi / 2: lands near the top-left corner
    key(0, u + F32(0.5), v + F32(0.5), 0, flip(d, 2))
    for px, name in (((-5, 100), "out_left"), ((330, 100), "out_right"), ((100, -5), "out_top"), ((100, 250), "out_bottom")):
        matched(jl, px, 0, name)
    d = rnd()
    u, v = add(jl, _solve_u(g["cams"][0], 0.0, -1), 0, "u_eq_min_x_inside", d)
    assert u == 0.0
    key(0, 1.5, float(v) + 0.25, 0, flip(d, 3))
    u, v = add(jl, _solve_u(g["cams"][0], float(FC.HUT_W), 1), 0, "u_eq_max_x_outside")
    assert u == F32(FC.HUT_W)
    key(0, FC.HUT_W - 1.5, float(v) + 0.25, 0, rnd())
    matched(jl, (120, 40), 0, "below_min_distance", mn=1.5)
    matched(jl, (160, 40), 0, "above_max_distance", mn=0.1, mx=0.9)
    matched(jl, (200, 40), 0, "viewing_angle", away=True)
    add(jl, world_point(jl, (250, 200), 3.0), 0, "empty_window")
    matched(jl, (40, 80), 3, "level_below", octave=1)
    matched(jl, (80, 80), 2, "level_above", octave=3)          # the level_plus switch takes it
    matched(jl, (120, 80), 0, "chi2_reject", dx=2.0, dy=2.0)   # e2 = 8: above both literals
    matched(jl, (160, 80), 0, "chi2_band", dx=2.5, dy=0.8)     # e2 = 6.89: between 5.99 and 7.8
    # a tie across cells: level 1, radius 3.6; the keypoint of the left column comes LATER in the array
    d = rnd()
    u, v = add(jl, world_point(jl, (102.5, 120.0), 3.0), 1, "tie_across_cells", d)
    key(0, u + F32(2.4), v, 1, flip(d, 4, 8))
    key(0, u - F32(2.4), v, 1, flip(d, 4, 40))
    # a tie within a cell: the lower index wins
    d = rnd()
    u, v = add(jl, world_point(jl, (150.0, 120.0), 3.0), 1, "tie_within_cell", d)
    key(0, u + F32(0.6), v, 1, flip(d, 5, 16))
    key(0, u - F32(0.6), v, 1, flip(d, 5, 64))
    # three keypoints, the nearest descriptor last
    d = rnd()
    u, v = add(jl, world_point(jl, (200.0, 120.0), 3.0), 0, "least_distance", d)
    key(0, u + F32(1.0), v, 0, flip(d, 9))
    key(0, u - F32(1.0), v, 0, flip(d, 7))
    key(0, u, v + F32(1.0), 0, flip(d, 3))
    # sim3: no chi2 gate (the chi2 rows match there), and the far rule: both keypoints of the window at distance 256
    d = rnd()
    u, v = add(jl, world_point(jl, (60.0, 160.0), 3.0), 1, "sim3_far", d)
    key(0, u + F32(2.9), v, 1, flip(d, 256))
    key(0, u - F32(2.9), v, 1, flip(d, 256))
    # right only: the offset, a tie, the right camera's own model near the border
    matched(jr, (250, 150), 2, "offset_applied")
    matched(jr, (25, 210), 1, "right_far_from_centre")
    kl = np.zeros(len(kps[0]), g["kl"].dtype)
    kr = np.zeros(len(kps[1]), g["kl"].dtype)
    for arr, rows in ((kl, kps[0]), (kr, kps[1])):
        arr["x"], arr["y"], arr["octave"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        arr["size"], arr["angle"] = 31.0, 0.0
    dl, dr = (np.array([r[3] for r in kps[c]], np.uint8).reshape(-1, 32) for c in (0, 1))
    jl.update(kps=kl, desc=dl)
    jr.update(kps=kr, desc=dr, idx_offset=len(kl))
    sim.update(kps=kl, desc=dl)
    n = len(pts)
    names = [why[i] for i in range(n)]
    jl["valid"] = np.array([0 if nm == "matchR" else 1 for nm in names], np.uint8)  # the left job skips it: invalid_job
    c = dict(jobs=[jl, jr, sim], pts=np.array(pts, orbo.FUSE_POINT_DTYPE), desc=np.array(desc, np.uint8), th=TH, gf=False,
             refuse=None, why=why)
    _cache["hand"] = c
    return c


# ------------------------------------------------------------------------------------------------ the KeyFrame's window origin
def keyframe_origin():
    """-> the smallest case that tells the KeyFrame's integer window origin from the Frame's float one; NOT one of cases()
    (those share BOUNDS, whole numbers, where the two origins are one): it brings its own "bounds".  The cells come from the
    float bounds (0.9, 60.9, 0.9, 45.9) and are 0.94 px wide, the KeyFrame places its window from (0, 0): 0.96 cell to the left.
    One Scw job (no chi-square test), two points at level 0 (radius 3), each with ONE keypoint at Hamming distance 1:
      0  u = 40.6, keypoint 2.9 px left of it, cell column 39; the window starts at column floor(37.6 * 64 / 60) = 40 -- not found
         (from the float origin it would start at column 39 and find it);
      1  u = 20, keypoint 0.5 px right of it -- found either way"""
    if "origin" in _cache:
        return _cache["origin"]
    g = golden()
    rng = np.random.default_rng(75)
    job = dict(keyframe_jobs(np.hstack([np.eye(3), np.zeros((3, 1))]), None, None, None, None)[0], sim3=True)
    pts, desc, keys = [], [], []
    for px, dx in (((40.6, 20.0), -2.9), ((20.0, 20.0), 0.5)):
        d = rng.integers(0, 256, 32).astype(np.uint8)
        pos = world_point(job, px, 3.0)
        u, v = project(job, pos)
        pts.append(fuse_point(job, pos, 0))
        desc.append(d)
        keys.append((u + F32(dx), v + F32(0.25), flip(d, 1)))
    k = np.zeros(len(keys), g["kl"].dtype)
    k["x"], k["y"], k["size"] = [r[0] for r in keys], [r[1] for r in keys], 31.0
    job.update(kps=k, desc=np.array([r[2] for r in keys], np.uint8))
    c = dict(jobs=[job], pts=np.array(pts, orbo.FUSE_POINT_DTYPE), desc=np.array(desc, np.uint8), th=TH, gf=False, refuse=None,
             bounds=(0.9, 60.9, 0.9, 45.9))
    _cache["origin"] = c
    return c


# ------------------------------------------------------------------------------------------------ all cases
def _first(c, n, jobs):
    jobs = [dict(j, valid=None if j["valid"] is None else j["valid"][:n]) for j in jobs]
    return dict(c, jobs=jobs, pts=c["pts"][:n], desc=c["desc"][:n])


def cases():
    if "c" in _cache:
        return _cache["c"]
    g = golden()
    s = scene()
    out = {"scene": s, "hand": hand()}
    for n in (1, 15, 16, 17):
        out["np%d" % n] = _first(s, n, s["jobs"][:2])
    out["jobs1"] = _first(s, 200, s["jobs"][1:2])
    rng = np.random.default_rng(73)
    j16 = [dict(s["jobs"][k % 6], valid=(rng.random(120) > 0.2).astype(np.uint8)) for k in range(16)]
    out["jobs16"] = dict(_first(s, 120, []), jobs=j16)
    out["jobs17"] = dict(_first(s, 20, []), jobs=[dict(j, valid=None) for j in j16] + [dict(j16[0], valid=None)],
                         refuse="invalid")
    e_k, e_d = g["kl"][:0], g["dl"][:0]
    mid = dict(s["jobs"][1], kps=e_k, desc=e_d)
    out["empty_job"] = _first(s, 100, [s["jobs"][0], mid, s["jobs"][3]])
    out["no_points"] = _first(s, 0, s["jobs"][:2])
    reps = 4097 // len(g["kl"]) + 1
    k_big, d_big = np.tile(g["kl"], reps), np.tile(g["dl"], (reps, 1))
    big = dict(s["jobs"][0], valid=None)
    out["kf4096"] = _first(s, 24, [dict(big, kps=k_big[:4096], desc=d_big[:4096]), s["jobs"][1]])
    out["kf4097"] = dict(_first(s, 24, [s["jobs"][0], dict(big, kps=k_big[:4097], desc=d_big[:4097])]), refuse="unsupported")
    out["mono"] = _first(s, 300, [dict(s["jobs"][2], valid=None)])
    out["sim3"] = _first(s, 300, [dict(s["jobs"][0], sim3=True)])
    out["gemm_float"] = dict(_first(s, 300, s["jobs"][2:4]), gf=True)
    _cache["c"] = out
    return out


def reference(name, switches=()):
    """the numpy restatement on a case -> (best_idx, best_dist, census); cached without switches"""
    key = ("ref", name)
    if switches or key not in _cache:
        c, g = cases()[name], golden()
        census = {}
        bi, bd = FR.fuse_search_rig(c["jobs"], c["pts"], c["desc"], g["cams"], c["th"], LSF, g["sf"], g["is2"], BOUNDS,
                                    not c["gf"], switches, census)
        if switches:
            return bi, bd, census
        _cache[key] = (bi, bd, census)
    return _cache[key]
