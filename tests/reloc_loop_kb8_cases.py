"""Deterministic inputs of the relocalisation and loop-closing SearchByProjection tests for fisheye cameras:
tests/test_reloc_loop_kb8_cpu.py and tests/test_gpu_reloc_loop_kb8.py.

Keypoints and descriptors of the realistic cases are the committed golden's (tests/golden/pipeline_hut_320x240.npz), at most
300 of them per frame / KeyFrame; MapPoints are generated on the rays of keypoints and around them.  Frame bounds (0, 320, 0,
240), scale factor 1.2, 8 levels.

A (relocalisation) -- a_cases() -> name -> dict(cam (a kb8 tuple), T, Ow, th, orb_dist, kf_kps (mvKeys then mvKeysRight), nl
  (NLeft), flags, x3dw, mn, mx, desc, cur_kps, cur_desc, occupied, check_ori, gf)
  a_scene   260 KeyFrame entries (180 left, 80 right) against 300 current keypoints, CAM1
  a_hand    hand-made, with WIDE (fx * pi / 2 < cx: the image reaches beyond 90 degrees off axis): a point behind the camera that
            lands inside the bounds and takes a keypoint, one that lands outside, bounds, range, an empty window, an occupied
            slot, a contested keypoint, a tie, a right-camera MapPoint whose angle decides the histogram
  a_mono    a monocular KeyFrame (no right entries), no orientation check, gemm_float
  a_empty   no KeyFrame entries

B (loop closing) -- b_cases() -> name -> dict(jobs, pts (FUSE_POINT_DTYPE), desc, th (int), ratio, gf, refuse (None, or the
  index of the job the device entry refuses)); a job is what tests/reloc_loop_kb8_ref.py takes, plus camera = 0 for the helpers
  b_scene   ~300 points against 3 KeyFrames, matched bytes and validity bytes
  b_hand    every gate, u == minX inside and u == maxX outside, ties across and within cells, a contested keypoint whose loser
            moves on, nine points on nine keypoints (a sorted prefix of eight runs off its end), a viewing angle on which the
            double and the float dot product disagree
  b_one, b_six   1 job; 6 jobs
  b_empty_job, b_no_points
  b_long    ~6000 points of which 1000 to 4096 survive the first job's gates
  b_4096    exactly 4096 survivors in job 0 (served); b_4097: 4097 in job 1 (refused), job 0 delivered
reference_a(name) / reference_b(name): the numpy restatement on a case (cached) -> result and census."""
import numpy as np

import frustum_cases as FC
import fuse_rig_cases as FRC
import kb8_cases as KC
import kb8_ref as KR
import reloc_loop_kb8_ref as RL
from oracle import orbo

F32 = np.float32
BOUNDS = FRC.BOUNDS
IMG = FRC.IMG
CAM1 = KC.LOCAL_CAM
WIDE = (95.0, 95.5, 159.5, 120.25, KC.K_TUM, 0.0)  # 95 * pi / 2 = 149.2 < 159.5
LSF = FRC.LSF
_cache = {}
I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32)


def golden():
    return FRC.golden()


def _kps(rows):
    k = np.zeros(len(rows), orbo.KP_DTYPE)
    for f, col in (("x", 0), ("y", 1), ("octave", 2), ("angle", 3)):
        k[f] = [r[col] for r in rows]
    k["size"] = 31.0
    return k


def _ray_point(cam, T, px, z):
    """the world point that the camera at pose T sees at pixel px, the ray scaled by z"""
    ray, _, _ = KR.unproject(cam, np.array([px], F32))
    xc = ray[0].astype(np.float64) * z
    return ((xc - T[:, 3].astype(np.float64)) @ T[:, :3].astype(np.float64)).astype(F32)


def _project(cam, T, pos):
    from projection_bounds_ref import _gemm_row
    pc = np.array([[_gemm_row(T[r, :3], pos, T[r, 3], True) for r in range(3)]], F32)
    uv = KR.project(cam, pc)
    return F32(uv[0, 0]), F32(uv[0, 1])


# ------------------------------------------------------------------------------------------------ A
def _a_pack(cam, T, th, orb_dist, entries, nl, cur, occupied, check_ori=True, gf=False):
    """entries: (pos, level, desc, angle, flag, mn factor, mx factor or None)"""
    T, Ow = FC.pose(np.asarray(T)[:, :3], np.asarray(T)[:, 3])
    n = len(entries)
    kf = np.zeros(n, orbo.KP_DTYPE)
    kf["size"] = 31.0
    x3 = np.zeros((n, 3), F32)
    mn, mx = np.zeros(n, F32), np.zeros(n, F32)
    desc = np.zeros((n, 32), np.uint8)
    flags = np.zeros(n, np.uint8)
    for i, (pos, level, d, angle, flag, fmn, fmx) in enumerate(entries):
        x3[i] = pos
        dist = float(np.linalg.norm(np.asarray(pos, np.float64) - Ow.astype(np.float64)))
        mn[i] = F32(fmn * dist)
        mx[i] = FRC.max_for_level(dist, level) if fmx is None else F32(fmx * dist)
        desc[i], flags[i] = d, flag
        kf["angle"][i], kf["octave"][i] = angle, level
    cur_kps, cur_desc = cur
    return dict(cam=cam, T=T, Ow=Ow, th=th, orb_dist=orb_dist, kf_kps=kf, nl=nl, flags=flags, x3dw=x3, mn=mn, mx=mx, desc=desc,
                cur_kps=cur_kps, cur_desc=np.ascontiguousarray(cur_desc, np.uint8), occupied=occupied, check_ori=check_ori, gf=gf)


def a_scene(n_left=180, n_right=80, check_ori=True, gf=False, seed=81):
    g = golden()
    rng = np.random.default_rng(seed)
    cam = KR.camera(*CAM1)
    T = np.asarray(FC.pose(FC.rotation(0.01, -0.02, 0.015), (0.05, -0.02, 0.03))[0], F32)
    cur_kps, cur_desc = g["kl"][:300].copy(), g["dl"][:300].copy()
    order = rng.permutation(300)
    entries = []
    for k in range(n_left + n_right):
        if k % 9 == 4:  # junk: anywhere around the camera, behind it included
            pos = (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-2, 6))
            entries.append((pos, int(rng.integers(0, 4)), rng.integers(0, 256, 32).astype(np.uint8), 0.0, 1, 0.5, 3.0))
            continue
        i2 = int(order[k % 300])
        pos = _ray_point(cam, T, (cur_kps["x"][i2], cur_kps["y"][i2]), rng.uniform(2.0, 6.0))
        d = cur_desc[i2].copy()
        d[k % 32] ^= np.uint8(1 << (k % 8))
        turn = 0.0 if k % 7 else 90.0  # one match in seven lands in another bin of the rotation histogram
        angle = F32((float(cur_kps["angle"][i2]) + turn + rng.uniform(-4, 4)) % 360.0)
        entries.append((pos, int(cur_kps["octave"][i2]), d, angle, 0 if k % 11 == 3 else 1, 0.6, None))
    occupied = (rng.random(300) < 0.08).astype(np.uint8)
    return _a_pack(CAM1, T, 3.0, 100, entries, n_left, (cur_kps, cur_desc), occupied, check_ori, gf)


def a_hand():
    """-> the case; c["why"]: entry index -> what it is there for"""
    rng = np.random.default_rng(82)
    cam = KR.camera(*WIDE)
    T = I34
    cur, entries, why = [], [], {}   # cur: (x, y, octave, angle, desc, occupied)

    def rnd():
        return rng.integers(0, 256, 32).astype(np.uint8)

    def key(x, y, octave, d, occ=0):
        cur.append((F32(x), F32(y), octave, 0.0, d, occ))
        return len(cur) - 1

    def entry(pos, level, name, d, angle=0.0, flag=1, mn=0.6, mx=None):
        entries.append((np.asarray(pos, F32), level, d, angle, flag, mn, mx))
        why[len(entries) - 1] = name
        return _project(cam, T, np.asarray(pos, F32))

    def matched(px, level, name, angle=0.0, bits=1, z=3.0, occ=0, **kw):
        d = rnd()
        u, v = entry(_ray_point(cam, T, px, z), level, name, d, angle, **kw)
        key(u + F32(0.5), v + F32(0.5), level, FRC.flip(d, bits), occ)

    nl = 24
    # left entries 0 .. nl - 1.  Entry 0 turns by 270 degrees: alone in bin 9, rejected; its angle is what the reference's
    # out-of-range read would NOT find for the right entry nl + 0
    matched((40, 30), 0, "alone_in_bin_9", angle=270.0)
    for k, px in enumerate(((80, 30), (120, 30), (160, 30), (200, 30))):
        matched(px, 0, "bin0_%d" % k)
    for k, px in enumerate(((40, 70), (80, 70), (120, 70))):
        matched(px, 0, "bin3_%d" % k, angle=90.0)
    for k, px in enumerate(((160, 70), (200, 70), (240, 70))):
        matched(px, 1, "bin6_%d" % k, angle=180.0)
    d = rnd()
    u, v = entry((3.0, 0.3, -0.15), 0, "behind_inside", d)  # theta = 1.62 > pi / 2: lands near the right border
    assert 0 <= u <= 320 and 0 <= v <= 240, (u, v)
    key(u - F32(0.5), v + F32(0.5), 0, FRC.flip(d, 2))
    entry((0.3, 0.2, -1.0), 0, "behind_outside", rnd())
    u, v = entry((0.0, -3.0, 0.5), 0, "out_of_bounds", rnd())  # in front of the camera, 80 degrees up: above the image
    assert v < 0
    key(u, 1.0, 0, rnd())
    matched((40, 110), 0, "below_min", mn=1.5)
    matched((80, 110), 0, "above_max", mn=0.1, mx=0.9)
    entry(_ray_point(cam, T, (280, 200), 3.0), 0, "empty_window", rnd())
    matched((120, 110), 0, "occupied_on_entry", occ=1)
    matched((160, 110), 0, "not_flagged", flag=0)
    matched((200, 110), 0, "above_orb_dist", bits=70)
    # a contested keypoint: both entries are nearest to keypoint A; the first takes it, the second moves on to B
    d = rnd()
    pos = _ray_point(cam, T, (40, 150), 3.0)
    u, v = entry(pos, 0, "contest_winner", d)
    entry(_ray_point(cam, T, (40, 150), 3.5), 0, "contest_loser", FRC.flip(d, 1, 200))
    key(u + F32(0.5), v, 0, FRC.flip(d, 1))          # A
    key(u - F32(0.5), v, 0, FRC.flip(d, 6, 100))     # B
    # a tie: two keypoints at the same distance, the first of the window order wins (the left column's, later in the array)
    d = rnd()
    u, v = entry(_ray_point(cam, T, (102.5, 150.0), 3.0), 1, "tie", d)
    key(u + F32(2.4), v, 1, FRC.flip(d, 4, 8))
    key(u - F32(2.4), v, 1, FRC.flip(d, 4, 40))
    while len(entries) < nl:
        entry((0.0, 0.0, 2.0), 0, "pad", rnd(), flag=0)
    assert len(entries) == nl
    # right entries nl ..: entry nl + 0 turns by 0 degrees (bin 0, kept); the left array's entry 0 says 270 (bin 9, rejected)
    matched((240, 110), 0, "right_decides", angle=0.0)
    matched((240, 150), 0, "right_bin3", angle=90.0)
    cur_kps = _kps([(r[0], r[1], r[2], r[3]) for r in cur])
    cur_desc = np.array([r[4] for r in cur], np.uint8)
    occupied = np.array([r[5] for r in cur], np.uint8)
    c = _a_pack(WIDE, T, 3.0, 64, entries, nl, (cur_kps, cur_desc), occupied)
    c["why"] = why
    return c


def a_cases():
    if "a" not in _cache:
        empty = a_scene()
        for k in ("kf_kps", "flags", "x3dw", "mn", "mx", "desc"):
            empty[k] = empty[k][:0]
        empty["nl"] = 0
        mono = a_scene(200, 0, check_ori=False, gf=True, seed=83)
        _cache["a"] = {"a_scene": a_scene(), "a_hand": a_hand(), "a_mono": mono, "a_empty": empty}
    return _cache["a"]


def reference_a(name, switches=()):
    key = ("ra", name)
    if switches or key not in _cache:
        c = a_cases()[name]
        census = {}
        nm, m = RL.search_by_projection_keyframe_kb8(c["T"], c["Ow"], KR.camera(*c["cam"]), c["th"], c["orb_dist"], LSF, c["kf_kps"],
                                                     c["flags"], c["x3dw"], c["mn"], c["mx"], c["desc"], c["cur_kps"],
                                                     c["cur_desc"], golden()["sf"], BOUNDS, c["check_ori"], c["occupied"],
                                                     not c["gf"], c["nl"], switches, census)
        if switches:
            return nm, m, census
        _cache[key] = (nm, m, census)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ B
def _job(T, kps, desc, matched=None, valid=None):
    pose = FRC._pose(T)
    return dict(pose=pose, camera=0, kps=kps, desc=desc, matched=matched, valid=valid)


def b_scene():
    if "b_scene" in _cache:
        return _cache["b_scene"]
    g = golden()
    rng = np.random.default_rng(84)
    sets = ((g["kl"][:300], g["dl"][:300]), (g["kr"][:280], g["dr"][:280]), (g["kl"][150:450], g["dl"][150:450]))
    jobs = [_job(T, k, d) for T, (k, d) in zip(FRC.scene_poses(), sets)]
    pts, desc = [], []
    for job in jobs:
        for i in range(0, len(job["kps"]), 4):
            kp = job["kps"][i]
            pos = FRC.world_point(job, (kp["x"], kp["y"]), rng.uniform(2.0, 6.0))
            pts.append(FRC.fuse_point(job, pos, min(int(kp["octave"]) + (i // 4) % 2, 7)))  # levels [l - 1, l]: both ends
            d = job["desc"][i].copy()
            d[i % 32] ^= np.uint8(1 << (i % 8))
            desc.append(d)
    T0, Ow0 = FC.pose(np.eye(3), np.zeros(3))
    for q in FC.random_points(rng, 70, T0, Ow0, spread=2.6, zr=(-1.5, 9.0)):
        p = np.zeros((), orbo.FUSE_POINT_DTYPE)
        p["pos"], p["normal"], p["min_distance"], p["max_distance"], p["valid"] = q["pos"], q["normal"], q["min_dist"], \
            q["max_dist"], 1
        pts.append(p)
        desc.append(rng.integers(0, 256, 32).astype(np.uint8))
    order = rng.permutation(len(pts))
    pts = np.array(pts, orbo.FUSE_POINT_DTYPE)[order]
    desc = np.array(desc, np.uint8)[order]
    pts["valid"] = np.where(np.arange(len(pts)) % 13 == 5, 0, pts["valid"])
    jobs[0]["valid"] = (rng.random(len(pts)) > 0.1).astype(np.uint8)
    jobs[1]["matched"] = (rng.random(len(jobs[1]["kps"])) < 0.15).astype(np.uint8)
    jobs[2]["valid"] = (rng.random(len(pts)) > 0.2).astype(np.uint8)
    jobs[2]["matched"] = (rng.random(len(jobs[2]["kps"])) < 0.1).astype(np.uint8)
    _cache["b_scene"] = dict(jobs=jobs, pts=pts, desc=desc, th=3, ratio=1.0, gf=False, refuse=None)
    return _cache["b_scene"]


def _dot_disagreement(rng, Ow):
    """a world point and a normal at 60 degrees to its viewing ray on which PO.dot(Pn) < 0.5 * dist holds in float and not in
    double: the double rule lets the point through"""
    from projection_bounds_ref import _dot, _norm
    for _ in range(200000):
        pos = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), rng.uniform(2.5, 4.0)], F32)
        PO = (pos - Ow).astype(F32)
        d3 = _norm(PO)
        a = np.cross(PO.astype(np.float64), rng.normal(size=3))
        a /= np.linalg.norm(a)
        ray = PO.astype(np.float64) / float(d3)
        nrm = (0.5 * ray + np.sqrt(0.75) * a).astype(F32)
        s = F32(0)
        for k in range(3):
            s = F32(s + F32(PO[k] * nrm[k]))
        if bool(s < F32(F32(0.5) * d3)) and not (_dot(PO, nrm) < 0.5 * float(d3)):
            return pos, nrm
    raise AssertionError("no disagreement found")


def b_hand():
    if "b_hand" in _cache:
        return _cache["b_hand"]
    g = golden()
    rng = np.random.default_rng(85)
    jl = _job(I34, None, None)
    cam = g["cams"][0]
    kps, pts, desc, why = [], [], [], {}   # kps: (x, y, octave, angle, desc, matched)

    def rnd():
        return rng.integers(0, 256, 32).astype(np.uint8)

    def add(pos, level, name, d=None, **kw):
        pts.append(FRC.fuse_point(jl, pos, level, **kw))
        desc.append(rnd() if d is None else d)
        why[len(pts) - 1] = name
        return FRC.project(jl, pos)

    def key(x, y, octave, d, m=0):
        kps.append((F32(x), F32(y), octave, 0.0, d, m))

    def matched(px, level, name, dx=0.5, dy=0.5, bits=1, octave=None, z=3.0, m=0, **kw):
        d = rnd()
        u, v = add(FRC.world_point(jl, px, z), level, name, d, **kw)
        key(u + F32(dx), v + F32(dy), level if octave is None else octave, FRC.flip(d, bits), m)

    matched((40, 40), 0, "match")
    matched((80, 40), 0, "invalid_point", valid=0)
    matched((120, 40), 0, "invalid_job")
    matched((160, 40), 1, "above_threshold", bits=60)
    add((0.3, 0.2, -1.0), 0, "z_negative")
    d = rnd()
    u, v = add((-0.8, -0.6, 0.0), 0, "z_zero_goes_on", d)  # theta = pi / 2: lands near the top-left corner
    key(u + F32(0.5), v + F32(0.5), 0, FRC.flip(d, 2))
    for px, name in (((-5, 100), "out_left"), ((330, 100), "out_right"), ((100, -5), "out_top"), ((100, 250), "out_bottom")):
        matched(px, 0, name)
    d = rnd()
    u, v = add(FRC._solve_u(cam, 0.0, -1), 0, "u_eq_min_x_inside", d)
    assert u == 0.0
    key(1.5, float(v) + 0.25, 0, FRC.flip(d, 3))
    d = rnd()
    u, v = add(FRC._solve_u(cam, float(FC.HUT_W), 1), 1, "u_eq_max_x_outside", d)
    assert u == F32(FC.HUT_W)
    key(FC.HUT_W - 2.6, float(v) + 0.25, 1, FRC.flip(d, 3))  # in the grid's last column; the closed_upper switch takes it
    matched((200, 40), 0, "below_min_distance", mn=1.5)
    matched((240, 40), 0, "above_max_distance", mn=0.1, mx=0.9)
    matched((280, 40), 0, "viewing_angle", away=True)
    add(FRC.world_point(jl, (250, 200), 3.0), 0, "empty_window")
    matched((40, 80), 3, "level_below", octave=1)
    matched((80, 80), 2, "level_above", octave=3)          # the level_plus switch takes it
    matched((120, 80), 0, "matched_on_entry", m=1)
    # a tie across cells: level 1, radius 3.6; the keypoint of the left column comes LATER in the array
    d = rnd()
    u, v = add(FRC.world_point(jl, (102.5, 120.0), 3.0), 1, "tie_across_cells", d)
    key(u + F32(2.4), v, 1, FRC.flip(d, 4, 8))
    key(u - F32(2.4), v, 1, FRC.flip(d, 4, 40))
    d = rnd()
    u, v = add(FRC.world_point(jl, (150.0, 120.0), 3.0), 1, "tie_within_cell", d)
    key(u + F32(0.6), v, 1, FRC.flip(d, 5, 16))
    key(u - F32(0.6), v, 1, FRC.flip(d, 5, 64))
    # a contested keypoint: both points are nearest to A; the lower iMP takes it and the loser moves on to B
    d = rnd()
    u, v = add(FRC.world_point(jl, (200.0, 120.0), 3.0), 0, "contest_winner", d)
    add(FRC.world_point(jl, (200.0, 120.0), 3.4), 0, "contest_loser", FRC.flip(d, 1, 200))
    key(u + F32(0.5), v, 0, FRC.flip(d, 1))        # A
    key(u - F32(0.5), v, 0, FRC.flip(d, 6, 100))   # B
    # nine points with ONE descriptor on nine keypoints at distances 1 .. 9: point k finds its k nearest taken; the ninth runs
    # off a sorted prefix of eight
    d = rnd()
    for k in range(9):
        u, v = add(FRC.world_point(jl, (60.0, 180.0), 3.0 + 0.05 * k), 0, "prefix_%d" % k, d)
    for k in range(9):
        key(u + F32(0.5 * (k % 3) - 0.5), v + F32(0.5 * (k // 3) - 0.5), 0, FRC.flip(d, k + 1, 8 * k))
    # the viewing angle on which the double and the float dot product disagree
    pos, nrm = _dot_disagreement(rng, jl["pose"][2])
    d = rnd()
    u, v = add(pos, 0, "dot_double_lets_through", d)
    pts[-1]["normal"] = nrm
    key(u + F32(0.5), v + F32(0.5), 0, FRC.flip(d, 2))
    k = _kps([(r[0], r[1], r[2], r[3]) for r in kps])
    jl.update(kps=k, desc=np.array([r[4] for r in kps], np.uint8), matched=np.array([r[5] for r in kps], np.uint8))
    names = [why[i] for i in range(len(pts))]
    jl["valid"] = np.array([0 if nm == "invalid_job" else 1 for nm in names], np.uint8)
    c = dict(jobs=[jl], pts=np.array(pts, orbo.FUSE_POINT_DTYPE), desc=np.array(desc, np.uint8), th=3, ratio=1.0, gf=False,
             refuse=None, why=why)
    _cache["b_hand"] = c
    return c


def _sure_points(rng, n, job, kps, kdesc, n_match):
    """n points that pass every gate of every pose near the job's: pixels 25 px inside the image, facing the camera, levels 1
    .. 3 (the range reaches 1.095 of the distance and more); the first n_match on keypoint rays with a descriptor one bit off"""
    cam = golden()["cams"][0]
    px = np.stack([rng.uniform(25, 295, n), rng.uniform(25, 215, n)], 1).astype(F32)
    inside = np.nonzero((kps["x"] > 25) & (kps["x"] < 295) & (kps["y"] > 25) & (kps["y"] < 215))[0]
    pick = inside[:n_match]
    px[:len(pick), 0], px[:len(pick), 1] = kps["x"][pick], kps["y"][pick]
    rays, _, _ = KR.unproject(cam, px)
    R, t, Ow = job["pose"]
    xc = rays.astype(np.float64) * rng.uniform(2.0, 6.0, n)[:, None]
    pw = ((xc - t.astype(np.float64)) @ R.astype(np.float64)).astype(F32)
    pts = np.zeros(n, orbo.FUSE_POINT_DTYPE)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    for i in range(n):
        level = int(kps["octave"][pick[i]]) + 1 if i < len(pick) else 1 + i % 3
        pts[i] = FRC.fuse_point(job, pw[i], min(max(level, 1), 7), mn=0.5)
        if i < len(pick):
            desc[i] = kdesc[pick[i]]
            desc[i, i % 32] ^= np.uint8(1 << (i % 8))
    return pts, desc


def _long(n_sure, n_junk, seed, off_second):
    """n_sure sure survivors and n_junk points that no job lets through, interleaved; job 0 takes every point, job 1 (a pose
    2 cm away) has off_second of the sure ones switched off"""
    g = golden()
    rng = np.random.default_rng(seed)
    k, d = g["kl"][:300], g["dl"][:300]
    j0 = _job(I34, k, d)
    T1 = np.asarray(FC.pose(FC.rotation(0.002, -0.003, 0.001), (0.02, -0.01, 0.01))[0], F32)
    j1 = _job(T1, g["kr"][:300], g["dr"][:300])
    pts, desc = _sure_points(rng, n_sure, j0, k, d, 200)
    junk = np.zeros(n_junk, orbo.FUSE_POINT_DTYPE)
    junk["pos"] = np.stack([rng.uniform(-2, 2, n_junk), rng.uniform(-2, 2, n_junk), rng.uniform(-6.0, -0.5, n_junk)], 1)  # behind
    junk["normal"], junk["min_distance"], junk["max_distance"], junk["valid"] = (0, 0, 1), 0.1, 50.0, 1
    junk["valid"][::5] = 0
    allp = np.concatenate([pts, junk])
    alld = np.concatenate([desc, rng.integers(0, 256, (n_junk, 32)).astype(np.uint8)])
    order = rng.permutation(len(allp))
    allp, alld = allp[order], alld[order]
    sure = np.nonzero(order < n_sure)[0]
    v = np.ones(len(allp), np.uint8)
    v[sure[rng.permutation(len(sure))[:off_second]]] = 0
    j1["valid"] = v
    return dict(jobs=[j0, j1], pts=allp, desc=alld, th=3, ratio=1.0, gf=False, refuse=None)


def b_cases():
    if "b" in _cache:
        return _cache["b"]
    g = golden()
    s = b_scene()
    rng = np.random.default_rng(86)
    out = {"b_scene": s, "b_hand": b_hand()}
    out["b_one"] = dict(s, jobs=s["jobs"][1:2], ratio=0.8)
    n = 150
    six = []
    for k in range(6):
        j = s["jobs"][k % 3]
        six.append(dict(j, valid=(rng.random(n) > 0.15).astype(np.uint8),
                        matched=(rng.random(len(j["kps"])) < 0.05 * k).astype(np.uint8)))
    out["b_six"] = dict(s, jobs=six, pts=s["pts"][:n], desc=s["desc"][:n], th=4, gf=True)
    empty = dict(s["jobs"][1], kps=g["kl"][:0], desc=g["dl"][:0], matched=None)
    out["b_empty_job"] = dict(s, jobs=[s["jobs"][0], empty, dict(s["jobs"][2], valid=None)])
    out["b_no_points"] = dict(s, jobs=[dict(j, valid=None) for j in s["jobs"][:2]], pts=s["pts"][:0], desc=s["desc"][:0])
    out["b_long"] = _long(2400, 3600, 87, 900)
    out["b_4096"] = _long(4096, 404, 88, 3000)
    c = _long(4097, 403, 89, 3000)
    out["b_4097"] = dict(c, jobs=c["jobs"][::-1], refuse=1)
    _cache["b"] = out
    return out


def reference_b(name, switches=()):
    """-> (match_kf per job, nmatches, n_gated, census); cached without switches"""
    key = ("rb", name)
    if switches or key not in _cache:
        c = b_cases()[name]
        census = {}
        m, nm, ng = RL.search_by_projection_sim3_kb8(c["jobs"], c["pts"], c["desc"], golden()["cams"][0], c["th"], c["ratio"], LSF,
                                                     golden()["sf"], BOUNDS, not c["gf"], switches, census)
        if switches:
            return m, nm, ng, census
        _cache[key] = (m, nm, ng, census)
    return _cache[key]
