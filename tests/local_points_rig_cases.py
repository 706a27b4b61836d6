"""Deterministic inputs of the rig (two-fisheye, Nleft != -1) SearchLocalPoints tests: tests/test_local_points_rig_cpu.py,
tests/test_gpu_local_points_rig.py, tests/test_cpp_local_points_rig.py, tests/tools/time_local_points_rig.py.

Keypoints and descriptors are the committed golden's (tests/golden/pipeline_hut_320x240.npz): kL / dL as the left frame, kR / dR
as the right one, mvLeftToRightMatch = its SearchForInitialization matches, mvRightToLeftMatch their inverse.  The left camera
is kb8_cases.LOCAL_CAM, the rig kb8_cases.rig().

scene()     the realistic one (under 1500 MapPoints): points on the left rays of the left keypoints and on the right rays of the
            right keypoints, "ambiguous" points (on a left ray, descriptor halfway between two left keypoints of one level in one
            window: the left ratio test fails), and random junk, interleaved; blocking (flags 3) and non-blocking (flags 1)
            alternate.  Far points on (thFarPoints 8).
cases()     name -> dict(tl, tr, desc, kl, dl, kr, dr, l2r, r2l, occ, th, nnratio, takes): caller-made records for the matcher
            alone; `takes` names the census entries of tests/local_points_rig_ref.py the case is there for.
"""
import os

import numpy as np

import frustum_cases as FC
import frustum_ref as FR
import kb8_cases as KC
import kb8_ref as KR
import local_points_rig_ref as RR
from oracle import orbo
from undistort_ref import hamming

F32 = np.float32
BOUNDS = (0.0, float(FC.HUT_W), 0.0, float(FC.HUT_H))
_cache = {}


def golden():
    """-> dict(kl, dl, kr, dr, l2r, r2l, ur, sf)"""
    if "g" in _cache:
        return _cache["g"]
    p = np.load(os.path.join(FC.GOLDEN, "pipeline_hut_320x240.npz"))
    kl, dl, kr, dr = p["kL"], p["dL"], p["kR"], p["dR"]
    l2r = p["init_matches"].astype(np.int32)
    assert len(l2r) == len(kl) and l2r.max() < len(kr) and l2r.min() >= -1
    r2l = np.full(len(kr), -1, np.int32)
    r2l[l2r[l2r >= 0]] = np.nonzero(l2r >= 0)[0]
    assert (r2l >= 0).sum() == (l2r >= 0).sum()  # SearchForInitialization matches are one to one
    sf = np.asarray(orbo.Extractor(FC.HUT_NF).tables()["scale"], F32)
    _cache["g"] = dict(kl=kl, dl=dl, kr=kr, dr=dr, l2r=l2r, r2l=r2l, ur=p["uRight"].astype(F32), sf=sf)
    return _cache["g"]


def _on_rays(cam, Rcw, t, twc, kps, z, sf):
    """MapPoints at depth z on the rays of `kps` of the camera x_c = Rcw * x_w + t whose centre isInFrustumChecks reads as twc"""
    rays, _, _ = KR.unproject(cam, np.stack([kps["x"], kps["y"]], 1))
    pc = rays.astype(np.float64) * z[:, None]
    pw = (pc - np.asarray(t, np.float64)) @ np.asarray(Rcw, np.float64)
    mp = np.zeros(len(kps), FR.MAP_POINT_DTYPE)
    mp["pos"] = pw.astype(F32)
    ray = pw - np.asarray(twc, np.float64)
    d = np.linalg.norm(ray, axis=1)
    mp["normal"] = (ray / d[:, None]).astype(F32)
    mp["min_dist"] = (0.6 * d).astype(F32)
    mp["max_dist"] = (F32(1.05) * d.astype(F32) * sf[kps["octave"]]).astype(F32)  # PredictScale -> octave + 1 (or the top level)
    return mp


def ambiguous_pairs(kps, desc, radius=9.0, limit=60):
    """(i, k, descriptor): keypoints of one octave within `radius` pixels and a descriptor halfway between theirs, so that
    best and second best lie on one level at nearly equal distance"""
    out, used = [], set()
    H = hamming(desc, desc)
    for i in range(len(kps)):
        if i in used:
            continue
        near = np.nonzero((np.abs(kps["x"] - kps["x"][i]) < radius) & (np.abs(kps["y"] - kps["y"][i]) < radius) &
                          (kps["octave"] == kps["octave"][i]))[0]
        near = [k for k in near if k != i and k not in used and H[i, k] <= 160]
        if not near:
            continue
        k = min(near, key=lambda c: H[i, c])
        bits_i, bits_k = np.unpackbits(desc[i]), np.unpackbits(desc[k])
        diff = np.nonzero(bits_i != bits_k)[0]
        b = bits_i.copy()
        b[diff[::2]] = bits_k[diff[::2]]
        out.append((i, int(k), np.packbits(b)))
        used.update((i, int(k)))
        if len(out) == limit:
            break
    return out


def scene():
    """-> dict(P, cam, cam_tuple, rig, pts, desc, n_kinds) and the golden's arrays"""
    if "s" in _cache:
        return _cache["s"]
    g = golden()
    kl, dl, kr, dr, sf = g["kl"], g["dl"], g["kr"], g["dr"], g["sf"]
    cam = KR.camera(*KC.LOCAL_CAM)
    rig = KC.rig()
    rng = np.random.default_rng(51)
    T, Ow = FC.pose(FC.rotation(-0.12, 0.2, 0.05), (0.2, -0.1, 0.3))
    fx, fy, cx, cy = KC.LOCAL_CAM[:4]
    P = FR.params(T, Ow, (fx, fy, cx, cy, KC.MBF), FC.LSF, (FC.HUT_W, FC.HUT_H), 0.5, far_points=True, th_far_points=8.0)
    left = _on_rays(cam, T[:, :3], T[:, 3], Ow, kl, rng.uniform(2.0, 6.0, len(kl)), sf)
    ldesc = dl.copy()
    ldesc[np.arange(len(kl)), np.arange(len(kl)) % 32] ^= np.uint8(1)
    M, twc_r = KR.rig_right_pose(P, rig)
    right = _on_rays(rig["cam2"], M[:, :3], M[:, 3], twc_r, kr, rng.uniform(2.0, 6.0, len(kr)), sf)
    rdesc = dr.copy()
    rdesc[np.arange(len(kr)), np.arange(len(kr)) % 32] ^= np.uint8(2)
    amb = ambiguous_pairs(kl, dl)
    ai = np.array([a[0] for a in amb])
    ambp = _on_rays(cam, T[:, :3], T[:, 3], Ow, kl[ai], rng.uniform(2.0, 5.0, len(ai)), sf)
    adesc = np.stack([a[2] for a in amb])
    # the golden has 15 stereo matches: four (left) and eight (right) more MapPoints on the rays of each matched keypoint of either side (a map holds
    # such duplicates until Fuse merges them), so that cross-writes come in numbers
    ml, mr = np.repeat(np.nonzero(g["l2r"] >= 0)[0], 4), np.repeat(np.nonzero(g["r2l"] >= 0)[0], 8)
    dupl = _on_rays(cam, T[:, :3], T[:, 3], Ow, kl[ml], rng.uniform(2.0, 5.0, len(ml)), sf)
    dupr = _on_rays(rig["cam2"], M[:, :3], M[:, 3], twc_r, kr[mr], rng.uniform(2.0, 5.0, len(mr)), sf)
    dupdesc = np.concatenate([dl[ml], dr[mr]])
    dupdesc[np.arange(len(dupdesc)), np.arange(len(dupdesc)) % 32] ^= np.uint8(4)
    m = 270
    junk = FC.random_points(rng, m, T, Ow, spread=2.6, zr=(-1.5, 9.0))
    jdesc = rng.integers(0, 256, (m, 32)).astype(np.uint8)
    pts = np.concatenate([left, right, ambp, dupl, dupr, junk])
    desc = np.concatenate([ldesc, rdesc, adesc, dupdesc, jdesc])
    dup = np.zeros(len(pts), bool)
    dup[len(left) + len(right) + len(ambp):len(pts) - m] = True
    order = rng.permutation(len(pts))
    pts, desc, dup = pts[order], desc[order], dup[order]
    pts["flags"] = np.where(np.arange(len(pts)) % 3 == 0, 3, 1)  # blocking and non-blocking alternate, one in three blocks
    pts["flags"][dup] = 1                                        # the duplicates are fresh points without observations
    assert len(pts) < 1500
    _cache["s"] = dict(g, P=P, cam=cam, cam_tuple=KC.LOCAL_CAM, rig=rig, pts=pts, desc=desc,
                       n_kinds=(len(left), len(right), len(ambp), len(dupl), len(dupr), m))
    return _cache["s"]


def scene_records(far=True):
    """-> (left records, right records, left depths, right depths, points either camera sees) of kb8_ref.frame_in_frustum_rig,
    and the same records after the far rule; cached"""
    key = ("rec", far)
    if key not in _cache:
        s = scene()
        P = dict(s["P"])
        P["far_points"] = 1 if far else 0
        if "raw" not in _cache:
            _cache["raw"] = KR.frame_in_frustum_rig(s["P"], s["cam"], s["rig"], s["pts"], FR.bounds_of(s["P"]), FC.NLEVELS)
        tl, tr, dl, dr, nv = _cache["raw"]
        _cache[key] = (P, _cache["raw"], RR.far_filtered_rig(P, tl, tr, dl))
    return _cache[key]


def _rec(kps, i, flags, view_cos=1.0, level_up=None, dx=0.0, dy=0.0):
    """a record that looks at keypoint i: levels [level - 1, level] hold its octave"""
    o = int(kps["octave"][i])
    up = (i % 2) if level_up is None else level_up
    t = np.zeros((), orbo.MP_TRACK_DTYPE)
    t["proj_x"], t["proj_y"] = F32(kps["x"][i] + F32(dx)), F32(kps["y"][i] + F32(dy))
    t["view_cos"], t["level"], t["flags"] = view_cos, min(o + up, FC.NLEVELS - 1), flags
    return t


def _none(blocking):
    t = np.zeros((), orbo.MP_TRACK_DTYPE)
    t["level"], t["flags"] = -1, 2 if blocking else 0
    return t


def _case(g, rows, **kw):
    """rows: (left record, right record, descriptor)"""
    c = dict(kl=g["kl"], dl=g["dl"], kr=g["kr"], dr=g["dr"], l2r=g["l2r"], r2l=g["r2l"], occ=None, th=1.0, nnratio=0.8, takes=())
    c["tl"] = np.array([r[0] for r in rows], orbo.MP_TRACK_DTYPE).reshape(-1)
    c["tr"] = np.array([r[1] for r in rows], orbo.MP_TRACK_DTYPE).reshape(-1)
    c["desc"] = np.array([r[2] for r in rows], np.uint8).reshape(-1, 32)
    c.update(kw)
    return c


def _dense_window(kps, desc, need, level, radius):
    """-> (centre keypoint, its `need` nearest descriptors' keypoints among octaves level - 1 and level inside the window, nearest
    first)"""
    best = None
    H = hamming(desc, desc)
    on = (kps["octave"] >= level - 1) & (kps["octave"] <= level)
    for i in np.nonzero(on)[0]:
        near = np.nonzero((np.abs(kps["x"] - kps["x"][i]) < radius) & (np.abs(kps["y"] - kps["y"][i]) < radius) & on)[0]
        if len(near) < need + 1:
            continue
        ordered = sorted(near, key=lambda c: (H[i, c], c))
        score = H[i, ordered[need]]  # distance of the first candidate the occupiers leave free
        if best is None or score < best[0]:
            best = (score, int(i), [int(c) for c in ordered[:need]])
    assert best is not None
    return best[1], best[2]


def cases():
    if "c" in _cache:
        return _cache["c"]
    g = golden()
    kl, dl, kr, dr, l2r, r2l = g["kl"], g["dl"], g["kr"], g["dr"], g["l2r"], g["r2l"]
    nl, nr = len(kl), len(kr)
    out = {}
    # the realistic scene at th 1 and 3, and with the maps cut (decoupled)
    _, _, (tl, tr) = scene_records(True)
    s = scene()
    base = dict(kl=kl, dl=dl, kr=kr, dr=dr, l2r=l2r, r2l=r2l, occ=None, nnratio=0.8, tl=tl, tr=tr, desc=s["desc"])
    out["scene_th1"] = dict(base, th=1.0, takes=("left_cross", "left_direct", "right_cross", "right_direct"))
    out["scene_th3"] = dict(base, th=3.0, takes=("left_cross", "right_cross", "left_ratio_skips_right", "right_empty_window"))
    occ = (np.random.default_rng(52).random(nl + nr) < 0.15).astype(np.uint8)
    out["scene_occupied"] = dict(base, th=3.0, occ=occ, takes=("cross_on_occupied", "cross_frees"))
    out["decoupled"] = dict(base, th=3.0, l2r=np.full(nl, -1, np.int32), r2l=np.full(nr, -1, np.int32),
                            takes=("left_direct", "right_direct"))
    e_k, e_d = kl[:0], dl[:0]
    out["no_right"] = dict(base, th=3.0, kr=e_k, dr=e_d, l2r=np.full(nl, -1, np.int32), r2l=np.zeros(0, np.int32),
                           takes=("left_direct", "right_empty_window"))
    out["no_left"] = dict(base, th=3.0, kl=e_k, dl=e_d, l2r=np.zeros(0, np.int32), r2l=np.full(nr, -1, np.int32),
                          takes=("right_direct",))
    # a freed-slot chain: right slot j occupied from the start; A (no observations) matches left keypoint i and cross-writes j,
    # which frees it; B, later, takes j through its right branch
    pairs = [(int(i), int(l2r[i])) for i in np.nonzero(l2r >= 0)[0][:24]]
    rows, occ = [], np.zeros(nl + nr, np.uint8)
    for i, j in pairs:
        occ[nl + j] = 1
        rows.append((_rec(kl, i, 1), _none(False), dl[i]))
    for i, j in pairs:
        rows.append((_none(True), _rec(kr, j, 3), dr[j]))
    out["freed_chain"] = _case(g, rows, occ=occ, takes=("cross_on_occupied", "cross_frees", "freed_taken"))
    # a blocking point that both cameras see at a matched pair (i, j): its left cross-write takes j away from its own right branch
    rows = [(_rec(kl, i, 3), _rec(kr, j, 3), dl[i]) for i, j in pairs]
    out["own_cross"] = _case(g, rows, takes=("left_cross", "own_cross_blocks_right"))
    # a ratio failure on the left (ambiguous descriptor) in front of a right branch that would match
    rows = []
    for i, k, d in ambiguous_pairs(kl, dl, limit=24):
        j = int(np.argmin(hamming(d[None], dr)[0]))  # the right keypoint a right branch would match, were it reached
        rows.append((_rec(kl, i, 3, view_cos=0.9, level_up=0, dx=0.25), _rec(kr, j, 3), d))
    out["left_ratio"] = _case(g, rows, th=3.0, takes=("left_ratio_skips_right",))
    # right records with bit 0 set and level -1 (a caller can make one; the frustum cannot)
    rows = []
    for n, (i, j) in enumerate(pairs):
        r = _rec(kr, j, 3)
        if n % 2 == 0:
            r["level"] = -1
        rows.append((_none(True), r, dr[j]))
    out["right_level"] = _case(g, rows, takes=("right_level_refused", "right_cross"))
    # windows whose best candidates are all taken by the time a point looks: occupiers, then lookers whose sorted prefix holds
    # taken keypoints only.  Ten occupiers on the left (a prefix of 1, 2 or 8 entries runs out); the right radius has no th, and no
    # right window of the golden holds nine keypoints of two adjacent levels: three occupiers there (a prefix of 1 or 2 runs out)
    rows = []
    for kps, desc, side in ((kl, dl, 0), (kr, dr, 1)):
        radius = float(F32(4.0) * g["sf"][4])
        c, taken = _dense_window(kps, desc, 10, 4, 3.0 * radius) if side == 0 else _dense_window(kps, desc, 3, 4, radius)
        for q in taken:
            here = _rec(kps, c, 3, view_cos=0.9, level_up=4 - int(kps["octave"][c]))
            rows.append((here, _none(True), desc[q]) if side == 0 else (_none(True), here, desc[q]))
        for n in range(6):
            here = _rec(kps, c, 3 if n % 2 else 1, view_cos=0.9, level_up=4 - int(kps["octave"][c]))
            d = desc[c].copy()
            d[n] ^= np.uint8(1 << n)
            rows.append((here, _none(False), d) if side == 0 else (_none(False), here, d))
    out["prefix_overflow"] = _case(g, rows, th=3.0, nnratio=1.0, l2r=np.full(nl, -1, np.int32), r2l=np.full(nr, -1, np.int32),
                                   takes=("left_direct", "right_direct"))
    _cache["c"] = out
    return out


def over_capacity_points(n=4097):
    """n copies of a MapPoint that both cameras see and that is not far (the UNSUPPORTED path: more than 4096 points handed
    on) -> (points, descriptors, the point's index in the scene)"""
    s = scene()
    _, _, (tl, tr) = scene_records(True)
    c = cases()["scene_th3"]
    _, m, _ = RR.search_by_projection_rig(c["tl"], c["tr"], c["desc"], c["kl"], c["dl"], c["kr"], c["dr"], c["l2r"], c["r2l"],
                                          s["sf"], BOUNDS, 3.0, 0.8, None)
    both = np.nonzero((tl["flags"] & tr["flags"] & 1) != 0)[0]
    i = int(next(k for k in both if (m == k).any()))  # one the matcher does place
    return np.repeat(s["pts"][i:i + 1], n), np.repeat(s["desc"][i:i + 1], n, axis=0), i
