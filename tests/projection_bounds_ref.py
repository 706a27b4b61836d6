"""CPU reference for the matchers that run after initialisation, over a Frame / KeyFrame grid with float bounds:
numpy float32 / float64 restatements of

  * FMatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)             fmatcher.cpp:2471-2687
  * FMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)  fmatcher.cpp:2689-2811
  * FMatcher::SearchByProjection(pKF, Scw, vpPoints, ..., th, ratioHamming) x 2  fmatcher.cpp:750-863, :865-981
  * FMatcher::SearchByProjection(F, vpMapPoints, th, ...)                        fmatcher.cpp:321-411
  * the search half of FMatcher::Fuse (both overloads)                           fmatcher.cpp:1918-2243
  * FMatcher::SearchBySim3                                                       fmatcher.cpp:2245-2469

restated from oracle/orb_oracle.cpp with `bounds` = Frame::(mnMinX, mnMaxX, mnMinY, mnMaxY) in place of the image size.

Frame side (the first, second and fourth form): the grid is undistort_ref.Grid (frame.cpp:322-323, 678-756) and the
in-image test the closed interval `u < mnMinX || u > mnMaxX` over the floats (fmatcher.cpp:2514-2517, 2719-2722).

KeyFrame side (both Sim3 projection forms, Fuse, SearchBySim3): a KeyFrame holds the bounds as `const int`
(keyframe.h:255-258), initialised from the Frame's floats (keyframe.cpp:44), i.e. truncated toward zero, while its cells
are the Frame's (binned with the float bounds, keyframe.cpp:58-67) and its mfGridElement*Inv the Frame's floats (:36).
So KeyFrame::GetFeaturesInArea (keyframe.cpp:655-699) takes its window origin from the integers and KeyFrame::IsInImage
(:701-703) is `x >= (int)mnMinX && x < (int)mnMaxX`: a projection between mnMinX and ceil(mnMinX), or between
floor(mnMaxX) and mnMaxX, is outside.  KfGrid / kf_bounds restate that; `kf_truncate=False` evaluates the KeyFrame forms
over the untruncated floats instead, only so that a test can show that its inputs tell the two readings apart.

At bounds (0, W, 0, H) every function equals the oracle's (tests/test_projection_bounds_cpu.py pins that).

numpy float32 / float64 scalar operations are IEEE operations without contraction, so the results are bit-exact
references for the device kernels.  `stats`, where given, collects what the tests assert about their inputs: the
accepted queries' projections and the matched keypoints ("accepted"), and per query the exit it took ("exit": one of
EXITS; of the gates inside the candidate loop the deepest one that any candidate of the query reached).

search_for_triangulation restates the candidate loop of FMatcher::SearchForTriangulation (fmatcher.cpp:1242-1482) with
Pinhole::epipolarConstrain (pinhole.cpp:128-142); its exits are TRI_EXITS.
"""
import math

import numpy as np

from oracle import orbo
from undistort_ref import COLS, ROWS, Grid, _round_half_away, _three_maxima, hamming

F32 = np.float32
HISTO = 30
INT_MIN = -2**31


def kf_bounds(bounds, truncate=True):
    """KeyFrame::mnMinX, mnMaxX, mnMinY, mnMaxY: `const int` copies of the Frame's floats, read back as float"""
    return [F32(int(F32(v))) if truncate else F32(v) for v in bounds]


class KfGrid(Grid):
    """a KeyFrame's grid: the Frame's cells and inverses, the window origin of GetFeaturesInArea from the int bounds"""

    def __init__(self, kps, bounds, truncate=True):
        Grid.__init__(self, kps, bounds)
        self.minX, _, self.minY, _ = kf_bounds(bounds, truncate)


def _gemm_row(r, x, t, dbl):
    """cv::gemm row: products accumulated in double and rounded once, or plain float arithmetic"""
    if dbl:
        s = 0.0
        for k in range(3):
            s += float(r[k]) * float(x[k])
        return F32(s + float(t))
    s = F32(0)
    for k in range(3):
        s = F32(s + F32(F32(r[k]) * F32(x[k])))
    return F32(s + F32(t))


def _norm(p):
    """cv::norm(NORM_L2) of a CV_32F vector: double accumulation"""
    n2 = 0.0
    for k in range(3):
        n2 += float(p[k]) * float(p[k])
    return F32(math.sqrt(n2))


def _dot(a, b):
    d = 0.0
    for k in range(3):
        d += float(a[k]) * float(b[k])
    return d


def _predict_level(max_dist, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale (mappoint.cpp:506-538); out-of-range conversions as cvttss2si gives them"""
    with np.errstate(all="ignore"):
        ratio = F32(max_dist) / F32(dist)
        lv = F32(np.ceil(F32(F32(orbo.logf(float(ratio))) / F32(log_scale_factor))))
    lvl = INT_MIN if (lv != lv or lv >= F32(2147483648.0) or lv < F32(-2147483648.0)) else int(lv)
    return 0 if lvl < 0 else min(lvl, nlevels - 1)


def _project(fx, fy, cx, cy, xc, yc, zc):
    """Pinhole::project (pinhole.cpp:13-16)"""
    with np.errstate(all="ignore"):
        return F32(F32(F32(fx) * xc) / zc + F32(cx)), F32(F32(F32(fy) * yc) / zc + F32(cy))


def _in_closed(u, v, b):
    return not (u < b[0] or u > b[1]) and not (v < b[2] or v > b[3])


def _is_in_image(u, v, b):
    return bool(u >= b[0] and u < b[1] and v >= b[2] and v < b[3])


def _note(stats, u, v, idx):
    if stats is not None:
        stats.setdefault("accepted", []).append((float(u), float(v), int(idx)))


EXITS = ("flag", "behind", "bounds", "range", "angle", "window", "level", "right", "chi2", "occupied", "threshold",
         "ratio", "rotation", "accepted")
_CAND_GATES = ("window", "level", "occupied", "right", "chi2")  # the candidate loop's gates, in the order they come


def _exit(stats, i, name):
    if stats is not None:
        stats.setdefault("exit", {})[int(i)] = name


class _Reach:
    """the deepest gate of the candidate loop that rejected a candidate of one query"""

    def __init__(self, gates=_CAND_GATES):
        self.gates, self.g = gates, 0

    def at(self, name):
        self.g = max(self.g, self.gates.index(name))

    @property
    def name(self):
        return self.gates[self.g]


def _to_int(v):
    """float -> int as cvttss2si converts it on the reference's x86-64 build: NaN and out-of-range give INT_MIN"""
    return INT_MIN if (v != v or v >= 2147483648.0 or v < -2147483648.0) else int(v)


def _query(grid, x, y, r, min_level, max_level, reach=None):
    """Grid.query (GetFeaturesInArea) for any float, a non-finite projection included (fmatcher.cpp's frame and keyframe
    forms let u = NaN through their bounds test); `reach` learns which gate rejected the keypoints of the cell range"""
    x, y, r = F32(x), F32(y), F32(r)
    with np.errstate(all="ignore"):
        dx, dy = F32(x - grid.minX), F32(y - grid.minY)
        c0 = max(0, _to_int(np.floor(F32(F32(dx - r) * grid.invW))))
        c1 = min(COLS - 1, _to_int(np.ceil(F32(F32(dx + r) * grid.invW))))
        r0 = max(0, _to_int(np.floor(F32(F32(dy - r) * grid.invH))))
        r1 = min(ROWS - 1, _to_int(np.ceil(F32(F32(dy + r) * grid.invH))))
    out = []
    if c0 >= COLS or c1 < 0 or r0 >= ROWS or r1 < 0:
        return out
    check = min_level > 0 or max_level >= 0
    for ix in range(c0, c1 + 1):
        for iy in range(r0, r1 + 1):
            for i in grid.cells.get((ix, iy), ()):
                o = int(grid.kps["octave"][i])
                if check and (o < min_level or (max_level >= 0 and o > max_level)):
                    if reach is not None:
                        reach.at("level")
                    continue
                if abs(F32(grid.kps["x"][i] - x)) < r and abs(F32(grid.kps["y"][i] - y)) < r:
                    out.append(i)
    return out


def _rot_bin(a1, a2):
    rot = F32(F32(a1) - F32(a2))
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    b = _round_half_away(F32(rot * (F32(1.0) / F32(HISTO))))
    return 0 if b == HISTO else b


def _drop_rotation_outliers(rot_hist, match, nm, stats=None, who=None):
    """`who`: per rot_hist entry the query that made it, for the "rotation" exit"""
    keep = _three_maxima([len(h) for h in rot_hist])
    for i in range(HISTO):
        if i not in keep:
            for k, idx in enumerate(rot_hist[i]):
                match[idx] = -1
                nm -= 1
                if who is not None:
                    _exit(stats, who[i][k], "rotation")
    return nm


def projection_direction(Tcw, Tlw, mb, mono, gemm_double):
    """fmatcher.cpp:2482-2495: twc = -Rcw.t()*tcw, tlc = Rlw*twc + tlw"""
    Tcw = np.asarray(Tcw, F32).reshape(3, 4)
    Tlw = np.asarray(Tlw, F32).reshape(3, 4)
    twc = np.zeros(3, F32)
    for r in range(3):
        if gemm_double:
            twc[r] = F32(_dot(Tcw[:, r], Tcw[:, 3]) * -1.0)
        else:
            s = F32(0)
            for k in range(3):
                s = F32(s + F32(Tcw[k, r] * Tcw[k, 3]))
            twc[r] = -s
    z = _gemm_row(Tlw[2, :3], twc, Tlw[2, 3], gemm_double)
    return bool(z > F32(mb) and not mono), bool(-z > F32(mb) and not mono)


def search_by_projection_frame(Tcw, Tlw, cam, th, last_kps, flags, x3dw, mp_desc, cur_kps, cur_desc, mvu_right,
                               scale_factors, bounds, mono=False, check_ori=True, occupied=None, gemm_double=True,
                               stats=None):
    """-> (nmatches, matchCur[n2] = last-frame index or -1, (bForward, bBackward)); cam = (fx, fy, cx, cy, mbf, mb)"""
    TH_HIGH = 100
    fx, fy, cx, cy, mbf, mb = (F32(v) for v in cam)
    T = np.asarray(Tcw, F32).reshape(3, 4)
    b = [F32(v) for v in bounds]
    fwd, bwd = projection_direction(Tcw, Tlw, mb, mono, gemm_double)
    n2 = len(cur_kps)
    match = np.full(n2, -1, np.int32)
    occ = np.zeros(n2, np.uint8) if occupied is None else np.asarray(occupied, np.uint8).copy()
    grid = Grid(cur_kps, bounds)
    dist = hamming(mp_desc, cur_desc) if len(last_kps) and n2 else None
    rot_hist, who = [[] for _ in range(HISTO)], [[] for _ in range(HISTO)]
    nm = 0
    for i in range(len(last_kps)):
        if not flags[i] & 1:
            _exit(stats, i, "flag")
            continue
        xc, yc, zc = (_gemm_row(T[r, :3], x3dw[i], T[r, 3], gemm_double) for r in range(3))
        with np.errstate(all="ignore"):
            invzc = F32(np.float64(1.0) / np.float64(zc))
        if invzc < 0:
            _exit(stats, i, "behind")
            continue
        u, v = _project(fx, fy, cx, cy, xc, yc, zc)
        if not _in_closed(u, v, b):
            _exit(stats, i, "bounds")
            continue
        o = int(last_kps["octave"][i])
        radius = F32(F32(th) * F32(scale_factors[o]))
        lv = (o, -1) if fwd else (0, o) if bwd else (o - 1, o + 1)
        best, best_i = 256, -1
        reach = _Reach()
        for i2 in _query(grid, u, v, radius, *lv, reach):
            if occ[i2]:
                reach.at("occupied")
                continue
            if mvu_right[i2] > 0:
                with np.errstate(all="ignore"):
                    ur = F32(u - F32(mbf * invzc))
                if abs(F32(ur - F32(mvu_right[i2]))) > radius:
                    reach.at("right")
                    continue
            if dist[i, i2] < best:
                best, best_i = int(dist[i, i2]), i2
        if best <= TH_HIGH:
            match[best_i] = i
            if flags[i] & 2:
                occ[best_i] = 1
            nm += 1
            _note(stats, u, v, best_i)
            _exit(stats, i, "accepted")
            if check_ori:
                k = _rot_bin(last_kps["angle"][i], cur_kps["angle"][best_i])
                rot_hist[k].append(best_i)
                who[k].append(i)
        else:
            _exit(stats, i, reach.name if best_i < 0 else "threshold")
    if check_ori:
        nm = _drop_rotation_outliers(rot_hist, match, nm, stats, who)
    return nm, match, (fwd, bwd)


def search_by_projection_mappoints(mps, mp_desc, cur_kps, cur_desc, mvu_right, scale_factors, bounds, th=1.0, nnratio=0.8,
                                   occupied=None, stats=None):
    """-> (nmatches, matchCur[n2] = MapPoint index or -1); no bound test of its own (Frame::isInFrustum is the caller's)"""
    TH_HIGH = 100
    n2 = len(cur_kps)
    match = np.full(n2, -1, np.int32)
    occ = np.zeros(n2, np.uint8) if occupied is None else np.asarray(occupied, np.uint8).copy()
    grid = Grid(cur_kps, bounds)
    dist = hamming(mp_desc, cur_desc) if len(mps) and n2 else None
    th, nnratio = F32(th), F32(nnratio)
    nm = 0
    for i in range(len(mps)):
        mp = mps[i]
        if not int(mp["flags"]) & 1:
            _exit(stats, i, "flag")
            continue
        lvl = int(mp["level"])
        r = F32(2.5) if float(mp["view_cos"]) > 0.998 else F32(4.0)
        if th != 1.0:
            r = F32(r * th)
        rs = F32(r * F32(scale_factors[lvl]))
        bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
        reach = _Reach()
        for idx in _query(grid, mp["proj_x"], mp["proj_y"], rs, lvl - 1, lvl, reach):
            if occ[idx]:
                reach.at("occupied")
                continue
            if mvu_right[idx] > 0 and abs(F32(F32(mp["proj_xr"]) - F32(mvu_right[idx]))) > rs:
                reach.at("right")
                continue
            d = int(dist[i, idx])
            if d < bd:
                bd2, bd, bl2, bl, bi = bd, d, bl, int(cur_kps["octave"][idx]), idx
            elif d < bd2:
                bl2, bd2 = int(cur_kps["octave"][idx]), d
        if bd <= TH_HIGH:
            if bl == bl2 and F32(bd) > F32(nnratio * F32(bd2)):
                _exit(stats, i, "ratio")
                continue
            match[bi] = i
            if int(mp["flags"]) & 2:
                occ[bi] = 1
            nm += 1
            _note(stats, mp["proj_x"], mp["proj_y"], bi)
            _exit(stats, i, "accepted")
        else:
            _exit(stats, i, reach.name if bi < 0 else "threshold")
    return nm, match


def search_by_projection_keyframe(Tcw, Ow, cam, th, orb_dist, log_scale_factor, kf_kps, flags, x3dw, min_dist, max_dist,
                                  mp_desc, cur_kps, cur_desc, scale_factors, bounds, check_ori=True, occupied=None,
                                  gemm_double=True, stats=None):
    """-> (nmatches, match_cur[n_cur] = KeyFrame keypoint index or -1); cam = (fx, fy, cx, cy)"""
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Ow = np.asarray(Ow, F32).reshape(3)
    b = [F32(v) for v in bounds]
    n2 = len(cur_kps)
    match = np.full(n2, -1, np.int32)
    has = np.zeros(n2, np.uint8) if occupied is None else np.asarray(occupied, np.uint8).copy()
    grid = Grid(cur_kps, bounds)
    dist = hamming(mp_desc, cur_desc) if len(kf_kps) and n2 else None
    rot_hist, who = [[] for _ in range(HISTO)], [[] for _ in range(HISTO)]
    nm = 0
    for i in range(len(kf_kps)):
        if not flags[i] & 1:
            _exit(stats, i, "flag")
            continue
        xc, yc, zc = (_gemm_row(T[r, :3], x3dw[i], T[r, 3], gemm_double) for r in range(3))
        u, v = _project(fx, fy, cx, cy, xc, yc, zc)  # no depth test in this overload
        if not _in_closed(u, v, b):
            _exit(stats, i, "bounds")
            continue
        d3 = _norm(np.asarray(x3dw[i], F32) - Ow)
        if d3 < min_dist[i] or d3 > max_dist[i]:
            _exit(stats, i, "range")
            continue
        lvl = _predict_level(max_dist[i], d3, log_scale_factor, len(scale_factors))
        radius = F32(F32(th) * F32(scale_factors[lvl]))
        best, best_i = 256, -1
        reach = _Reach()
        for i2 in _query(grid, u, v, radius, lvl - 1, lvl + 1, reach):
            if has[i2]:
                reach.at("occupied")
                continue
            if dist[i, i2] < best:
                best, best_i = int(dist[i, i2]), i2
        if best <= orb_dist:
            match[best_i] = i
            has[best_i] = 1
            nm += 1
            _note(stats, u, v, best_i)
            _exit(stats, i, "accepted")
            if check_ori:
                k = _rot_bin(kf_kps["angle"][i], cur_kps["angle"][best_i])
                rot_hist[k].append(best_i)
                who[k].append(i)
        else:
            _exit(stats, i, reach.name if best_i < 0 else "threshold")
    if check_ori:
        nm = _drop_rotation_outliers(rot_hist, match, nm, stats, who)
    return nm, match


def search_by_projection_sim3(Tcw, Ow, cam, th, ratio_hamming, log_scale_factor, flags, x3dw, normals, min_dist, max_dist,
                              mp_desc, kf_kps, kf_desc, scale_factors, bounds, proj_variant=0, matched=None,
                              gemm_double=True, stats=None, kf_truncate=True):
    """-> (nmatches, match_kf[n_kf] = iMP or -1); cam = (fx, fy, cx, cy)"""
    TH_LOW = 50
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Ow = np.asarray(Ow, F32).reshape(3)
    b = kf_bounds(bounds, kf_truncate)
    n = len(kf_kps)
    match = np.full(n, -1, np.int32)
    taken = np.zeros(n, np.uint8) if matched is None else np.asarray(matched, np.uint8).copy()
    grid = KfGrid(kf_kps, bounds, kf_truncate)
    dist = hamming(mp_desc, kf_desc) if len(flags) and n else None
    nm = 0
    for i in range(len(flags)):
        if not flags[i] & 1:
            _exit(stats, i, "flag")
            continue
        xc, yc, zc = (_gemm_row(T[r, :3], x3dw[i], T[r, 3], gemm_double) for r in range(3))
        if zc < 0.0:
            _exit(stats, i, "behind")
            continue
        if proj_variant == 0:
            u, v = _project(fx, fy, cx, cy, xc, yc, zc)
        else:  # fmatcher.cpp:908-913
            with np.errstate(all="ignore"):
                invz = F32(F32(1) / zc)
                u, v = F32(F32(fx * F32(xc * invz)) + cx), F32(F32(fy * F32(yc * invz)) + cy)
        if not _is_in_image(u, v, b):
            _exit(stats, i, "bounds")
            continue
        PO = np.asarray(x3dw[i], F32) - Ow
        d3 = _norm(PO)
        if d3 < min_dist[i] or d3 > max_dist[i]:
            _exit(stats, i, "range")
            continue
        if _dot(PO, normals[i]) < 0.5 * float(d3):
            _exit(stats, i, "angle")
            continue
        lvl = _predict_level(max_dist[i], d3, log_scale_factor, len(scale_factors))
        radius = F32(F32(int(th)) * F32(scale_factors[lvl]))
        best, best_i = 256, -1
        reach, tested = _Reach(("window", "occupied", "level")), False  # vpMatched is asked before the level here
        for idx in _query(grid, u, v, radius, -1, -1):
            if taken[idx]:
                reach.at("occupied")
                continue
            o = int(kf_kps["octave"][idx])
            if o < lvl - 1 or o > lvl:
                reach.at("level")
                continue
            tested = True
            if dist[i, idx] < best:
                best, best_i = int(dist[i, idx]), idx
        if F32(best) <= F32(F32(TH_LOW) * F32(ratio_hamming)):
            taken[best_i] = 1
            match[best_i] = i
            nm += 1
            _note(stats, u, v, best_i)
            _exit(stats, i, "accepted")
        else:
            _exit(stats, i, "threshold" if tested else reach.name)
    return nm, match


def fuse_search(points, mp_desc, kf_kps, kf_desc, kf_u_right, scale_factors, inv_level_sigma2, Rcw, tcw, Ow, cam, th,
                log_scale_factor, bounds, sim3=False, gemm_double=True, stats=None, kf_truncate=True):
    """-> (best_idx[n], best_dist[n]); cam = (fx, fy, cx, cy, bf)"""
    fx, fy, cx, cy, bf = (F32(v) for v in cam)
    R = np.asarray(Rcw, F32).reshape(3, 3)
    t = np.asarray(tcw, F32).reshape(3)
    Ow = np.asarray(Ow, F32).reshape(3)
    b = kf_bounds(bounds, kf_truncate)
    n = len(points)
    bi = np.full(n, -1, np.int32)
    bd = np.full(n, 256, np.int32)
    grid = KfGrid(kf_kps, bounds, kf_truncate)
    dist = hamming(mp_desc, kf_desc) if n and len(kf_kps) else None
    for i in range(n):
        mp = points[i]
        if not mp["valid"]:
            _exit(stats, i, "flag")
            continue
        p = mp["pos"]
        xc, yc, zc = (_gemm_row(R[r], p, t[r], gemm_double) for r in range(3))
        if zc < 0.0:
            _exit(stats, i, "behind")
            continue
        with np.errstate(all="ignore"):
            invz = F32(F32(1) / zc)
        u, v = _project(fx, fy, cx, cy, xc, yc, zc)
        if not _is_in_image(u, v, b):
            _exit(stats, i, "bounds")
            continue
        ur = F32(u - F32(bf * invz))
        PO = np.asarray(p, F32) - Ow
        d3 = _norm(PO)
        if d3 < mp["min_distance"] or d3 > mp["max_distance"]:
            _exit(stats, i, "range")
            continue
        if _dot(PO, mp["normal"]) < 0.5 * float(d3):
            _exit(stats, i, "angle")
            continue
        lvl = _predict_level(mp["max_distance"], d3, log_scale_factor, len(scale_factors))
        radius = F32(F32(th) * F32(scale_factors[lvl]))
        best, best_i = (2**31 - 1 if sim3 else 256), -1
        reach, tested = _Reach(), False
        for idx in _query(grid, u, v, radius, -1, -1):
            o = int(kf_kps["octave"][idx])
            if o < lvl - 1 or o > lvl:
                reach.at("level")
                continue
            if not sim3:
                ex, ey = F32(u - kf_kps["x"][idx]), F32(v - kf_kps["y"][idx])
                e2 = F32(F32(ex * ex) + F32(ey * ey))
                right = kf_u_right[idx] >= 0
                if right:
                    er = F32(ur - F32(kf_u_right[idx]))
                    e2 = F32(e2 + F32(er * er))
                chi2 = F32(e2 * F32(inv_level_sigma2[o]))
                if stats is not None:  # for the rows that are built to land on the literal
                    stats.setdefault("chi2", {})[(i, int(idx))] = chi2
                if float(chi2) > (7.8 if right else 5.99):
                    reach.at("chi2")
                    continue
            tested = True
            if dist[i, idx] < best:
                best, best_i = int(dist[i, idx]), idx
        if best_i >= 0:
            bi[i], bd[i] = best_i, best
            _note(stats, u, v, best_i)
            _exit(stats, i, "accepted")
        else:  # "threshold": a candidate at the greatest distance, 256, fails `dist < bestDist` of the first overload
            _exit(stats, i, "threshold" if tested else reach.name)
    return bi, bd


def _sim3_direction(valid, x3dw, mn, mx, desc, Ra, ta, Rb, tb, cam, th, log_scale_factor, kf_kps, kf_desc, scale_factors,
                    bounds, gemm_double, stats, kf_truncate=True):
    """fmatcher.cpp:2291-2368 (and its mirror :2371-2448)"""
    TH_HIGH = 100
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    Ra, Rb = np.asarray(Ra, F32).reshape(3, 3), np.asarray(Rb, F32).reshape(3, 3)
    ta, tb = np.asarray(ta, F32).reshape(3), np.asarray(tb, F32).reshape(3)
    b = kf_bounds(bounds, kf_truncate)
    out = np.full(len(valid), -1, np.int32)
    grid = KfGrid(kf_kps, bounds, kf_truncate)
    dist = hamming(desc, kf_desc) if len(valid) and len(kf_kps) else None
    for i in range(len(valid)):
        if not valid[i]:
            _exit(stats, i, "flag")
            continue
        c1 = [_gemm_row(Ra[r], x3dw[i], ta[r], gemm_double) for r in range(3)]
        c2 = [_gemm_row(Rb[r], c1, tb[r], gemm_double) for r in range(3)]
        if c2[2] < 0.0:
            _exit(stats, i, "behind")
            continue
        with np.errstate(all="ignore"):
            invz = F32(np.float64(1.0) / np.float64(c2[2]))
            u, v = F32(F32(fx * F32(c2[0] * invz)) + cx), F32(F32(fy * F32(c2[1] * invz)) + cy)
        if not _is_in_image(u, v, b):
            _exit(stats, i, "bounds")
            continue
        d3 = _norm(c2)
        if d3 < mn[i] or d3 > mx[i]:
            _exit(stats, i, "range")
            continue
        lvl = _predict_level(mx[i], d3, log_scale_factor, len(scale_factors))
        radius = F32(F32(th) * F32(scale_factors[lvl]))
        best, best_i = 2**31 - 1, -1
        reach = _Reach()
        for idx in _query(grid, u, v, radius, -1, -1):
            o = int(kf_kps["octave"][idx])
            if o < lvl - 1 or o > lvl:
                reach.at("level")
                continue
            if dist[i, idx] < best:
                best, best_i = int(dist[i, idx]), idx
        if best <= TH_HIGH:
            out[i] = best_i
            _note(stats, u, v, best_i)
            _exit(stats, i, "accepted")
        else:
            _exit(stats, i, reach.name if best_i < 0 else "threshold")
    return out


def search_by_sim3(valid1, x1, mn1, mx1, desc1, kps1, R1w, t1w, valid2, x2, mn2, mx2, desc2, kps2, R2w, t2w, sR12, t12, sR21,
                   t21, cam, th, log_scale_factor, scale_factors, bounds, gemm_double=True, stats=None, kf_truncate=True):
    """-> (nFound, match12[n1] = idx2 or -1, (vnMatch1, vnMatch2))"""
    vn1 = _sim3_direction(valid1, x1, mn1, mx1, desc1, R1w, t1w, sR21, t21, cam, th, log_scale_factor, kps2, desc2,
                          scale_factors, bounds, gemm_double, stats, kf_truncate)
    vn2 = _sim3_direction(valid2, x2, mn2, mx2, desc2, R2w, t2w, sR12, t12, cam, th, log_scale_factor, kps1, desc1,
                          scale_factors, bounds, gemm_double, None, kf_truncate)
    m12 = np.full(len(vn1), -1, np.int32)
    n = 0
    for i1 in range(len(vn1)):
        if vn1[i1] >= 0 and vn2[vn1[i1]] == i1:
            m12[i1] = vn1[i1]
            n += 1
    return n, m12, (vn1, vn2)


TRI_EXITS = ("node", "flag", "stereo", "threshold", "epipole", "chi2", "rotation", "accepted")
_TRI_GATES = ("flag", "stereo", "threshold", "epipole", "chi2")


def search_for_triangulation(kps1, desc1, has_mp1, u_right1, fv1, kps2, desc2, has_mp2, u_right2, fv2, scale_factors2,
                             level_sigma2_2, F12, ep, only_stereo=False, coarse=False, check_ori=True, stats=None):
    """FMatcher::SearchForTriangulation (fmatcher.cpp:1242-1482, pinhole, no second camera) -> (nmatches, match12[n1]).
    fv*: dicts with fv_nodes / fv_off / fv_feat.  stats["exit"][idx1] is one of TRI_EXITS ("node": the feature's
    vocabulary node is not in the other KeyFrame), stats["dsqr"][(idx1, idx2)] the float Pinhole::epipolarConstrain
    compares, stats["epi"][(idx1, idx2)] the squared distance to the epipole."""
    TH_LOW = 50
    F = np.asarray(F12, F32).reshape(9)
    epx, epy = F32(ep[0]), F32(ep[1])
    n1 = len(kps1)
    match = np.full(n1, -1, np.int32)
    dist = hamming(desc1, desc2) if n1 and len(kps2) else None
    nodes1, off1, feat1 = (np.asarray(fv1[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    nodes2, off2, feat2 = (np.asarray(fv2[k]) for k in ("fv_nodes", "fv_off", "fv_feat"))
    where2 = {int(n): j for j, n in enumerate(nodes2)}
    rot_hist, who = [[] for _ in range(HISTO)], [[] for _ in range(HISTO)]
    nm = 0
    for j1, node in enumerate(nodes1):
        j2 = where2.get(int(node))
        for idx1 in feat1[off1[j1]:off1[j1 + 1]]:
            idx1 = int(idx1)
            if j2 is None:
                _exit(stats, idx1, "node")
                continue
            if has_mp1[idx1]:
                _exit(stats, idx1, "flag")
                continue
            stereo1 = u_right1[idx1] >= 0
            if only_stereo and not stereo1:
                _exit(stats, idx1, "stereo")
                continue
            x1, y1 = F32(kps1["x"][idx1]), F32(kps1["y"][idx1])
            a = F32(F32(F32(x1 * F[0]) + F32(y1 * F[3])) + F[6])
            b = F32(F32(F32(x1 * F[1]) + F32(y1 * F[4])) + F[7])
            c = F32(F32(F32(x1 * F[2]) + F32(y1 * F[5])) + F[8])
            den = F32(F32(a * a) + F32(b * b))
            best, best_i = TH_LOW, -1
            reach = _Reach(_TRI_GATES)
            for idx2 in feat2[off2[j2]:off2[j2 + 1]]:
                idx2 = int(idx2)
                if has_mp2[idx2]:
                    continue
                stereo2 = u_right2[idx2] >= 0
                if only_stereo and not stereo2:
                    reach.at("stereo")
                    continue
                d = int(dist[idx1, idx2])
                if d > TH_LOW or d > best:
                    reach.at("threshold")
                    continue
                x2, y2, o2 = F32(kps2["x"][idx2]), F32(kps2["y"][idx2]), int(kps2["octave"][idx2])
                if not stereo1 and not stereo2:
                    ex, ey = F32(epx - x2), F32(epy - y2)
                    e2 = F32(F32(ex * ex) + F32(ey * ey))
                    if stats is not None:
                        stats.setdefault("epi", {})[(idx1, idx2)] = e2
                    if e2 < F32(F32(100) * F32(scale_factors2[o2])):
                        reach.at("epipole")
                        continue
                ok = bool(coarse)
                if not ok and den != 0:
                    num = F32(F32(F32(a * x2) + F32(b * y2)) + c)
                    dsqr = F32(F32(num * num) / den)
                    if stats is not None:
                        stats.setdefault("dsqr", {})[(idx1, idx2)] = dsqr
                    ok = float(dsqr) < 3.84 * float(F32(level_sigma2_2[o2]))
                if not ok:
                    reach.at("chi2")
                    continue
                best, best_i = d, idx2
            if best_i >= 0:
                match[idx1] = best_i
                nm += 1
                _exit(stats, idx1, "accepted")
                if check_ori:
                    k = _rot_bin(kps1["angle"][idx1], kps2["angle"][best_i])
                    rot_hist[k].append(idx1)
                    who[k].append(idx1)
            else:
                _exit(stats, idx1, reach.name)
    if check_ori:
        nm = _drop_rotation_outliers(rot_hist, match, nm, stats, who)
    return nm, match
