"""Closed-boundary gate tables for the matchers that project a MapPoint before they compare descriptors: one table per
entry point, every row one query that lands ON a gate of the reference, one float inside it, or one float outside it.
No GPU in here: tests/test_matcher_gates_cpu.py and tests/test_gpu_matcher_gates.py import the same tables.

  table          reference form                                                       oracle / numpy restatement
  frame          SearchByProjection(CurrentFrame, LastFrame)  fmatcher.cpp:2471-2687  search_by_projection_frame
  mappoints      SearchByProjection(F, vpMapPoints)           fmatcher.cpp:321-411    search_by_projection_mappoints
  keyframe       SearchByProjection(CurrentFrame, pKF)        fmatcher.cpp:2689-2811  search_by_projection_keyframe
  sim3proj       SearchByProjection(pKF, Scw, ...) x 2        fmatcher.cpp:750-981    search_by_projection_sim3
  fuse           Fuse(pKF, vpMapPoints, th)                   fmatcher.cpp:1918-2119  fuse_search, sim3 = 0
  fuse_sim3      Fuse(pKF, Scw, vpPoints, th, ...)            fmatcher.cpp:2121-2243  fuse_search, sim3 = 1
  sim3dir        SearchBySim3, one direction                  fmatcher.cpp:2291-2368  _sim3_direction
  triangulation  SearchForTriangulation                       fmatcher.cpp:1242-1482  search_for_triangulation

Construction.  The pose is the identity, fx = fy = 512, cx = 320, cy = 240, the image 640 x 480 and every point sits at
z = 4, so u = 512 * x / 4 + 320 is one rounding (the last addition) in each of the reference's three spellings of the
projection.  `solve` finds the float x whose projection IS a wanted u, or the nearest x whose projection is the next float
on one side of it: "one step inside" is chosen in the projected value, not in x (one ulp below x = 0.625 projects to 640
again), and the CPU test asserts the projected value the row names.  A depth of -0.0 cannot reach a depth gate: Rcw * p +
tcw accumulates from +0.0 (cv::gemm), and +0 + -0 = +0, so the rows at z = -0.0 arrive as zc = +0 like their z = +0 twins,
pass `1 / zc < 0` and `zc < 0` alike and leave at the bounds with u = -inf.

Each row owns a slot of a 64 px lattice (or a place on the image border, half a pitch away from the slots) and the one or
two keypoints there carry the row's descriptor with k bits flipped, i.e. at Hamming distance exactly k.  The largest window
radius is th * scale[7] < 32, so no row sees another row's keypoints; rows that share a slot say so (`share`).  The
triangulation table isolates its rows by vocabulary node instead.

A row is a dict: gate, line (the reference line it restates), side (inside / on / outside / non-finite), group (siblings
share it), expect (keypoint index, -1 = no match; a dict {run name: index} where the row is built for some runs only),
exit (the exit projection_bounds_ref records for it; a dict per run likewise), and the query itself."""
import numpy as np

import projection_bounds_ref as R
from oracle import orbo

F32 = np.float32
W, H = 640, 480
FX = FY = F32(512.0)
CX, CY = F32(320.0), F32(240.0)
Z = F32(4.0)
BOUNDS = np.array([0, W, 0, H], np.float32)
LSF = float(np.log(np.float32(1.2)).astype(np.float32))
MB = F32(0.5371)    # stereo baseline of the frame form (bForward = tlc.z > mb)
BF = F32(40.0)      # mbf: ur = u - 40 / 4 = u - 10, exact
POSE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)  # [I | 0]
OW = np.zeros(3, np.float32)
PITCH = 64
MAX_ROWS, MAX_KPS = 96, 192

_tab = {}


def tables():
    """the extractor's level tables (scale 1.2, 8 levels), as the device context computes them"""
    if not _tab:
        _tab.update(orbo.Extractor(1000).tables())
    return _tab


def up(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(np.inf))
    return x


def down(x, n=1):
    x = F32(x)
    for _ in range(n):
        x = np.nextafter(x, F32(-np.inf))
    return x


def project(x, f=FX, c=CX, z=Z):
    """Pinhole::project (pinhole.cpp:13-16) of one coordinate"""
    with np.errstate(all="ignore"):
        return F32(F32(F32(f) * F32(x)) / F32(z) + F32(c))


def solve(target, f=FX, c=CX, side=0):
    """the float x with project(x) == target; side = +-1: the nearest x on that side whose projection differs"""
    target = F32(target)
    x = F32((float(target) - float(c)) * float(Z) / float(f))
    for _ in range(64):
        p = project(x, f, c)
        if p == target:
            break
        x = up(x) if p < target else down(x)
    assert project(x, f, c) == target, target
    while side and project(x, f, c) == target:
        x = up(x) if side > 0 else down(x)
    return x


def flip(desc, k, start=0):
    """the descriptor at Hamming distance exactly k: bits [start, start + k) flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + k] ^= 1
    return np.packbits(bits)


def cell(x, y):
    """PosInGrid (frame.cpp:746-756) over the integer image"""
    return (R._round_half_away(F32(F32(x) * (F32(64) / F32(W)))), R._round_half_away(F32(F32(y) * (F32(48) / F32(H)))))


def max_for_level(d3, level):
    """a maxDistance for which MapPoint::PredictScale gives `level`, away from its rounding edges"""
    return F32(d3) if level == 0 else F32(float(d3) * 1.2 ** (level - 0.5))


def max_for_ratio(d3, ratio):
    """the maxDistance with float(max / d3) == ratio exactly"""
    m = F32(F32(d3) * F32(ratio))
    for k in range(-8, 9):
        c = up(m, k) if k >= 0 else down(m, -k)
        if F32(c / F32(d3)) == F32(ratio):
            return c
    raise AssertionError((d3, ratio))


def sum_of_squares_hit(target, extra=0.0, lim=1.95, g=2.0 ** -14):
    """(ex, ey) on a 2^-14 grid, 0 < ex, ey < lim, whose float32 (ex*ex + ey*ey) + extra is exactly `target`"""
    target = F32(target)
    k = np.arange(int(0.3 / g), int(lim / g))
    ey = (k * g).astype(np.float32)
    rem = float(target) - float(extra) - ey.astype(np.float64) ** 2
    ok = rem > 0.09
    ey, rem = ey[ok], rem[ok]
    n0 = np.round(np.sqrt(rem) / g)
    for d in (0, -1, 1, -2, 2):
        ex = ((n0 + d) * g).astype(np.float32)
        val = ((ex * ex + ey * ey).astype(np.float32) + F32(extra)).astype(np.float32)
        hit = np.nonzero((val == target) & (ex > 0.3) & (ex < lim))[0]
        if len(hit):
            return F32(ex[hit[0]]), F32(ey[hit[0]])
    raise AssertionError(target)


class Table:
    def __init__(self, name, seed):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.rows, self.kps, self.runs, self._mark = [], [], [], 0
        self._free = [(F32(PITCH * i + PITCH // 2), F32(PITCH * j + PITCH // 2))
                      for j in range(H // PITCH) for i in range(W // PITCH)]
        self._edge = {"l": 0, "r": 0, "t": 0, "b": 0}

    def sided(self, run):
        """the rows' sides (inside / on / outside) are meant for this run: a table whose runs move a gate -- the frame
        form's forward / backward windows, the local-map form's th, bOnlyStereo / bCoarse -- names them for its plain runs"""
        return {"frame": run.get("kind") == "none", "mappoints": run["name"] == "th1",
                "triangulation": run["name"] == "plain"}.get(self.name, True)

    def slot(self, pred=None):
        """the next free slot centre [for which pred(u, v) holds]"""
        for k, (u, v) in enumerate(self._free):
            if pred is None or pred(u, v):
                return self._free.pop(k)
        raise AssertionError("no slot left")

    def edge(self, which):
        """a place on the image border, half a pitch away from every slot centre"""
        self._edge[which] += 1
        k = F32(PITCH * self._edge[which])
        return {"l": (F32(0), k), "r": (F32(W), k), "t": (k, F32(0)), "b": (k, F32(H))}[which]

    def new_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def kp(self, x, y, octave, desc, u_right=-1.0, occupied=0, angle=0.0):
        self.kps.append(dict(x=F32(x), y=F32(y), octave=int(octave), desc=np.asarray(desc, np.uint8), u_right=F32(u_right),
                             occupied=int(occupied), angle=F32(angle)))
        return len(self.kps) - 1

    def row(self, gate, side, line, expect, exit, group=None, **query):
        """`own`: the keypoints made for this row since the last one (a row with share=True looks at the previous row's)"""
        own = self.rows[-1]["own"] if query.get("share") else list(range(self._mark, len(self.kps)))
        self._mark = len(self.kps)
        self.rows.append(dict(gate=gate, side=side, line=line, expect=expect, exit=exit, group=group or gate, own=own, **query))
        return len(self.rows) - 1

    def outcome(self, per_row_result):
        """per row: which of its own keypoints it matched (position in `own`), -1 for none, -2 for somebody else's"""
        return [-1 if k < 0 else (r["own"].index(k) if k in r["own"] else -2) for r, k in zip(self.rows, per_row_result)]

    # ---- arrays
    def kp_arrays(self):
        n = len(self.kps)
        k = np.zeros(n, orbo.KP_DTYPE)
        for f in ("x", "y", "octave", "angle"):
            k[f] = [p[f] for p in self.kps]
        k["size"] = 31.0
        return dict(kps=k, desc=np.stack([p["desc"] for p in self.kps]),
                    u_right=np.array([p["u_right"] for p in self.kps], np.float32),
                    occupied=np.array([p["occupied"] for p in self.kps], np.uint8))

    def col(self, key, dtype, default=0):
        return np.array([r.get(key, default) for r in self.rows], dtype)

    def expected(self, run):
        """hand-written expectation per row for `run`: keypoint index, -1, or None where the row is not built for it"""
        out = []
        for r in self.rows:
            e = r["expect"]
            out.append(e.get(run["name"], e.get(run.get("kind"))) if isinstance(e, dict) else e)
        return out

    def exits(self, run):
        out = []
        for r in self.rows:
            e = r["exit"]
            out.append(e.get(run["name"], e.get(run.get("kind"))) if isinstance(e, dict) else e)
        return out


def point(u, v, z=Z, level=1, side_u=0, side_v=0):
    """the MapPoint that projects to (u, v) [or one float beside it], its distance range set for PredictScale = level"""
    pos = np.array([solve(u, FX, CX, side_u), solve(v, FY, CY, side_v), z], np.float32)
    if z < 0:  # behind the camera, projecting to the same pixel
        pos[0], pos[1] = -pos[0], -pos[1]
    d3 = R._norm(pos)
    return dict(pos=pos, normal=(pos / d3).astype(np.float32), min_distance=F32(d3 * F32(0.5)),
                max_distance=max_for_level(d3, level), d3=d3)


# ------------------------------------------------------------------------------------------------ shared row builders
def _bounds_rows(t, closed, octave, radius_reach, mk):
    """the four image bounds x (inside, on, outside).  closed: the Frame's `u > mnMaxX` rejects; else KeyFrame::IsInImage's
    half-open `u < mnMaxX`.  mk(u, v, su, sv, desc) -> the query fields of a point projecting there."""
    line = "fmatcher.cpp:2514-2517" if closed else "keyframe.cpp:701-703"
    for which, axis, bound, inward in (("l", 0, 0.0, +1), ("r", 0, float(W), -1), ("t", 1, 0.0, +1), ("b", 1, float(H), -1)):
        for side in ("inside", "on", "outside"):
            u, v = t.edge(which)
            d = t.new_desc()
            off = F32(radius_reach) * inward  # the keypoint sits inside the image, within the window of the bound
            k = t.kp(u + off if axis == 0 else u, v + off if axis == 1 else v, octave, flip(d, 7))
            s = {"inside": inward, "on": 0, "outside": -inward}[side]
            on_passes = closed or inward > 0  # the lower bounds are closed in both forms
            ok = side == "inside" or (side == "on" and on_passes)
            q = mk(u, v, s if axis == 0 else 0, s if axis == 1 else 0, d)
            want = project(q["pos"][axis], FX if axis == 0 else FY, CX if axis == 0 else CY)
            t.row("bounds", side, line, k if ok else -1, "accepted" if ok else "bounds", group="bounds-" + which,
                  proj=(axis, want, F32(bound)), **q)


def _threshold_rows(t, mk, octave, on, line, exit="threshold"):
    for side, k in (("inside", on - 1), ("on", on), ("outside", on + 1)):
        u, v = t.slot()
        d = t.new_desc()
        kp = t.kp(u + 1, v, octave, flip(d, k))
        t.row("threshold", side, line, kp if side != "outside" else -1, "accepted" if side != "outside" else exit,
              dist=k, **mk(u, v, d))


def _tie_rows(t, mk, octave, line, octave2=None, off=4.0):
    """two keypoints of one window at equal distance: the first in GetFeaturesInArea order (grid cell column-major, then
    index) wins.  Across cells the winner has the HIGHER index; inside one cell the lower index wins."""
    for name in ("cells", "index"):
        for side, da, db in (("inside", 19, 20), ("on", 20, 20), ("outside", 20, 19)):
            o = F32(off if name == "cells" else 1.0)
            u, v = t.slot(lambda u, v: (cell(u + o, v) != cell(u - o, v)) == (name == "cells"))
            xa, xb = (u + o, u - o) if name == "cells" else (u - o, u + o)
            d = t.new_desc()
            ka = t.kp(xa, v, octave, flip(d, da, 0))
            kb = t.kp(xb, v, octave if octave2 is None else octave2, flip(d, db, 100))
            first = kb if name == "cells" else ka  # the first of GetFeaturesInArea's order
            t.row("tie", side, line, ka if side == "inside" else kb if side == "outside" else first, "accepted",
                  group="tie-" + name, **mk(u, v, d))


def _window_rows(t, mk, octave, radius, line):
    """|kp.x - u| < r is strict: a keypoint exactly r away is outside"""
    for side in ("inside", "on", "outside"):
        u, v = t.slot()
        d = t.new_desc()
        x = F32(u + F32(radius))
        assert F32(x - u) == F32(radius)
        x = {"inside": down(x), "on": x, "outside": up(x)}[side]
        k = t.kp(x, v, octave, flip(d, 5))
        t.row("window", side, line, k if side == "inside" else -1, "accepted" if side == "inside" else "window",
              dx=F32(x - u), radius=F32(radius), **mk(u, v, d))
    u, v = t.slot()  # the same edge in y
    d = t.new_desc()
    t.kp(u, F32(v - F32(radius)), octave, flip(d, 5))
    t.row("window", "on", line, -1, "window", dx=F32(radius), radius=F32(radius), **mk(u, v, d))


# ------------------------------------------------------------------------------------------------ KeyFrame-side forms
def _kf_side(name, seed, th, chi2, angle, sim3dir=False, threshold=None, occupied=False):
    """fuse / fuse_sim3 / sim3dir / sim3proj: zc < 0 rejects (so -0 passes), KeyFrame::IsInImage, distance range, viewing
    angle (not SearchBySim3), PredictScale, levels [l - 1, l], chi-square (Fuse's first overload only)"""
    t = Table(name, seed)
    sf, isig2 = tables()["scale"], tables()["inv_sigma2"]

    def mk(u, v, d, level=1, su=0, sv=0, z=Z, **over):
        q = point(u, v, z, level, su, sv)
        q.update(desc=d, valid=1)
        q.update(over)
        return q

    fm = "fmatcher.cpp:"
    # flag
    for side, valid in (("inside", 1), ("outside", 0)):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 1, flip(d, 3))
        t.row("flag", side, fm + "1966", k if valid else -1, "accepted" if valid else "flag", **mk(u, v, d, valid=valid))
    # depth: zc < 0.0f.  Zero of either sign passes it and projects to -inf (x, y < 0), which fails IsInImage
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 1, flip(d, 3))
    t.row("depth", "outside", fm + "1985", -1, "behind", **mk(u, v, d, z=-Z))
    for side, z in (("on", F32(-0.0)), ("on", F32(0.0))):
        u, v = t.slot()
        d = t.new_desc()
        t.kp(u, v, 1, flip(d, 3))
        q = mk(u, v, d)
        q.update(pos=np.array([-1, -1, z], np.float32), min_distance=F32(0), max_distance=F32(8))
        t.row("depth", side, fm + "1985", -1, "bounds", zc=z, **q)
    u, v = t.slot()
    d = t.new_desc()
    k = t.kp(u, v, 1, flip(d, 3))
    t.row("depth", "inside", fm + "1985", k, "accepted", **mk(u, v, d))
    # image bounds, half-open; level 7 so that the window (and Fuse's chi-square) reaches a keypoint inside the grid
    _bounds_rows(t, False, 7, 6, lambda u, v, su, sv, d: mk(u, v, d, 12, su, sv))
    # distance range: dist3D < minDistance || dist3D > maxDistance
    for end in ("min", "max"):
        for side in ("inside", "on", "outside"):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, 0, flip(d, 3))
            q = mk(u, v, d, 0)
            if end == "min":
                q["min_distance"] = {"inside": down(q["d3"]), "on": q["d3"], "outside": up(q["d3"])}[side]
            else:  # one float above dist3D the ratio is just over 1: level 1, and octave 0 is still in [0, 1]
                q["max_distance"] = {"inside": up(q["d3"]), "on": q["d3"], "outside": down(q["d3"])}[side]
            t.row("range", side, fm + "2011", k if side != "outside" else -1, "accepted" if side != "outside" else "range",
                  group="range-" + end, **q)
    # viewing angle: PO.dot(Pn) < 0.5 * dist3D in double; Pn = (0, 0, n) makes the dot product 4 n exactly
    if angle:
        for side in ("inside", "on", "outside"):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, 1, flip(d, 3))
            q = mk(u, v, d)
            n = F32(q["d3"] / F32(8))
            assert float(n) * 4.0 == 0.5 * float(q["d3"])
            q["normal"] = np.array([0, 0, {"inside": up(n), "on": n, "outside": down(n)}[side]], np.float32)
            t.row("angle", side, fm + "2018", k if side != "outside" else -1, "accepted" if side != "outside" else "angle",
                  **q)
    # PredictScale: ceil(logf(max / dist) / logScaleFactor), clamped; levels [l - 1, l].  Two keypoints per row, the one of
    # the higher octave nearer in Hamming distance, so the level decides which wins
    for ratio, lo, group in ((F32(1.0), 0, "scale-1"), (F32(1.2), 1, "scale-1.2")):
        for side in ("inside", "on", "outside"):
            u, v = t.slot()
            d = t.new_desc()
            k_lo = t.kp(u, v, lo, flip(d, 20))
            k_hi = t.kp(u + 1, v, lo + 1, flip(d, 10))
            q = mk(u, v, d)
            q["max_distance"] = max_for_ratio(q["d3"], ratio)
            q["max_distance"] = {"inside": down, "on": F32, "outside": up}[side](q["max_distance"])
            q["ratio"] = (side, ratio)
            gone = side == "inside" and lo == 0  # a ratio below 1 is a point beyond its maxDistance
            t.row("scale", side, "mappoint.cpp:506-521", -1 if gone else k_hi if side == "outside" else k_lo,
                  "range" if gone else "accepted", group=group, level=lo + (side == "outside"), **q)
    for octave in (7, 5):  # ratio 1.2^20: level 20 clamped to the top level 7, levels [6, 7]
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, octave, flip(d, 3))
        t.row("scale", "inside" if octave == 7 else "outside", "mappoint.cpp:517-518", k if octave == 7 else -1,
              "accepted" if octave == 7 else "level", group="scale-top", level=7, **mk(u, v, d, 20.5))
    # level window [l - 1, l] at level 3
    for group, octaves in (("level-lo", (1, 2, 3)), ("level-hi", (4, 3, 2))):
        for side, octave in zip(("outside", "on", "inside"), octaves):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, octave, flip(d, 3))
            ok = octave in (2, 3)
            t.row("level", side, fm + "2046", k if ok else -1, "accepted" if ok else "level", group=group, **mk(u, v, d, 3))
    # window edge at level 0: radius = th
    _window_rows(t, lambda u, v, d: mk(u, v, d, 0), 0, F32(th) * sf[0], "keyframe.cpp:690-692")
    if chi2:
        # right coordinate: mvuRight >= 0 takes the stereo branch; ur = u - 10.  0 and -0.0 are stereo there and fail it
        for side, ur_of, ok, group in (("on", lambda u: F32(0.0), False, "right"), ("on", lambda u: F32(-0.0), False, "right"),
                                       ("outside", lambda u: F32(-1.0), True, "right"),
                                       ("inside", lambda u: F32(1e-30), False, "right"),
                                       ("inside", lambda u: F32(u - 10), True, "right-match")):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, 1, flip(d, 3), u_right=ur_of(u))
            t.row("right", side, fm + "2053", k if ok else -1, "accepted" if ok else "chi2", group=group, u_right=ur_of(u),
                  **mk(u, v, d))
        # chi-square: the float product against the double literals.  7.8f > 7.8 and 5.99f < 5.99
        for right, lit, group in ((True, 7.8, "chi2-7.8"), (False, 5.99, "chi2-5.99")):
            for side, target in (("inside", down(F32(lit))), ("on", F32(lit)), ("outside", up(F32(lit)))):
                u, v = t.slot()
                d = t.new_desc()
                er = F32(1.0) if right else F32(0.0)
                ex, ey = sum_of_squares_hit(target, float(er * er))
                k = t.kp(F32(u - ex), F32(v - ey), 0, flip(d, 3), u_right=F32(u - 10 - er) if right else -1.0)
                ok = float(target) <= lit
                t.row("chi2", side, fm + ("2060" if right else "2074"), k if ok else -1, "accepted" if ok else "chi2",
                      group=group, chi2=target, **mk(u, v, d, 0))
    # acceptance
    if threshold is not None:
        _threshold_rows(t, lambda u, v, d: mk(u, v, d), 1, threshold, fm + "2360")
    # the greatest distance, 256: `dist < bestDist` with bestDist = 256 (Fuse) or INT_MAX (Sim3 forms)
    u, v = t.slot()
    d = t.new_desc()
    k = t.kp(u, v, 1, flip(d, 256))
    first = chi2 or occupied  # the forms that start from bestDist = 256
    t.row("threshold", "on", fm + "2039", -1 if first or threshold is not None else k,
          "threshold" if first or threshold is not None else "accepted", group="dist-256", dist=256, **mk(u, v, d))
    _tie_rows(t, lambda u, v, d: mk(u, v, d), 1, "keyframe.cpp:677-696", off=1.5)
    if occupied:
        # vpMatched: set on entry, and set by an earlier query of the same call
        u, v = t.slot()
        d = t.new_desc()
        t.kp(u, v, 1, flip(d, 3), occupied=1)
        t.row("occupied", "outside", fm + "832", -1, "occupied", **mk(u, v, d))
        u, v = t.slot()
        d = t.new_desc()
        k1 = t.kp(u, v, 1, flip(d, 3))
        k2 = t.kp(u + 1, v, 1, flip(d, 9))
        t.row("occupied", "inside", fm + "852", k1, "accepted", group="occupied-dyn", **mk(u, v, d))
        t.row("occupied", "outside", fm + "832", k2, "accepted", group="occupied-dyn", share=True, **mk(u, v, d))
    # non-finite: x = y = 0 at z = +0 gives u = v = NaN, which fails IsInImage here
    u, v = t.slot()
    d = t.new_desc()
    t.kp(3, 3, 0, flip(d, 0))
    q = mk(u, v, d, 0)
    q.update(pos=np.zeros(3, np.float32), min_distance=F32(0), max_distance=F32(8))
    t.row("non-finite", "non-finite", fm + "1990", -1, "bounds", **q)
    t.th = th
    return t


def fuse():
    t = _kf_side("fuse", 11, 2.0, chi2=True, angle=True)
    t.runs = [dict(name="gemm", gemm_float=False), dict(name="float", gemm_float=True)]
    return t


def fuse_sim3():
    t = _kf_side("fuse_sim3", 12, 3.0, chi2=False, angle=True)
    t.runs = [dict(name="gemm", gemm_float=False), dict(name="float", gemm_float=True)]
    return t


def sim3dir():
    t = _kf_side("sim3dir", 13, 3.0, chi2=False, angle=False, sim3dir=True, threshold=100)
    t.runs = [dict(name="gemm", gemm_float=False), dict(name="float", gemm_float=True)]
    return t


def sim3proj():
    """ratioHamming = 1.03: TH_LOW * ratioHamming = 51.5, an int against a fractional float product"""
    t = _kf_side("sim3proj", 14, 3, chi2=False, angle=True, occupied=True)
    for side, k in (("inside", 51), ("outside", 52)):
        u, v = t.slot()
        d = t.new_desc()
        kp = t.kp(u + 1, v, 1, flip(d, k))
        q = point(u, v)
        q.update(desc=d, valid=1)
        t.row("threshold", side, "fmatcher.cpp:848", kp if k == 51 else -1, "accepted" if k == 51 else "threshold",
              group="threshold-51.5", dist=k, **q)
    t.runs = [dict(name="v%d%s" % (var, "f" if gf else ""), variant=var, gemm_float=gf, ratio=1.03)
              for var in (0, 1) for gf in (False, True)]
    return t


# ------------------------------------------------------------------------------------------------ Frame-side forms
def frame():
    """th = 7; the last frame's octave sets radius and level window; bForward / bBackward / bMono are per run"""
    t = Table("frame", 21)
    sf = tables()["scale"]
    th = F32(7.0)
    fm = "fmatcher.cpp:"

    def mk(u, v, d, octave=0, su=0, sv=0, z=Z, **over):
        q = point(u, v, z, 1, su, sv)
        q.update(desc=d, flags=3, octave=octave, angle=0.0)
        q.update(over)
        return q

    for side, fl in (("inside", 1), ("outside", 0), ("outside", 2)):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 0, flip(d, 3))
        t.row("flag", side, fm + "2499-2503", k if fl & 1 else -1, "accepted" if fl & 1 else "flag", **mk(u, v, d, flags=fl))
    # depth: invzc = 1.0 / z in double, `invzc < 0`: zc = +0 gives +inf and goes on to the bounds
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 0, flip(d, 3))
    t.row("depth", "outside", fm + "2508-2510", -1, "behind", group="depth-zero", **mk(u, v, d, z=-Z))
    for side, z, ex in (("on", F32(-0.0), "bounds"), ("on", F32(0.0), "bounds")):
        u, v = t.slot()
        d = t.new_desc()
        t.kp(u, v, 0, flip(d, 3))
        q = mk(u, v, d)
        q["pos"] = np.array([-1, -1, z], np.float32)
        t.row("depth", side, fm + "2508-2510", -1, ex, group="depth-zero", zc=z, **q)
    u, v = t.slot()
    d = t.new_desc()
    k = t.kp(u, v, 0, flip(d, 3))
    t.row("depth", "inside", fm + "2508-2510", k, "accepted", group="depth-zero", **mk(u, v, d))
    _bounds_rows(t, True, 0, 6, lambda u, v, su, sv, d: mk(u, v, d, 0, su, sv))
    _window_rows(t, lambda u, v, d: mk(u, v, d, 0), 0, th * sf[0], "frame.cpp:733-736")
    # level windows: [o - 1, o + 1]; forward [o, -1] (no upper end); backward [0, o]; last octave 2
    for group, octaves in (("level-lo", (0, 1, 2)), ("level-hi", (4, 3, 2))):  # sides as the plain window [1, 3] sees them
        for side, octave in zip(("outside", "on", "inside"), octaves):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, octave, flip(d, 3))
            ok = dict(none=octave in (1, 2, 3), fwd=octave >= 2, bwd=octave <= 2)
            t.row("level", side, fm + "2528-2535", {kind: (k if ok[kind] else -1) for kind in ok},
                  {kind: ("accepted" if ok[kind] else "level") for kind in ok}, group=group, **mk(u, v, d, 2))
    u, v = t.slot()  # last octave 0 going forward: minLevel = 0, maxLevel = -1 switches the level test off
    d = t.new_desc()
    k = t.kp(u, v, 5, flip(d, 3))
    t.row("level", "outside", "frame.cpp:712", dict(none=-1, fwd=k, bwd=-1), dict(none="level", fwd="accepted", bwd="level"),
          group="level-off", **mk(u, v, d, 0))
    # right coordinate: mvuRight > 0; ur = u - mbf * invzc = u - 10; er > radius rejects
    for side, ur_of, ok, group in (("on", lambda u: F32(0.0), True, "right-sign"), ("on", lambda u: F32(-0.0), True, "right-sign"),
                                   ("outside", lambda u: F32(-1.0), True, "right-sign"),
                                   ("inside", lambda u: F32(1e-30), False, "right-sign"),
                                   ("inside", lambda u: down(F32(u - 10 + th)), True, "right-er"),
                                   ("on", lambda u: F32(u - 10 + th), True, "right-er"),
                                   ("outside", lambda u: up(F32(u - 10 + th)), False, "right-er")):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 0, flip(d, 3), u_right=ur_of(u))
        t.row("right", side, fm + "2545-2551", k if ok else -1, "accepted" if ok else "right", group=group,
              u_right=ur_of(u), **mk(u, v, d))
    # occupied on entry; and by an earlier query with observations (flags & 2)
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 0, flip(d, 3), occupied=1)
    t.row("occupied", "outside", fm + "2541-2543", -1, "occupied", **mk(u, v, d))
    for fl in (3, 1):
        u, v = t.slot()
        d = t.new_desc()
        k1 = t.kp(u, v, 0, flip(d, 3))
        k2 = t.kp(u + 1, v, 0, flip(d, 9))
        # with observations the first query keeps k1 and the second takes k2; without, the second overwrites k1
        t.row("occupied", "inside", fm + "2562-2565", k1 if fl & 2 else -1, "accepted", group="flags&2-%d" % fl,
              **mk(u, v, d, flags=fl))
        t.row("occupied", "outside", fm + "2541-2543", k2 if fl & 2 else k1, "accepted", group="flags&2-%d" % fl, share=True,
              **mk(u, v, d))
    _threshold_rows(t, lambda u, v, d: mk(u, v, d), 0, 100, fm + "2562")
    _tie_rows(t, lambda u, v, d: mk(u, v, d), 0, "frame.cpp:712-741")
    # non-finite: x = y = 0 at z = +0 gives u = NaN, which passes `u < mnMinX || u > mnMaxX`; a keypoint waits in cell (0, 0)
    u, v = t.slot()
    d = t.new_desc()
    t.kp(3, 3, 0, flip(d, 0))
    q = mk(u, v, d)
    q["pos"] = np.zeros(3, np.float32)
    t.row("non-finite", "non-finite", "frame.cpp:686-708", -1, "window", **q)
    # rotation consistency: the only match outside the histogram's maxima
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 0, flip(d, 3))
    t.row("rotation", "outside", fm + "2668-2681", -1, "rotation", **mk(u, v, d, angle=180.0))
    t.th = th
    t.runs = [dict(name=n + ("-f" if gf else ""), kind=kind, tlw_z=z, mono=mono, gemm_float=gf)
              for n, kind, z, mono in (("on", "none", MB, False), ("fwd", "fwd", up(MB), False), ("below", "none", down(MB), False),
                                       ("bwd-on", "none", -MB, False), ("bwd", "bwd", -up(MB), False),
                                       ("mono", "none", up(MB), True), ("mono-bwd", "none", -up(MB), True))
              for gf in (False, True)]
    return t


def keyframe():
    """th = 7, ORBdist = 80; no depth test; closed bounds; PredictScale; levels [l - 1, l + 1]"""
    t = Table("keyframe", 22)
    sf = tables()["scale"]
    th = F32(7.0)
    fm = "fmatcher.cpp:"

    def mk(u, v, d, level=1, su=0, sv=0, z=Z, **over):
        q = point(u, v, z, level, su, sv)
        q.update(desc=d, flags=1, angle=0.0)
        q.update(over)
        return q

    for side, fl in (("inside", 1), ("outside", 0)):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 1, flip(d, 3))
        t.row("flag", side, fm + "2707-2711", k if fl else -1, "accepted" if fl else "flag", **mk(u, v, d, flags=fl))
    # no depth test: a point behind the camera that projects into the image is matched
    u, v = t.slot()
    d = t.new_desc()
    k = t.kp(u, v, 1, flip(d, 3))
    t.row("depth", "outside", fm + "2716", k, "accepted", **mk(u, v, d, z=-Z))
    _bounds_rows(t, True, 0, 6, lambda u, v, su, sv, d: mk(u, v, d, 0, su, sv))
    for end in ("min", "max"):
        for side in ("inside", "on", "outside"):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, 0, flip(d, 3))
            q = mk(u, v, d, 0)
            if end == "min":
                q["min_distance"] = {"inside": down(q["d3"]), "on": q["d3"], "outside": up(q["d3"])}[side]
            else:
                q["max_distance"] = {"inside": up(q["d3"]), "on": q["d3"], "outside": down(q["d3"])}[side]
            t.row("range", side, fm + "2729-2733", k if side != "outside" else -1, "accepted" if side != "outside" else "range",
                  group="range-" + end, **q)
    # PredictScale with levels [l - 1, l + 1]: octaves lo - 1 (nearer) and lo + 2 tell level lo from lo + 1
    for ratio, lo, group in ((F32(1.0), 0, "scale-1"), (F32(1.2), 1, "scale-1.2")):
        for side in ("inside", "on", "outside"):
            u, v = t.slot()
            d = t.new_desc()
            k_lo = t.kp(u, v, max(lo - 1, 0), flip(d, 10 if lo else 20))
            k_hi = t.kp(u + 1, v, lo + 2, flip(d, 20 if lo else 10))
            q = mk(u, v, d)
            q["max_distance"] = {"inside": down, "on": F32, "outside": up}[side](max_for_ratio(q["d3"], ratio))
            q["ratio"] = (side, ratio)
            gone = side == "inside" and lo == 0
            t.row("scale", side, "mappoint.cpp:523-538", -1 if gone else k_hi if side == "outside" else k_lo,
                  "range" if gone else "accepted", group=group, level=lo + (side == "outside"), **q)
    for octave in (6, 5):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, octave, flip(d, 3))
        t.row("scale", "inside" if octave == 6 else "outside", "mappoint.cpp:534-535", k if octave == 6 else -1,
              "accepted" if octave == 6 else "level", group="scale-top", level=7, **mk(u, v, d, 20.5))
    for group, octaves in (("level-lo", (0, 1, 2)), ("level-hi", (4, 3, 2))):  # level 2: [1, 3]
        for side, octave in zip(("outside", "on", "inside"), octaves):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, octave, flip(d, 3))
            ok = octave in (1, 2, 3)
            t.row("level", side, fm + "2745", k if ok else -1, "accepted" if ok else "level", group=group, **mk(u, v, d, 2))
    _window_rows(t, lambda u, v, d: mk(u, v, d, 0), 0, th * sf[0], "frame.cpp:733-736")
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 1, flip(d, 3), occupied=1)
    t.row("occupied", "outside", fm + "2756", -1, "occupied", **mk(u, v, d))
    u, v = t.slot()
    d = t.new_desc()
    k1 = t.kp(u, v, 1, flip(d, 3))
    k2 = t.kp(u + 1, v, 1, flip(d, 9))
    t.row("occupied", "inside", fm + "2771", k1, "accepted", group="occupied-dyn", **mk(u, v, d))
    t.row("occupied", "outside", fm + "2756", k2, "accepted", group="occupied-dyn", share=True, **mk(u, v, d))
    _threshold_rows(t, lambda u, v, d: mk(u, v, d), 1, 80, fm + "2768")
    _tie_rows(t, lambda u, v, d: mk(u, v, d), 1, "frame.cpp:712-741")
    # non-finite: the origin gives u = NaN (0 / 0), dist3D = 0 inside [0, 8], ratio = inf -> INT_MIN -> level 0
    u, v = t.slot()
    d = t.new_desc()
    t.kp(3, 3, 0, flip(d, 0))
    q = mk(u, v, d, 0)
    q.update(pos=np.zeros(3, np.float32), min_distance=F32(0), max_distance=F32(8))
    t.row("non-finite", "non-finite", "frame.cpp:686-708", -1, "window", **q)
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 1, flip(d, 3))
    t.row("rotation", "outside", fm + "2795-2808", -1, "rotation", **mk(u, v, d, angle=180.0))
    t.th = th
    t.runs = [dict(name="gemm", gemm_float=False, orb_dist=80), dict(name="float", gemm_float=True, orb_dist=80)]
    return t


def mappoints():
    """nnratio = 0.75; runs th = 1.0 (bFactor false), the float above 1.0, and 3.0"""
    t = Table("mappoints", 23)
    sf = tables()["scale"]
    fm = "fmatcher.cpp:"
    cos_on = F32(0.998)  # 0.998f > 0.998: RadiusByViewingCos gives 2.5 for it, 4.0 for the float below

    def mk(u, v, d, level=0, view_cos=0.5, **over):
        q = dict(proj_x=F32(u), proj_y=F32(v), proj_xr=F32(u - 10), view_cos=F32(view_cos), level=level, flags=3, desc=d)
        q.update(over)
        return q

    for side, fl in (("inside", 1), ("outside", 0), ("outside", 2)):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 0, flip(d, 3))
        t.row("flag", side, fm + "331-338", k if fl & 1 else -1, "accepted" if fl & 1 else "flag", **mk(u, v, d, flags=fl))
    # viewing cosine against the double 0.998, seen through the radius: 2.5 th or 4 th
    for dx, runs in ((3, ("th1",)), (9, ("th3",))):
        for side, c in (("inside", down(cos_on)), ("on", cos_on), ("outside", up(cos_on))):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u + dx, v, 0, flip(d, 3))
            wide = float(c) <= 0.998
            t.row("angle", side, fm + "493-499", {r: (k if wide else -1) for r in runs},
                  {r: ("accepted" if wide else "window") for r in runs}, group="viewcos-%d" % dx, **mk(u, v, d, view_cos=c))
    # window edge |dx| == r at r = 4 (th == 1.0 leaves r alone; the float above 1.0 widens it past the keypoint)
    for side in ("inside", "on", "outside"):
        u, v = t.slot()
        d = t.new_desc()
        x = {"inside": down(F32(u + 4)), "on": F32(u + 4), "outside": up(F32(u + 4))}[side]
        k = t.kp(x, v, 0, flip(d, 3))
        e = {"th1": k if side == "inside" else -1, "th1+": k if side != "outside" else -1, "th3": k}
        t.row("window", side, "frame.cpp:733-736", e, {r: ("accepted" if e[r] >= 0 else "window") for r in e},
              dx=F32(x - u), radius=F32(4), **mk(u, v, d))
    for group, octaves in (("level-lo", (0, 1, 2)), ("level-hi", (3, 2, 1))):  # level 2: [1, 2]
        for side, octave in zip(("outside", "on", "inside"), octaves):
            u, v = t.slot()
            d = t.new_desc()
            k = t.kp(u, v, octave, flip(d, 3))
            ok = octave in (1, 2)
            t.row("level", side, fm + "352-354", k if ok else -1, "accepted" if ok else "level", group=group,
                  **mk(u, v, d, 2))
    # right coordinate: mvuRight > 0; er = |proj_xr - mvuRight| > r * scale rejects (r * scale = 4 at th = 1)
    for side, ur_of, ok, group in (("on", lambda u: F32(0.0), True, "right-sign"), ("on", lambda u: F32(-0.0), True, "right-sign"),
                                   ("outside", lambda u: F32(-1.0), True, "right-sign"),
                                   ("inside", lambda u: F32(1e-30), None, "right-sign"),
                                   ("inside", lambda u: down(F32(u - 10 + 4)), True, "right-er"),
                                   ("on", lambda u: F32(u - 10 + 4), True, "right-er"),
                                   ("outside", lambda u: up(F32(u - 10 + 4)), False, "right-er")):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 0, flip(d, 3), u_right=ur_of(u))
        e = k if ok else {"th1": -1, "th1+": -1, "th3": k}  # one float of 90 is more than one float of 4
        if ok is None:  # a right coordinate that is in force and far away, at every th
            e = -1
        t.row("right", side, fm + "368-375", e,
              "accepted" if ok else "right" if ok is None else {"th1": "right", "th1+": "right", "th3": "accepted"},
              group=group, u_right=ur_of(u), **mk(u, v, d))
    u, v = t.slot()
    d = t.new_desc()
    t.kp(u, v, 0, flip(d, 3), occupied=1)
    t.row("occupied", "outside", fm + "363-365", -1, "occupied", **mk(u, v, d))
    for fl in (3, 1):
        u, v = t.slot()
        d = t.new_desc()
        k1 = t.kp(u, v, 0, flip(d, 3))
        k2 = t.kp(u + 1, v, 1, flip(d, 9))
        t.row("occupied", "inside", fm + "405", k1 if fl & 2 else -1, "accepted", group="flags&2-%d" % fl,
              **mk(u, v, d, 1, flags=fl))
        t.row("occupied", "outside", fm + "363-365", k2 if fl & 2 else k1, "accepted", group="flags&2-%d" % fl, share=True,
              **mk(u, v, d, 1))
    _threshold_rows(t, lambda u, v, d: mk(u, v, d), 0, 100, fm + "398")
    # ratio test, float: bestDist > nnratio * bestDist2 on the same level only; 0.75 * 80 = 60
    for side, best, same in (("inside", 59, True), ("on", 60, True), ("outside", 61, True), ("outside", 61, False)):
        u, v = t.slot()
        d = t.new_desc()
        k = t.kp(u, v, 1, flip(d, best))
        t.kp(u + 1, v, 1 if same else 0, flip(d, 80, 100))
        ok = best <= 60 or not same
        t.row("ratio", side, fm + "400-403", k if ok else -1, "accepted" if ok else "ratio",
              group="ratio" if same else "ratio-levels", dist=best, **mk(u, v, d, 1))
    _tie_rows(t, lambda u, v, d: mk(u, v, d, 1), 1, "frame.cpp:712-741", octave2=0)
    u, v = t.slot()
    d = t.new_desc()
    t.kp(3, 3, 0, flip(d, 0))
    t.row("non-finite", "non-finite", "frame.cpp:686-708", -1, "window", **mk(np.nan, np.nan, d))
    t.runs = [dict(name="th1", th=F32(1.0)), dict(name="th1+", th=up(F32(1.0))), dict(name="th3", th=F32(3.0))]
    t.nnratio = 0.75
    return t


# ------------------------------------------------------------------------------------------------ triangulation
def _epipolar_hit(target):
    """(B, num): with the line (1, B, 0), den = 1 + B * B and num = kp2.x (kp2.y = 0), float(num * num / den) == target"""
    for B in (0.0, 1.0, 2.0, 3.0, 0.5, 1.5, 2.5):
        den = F32(1.0 + B * B)
        n0 = F32(np.sqrt(float(target) * float(den)))
        for k in range(-16, 17):
            num = up(n0, k) if k >= 0 else down(n0, -k)
            if F32(F32(num * num) / den) == F32(target):
                return B, num
    raise AssertionError(target)


def triangulation():
    """Every row is one vocabulary node with one feature of KeyFrame 1 and one or two of KeyFrame 2.  F12 = [1 B 0; 0 0 0;
    1 B 0] gives the epipolar line (a, b, c) = (kp1.x + 1, B (kp1.x + 1), 0): (1, B, 0) for kp1.x = 0, and den = 0 for
    kp1.x = -1.  The epipole is the origin, which lies on that line."""
    t = Table("triangulation", 31)
    sig2 = tables()["sigma2"]
    fm = "fmatcher.cpp:"
    on = F32(3.84)  # 3.84f < 3.84: dsqr == 3.84f passes `dsqr < 3.84 * sigma2` at level 0
    B, num_on = _epipolar_hit(on)
    t.F12 = np.array([[1, B, 0], [0, 0, 0], [1, B, 0]], np.float32)
    t.ep = (0.0, 0.0)
    t.kps1 = []
    far = F32(1000.0)

    def add(gate, side, line, expect, exit, cands, group=None, x1=0.0, mp1=0, ur1=-1.0, angle=0.0, **extra):
        """cands: list of dict(x, y, dist, octave, ur, mp) -> KeyFrame-2 features of this row's node"""
        d = t.new_desc()
        ks = []
        for c in cands:
            ks.append(t.kp(c.get("x", 0.0), c.get("y", far), c.get("octave", 0), flip(d, c["dist"], c.get("start", 0)),
                           u_right=c.get("ur", -1.0), occupied=c.get("mp", 0)))
        e = (lambda v: v if v is None or v < 0 else ks[v])
        if not isinstance(expect, dict):  # the rows are built for the runs without bOnlyStereo unless they say otherwise
            expect, exit = dict(plain=expect, coarse=expect), dict(plain=exit, coarse=exit)
        expect = {r: e(v) for r, v in expect.items()}
        t.row(gate, side, line, expect, exit, group, x1=F32(x1), mp1=mp1, ur1=F32(ur1), angle=F32(angle), desc=d,
              cands=ks, **extra)

    # points on the line x + B y = 0 far from the epipole: (-B y, y)
    def on_line(y=far):
        return dict(x=F32(-B * float(y)), y=F32(y))

    add("flag", "inside", fm + "1313", 0, "accepted", [dict(dist=10, **on_line())])
    add("flag", "outside", fm + "1313", -1, "flag", [dict(dist=10, **on_line())], mp1=1)
    add("flag", "outside", fm + "1344", -1, "flag", [dict(dist=10, mp=1, **on_line())], group="flag-2")
    # TH_LOW: dist > TH_LOW || dist > bestDist
    for side, k in (("inside", 49), ("on", 50), ("outside", 51)):
        add("threshold", side, fm + "1352", 0 if k <= 50 else -1, "accepted" if k <= 50 else "threshold",
            [dict(dist=k, **on_line())], dist=k)
    # `dist > bestDist` skips, an equal distance replaces: the LAST of a tie wins
    for side, da, db in (("inside", 30, 31), ("on", 30, 30), ("outside", 31, 30)):
        add("tie", side, fm + "1352", 0 if side == "inside" else 1, "accepted",
            [dict(dist=da, **on_line()), dict(dist=db, start=100, **on_line())])
    # a nearer candidate that fails the epipolar test does not lower bestDist
    add("chi2", "outside", fm + "1376", dict(plain=1, coarse=0), dict(plain="accepted", coarse="accepted"),
        [dict(dist=10, x=F32(50.0), y=far), dict(dist=30, start=100, **on_line())], group="chi2-skip")
    # epipolar distance, double: dsqr < 3.84 * sigma2[octave]; stereo KeyFrame-1 features skip the epipole test
    for side, dsqr in (("inside", down(on)), ("on", on), ("outside", up(on))):
        try:
            b2, num = _epipolar_hit(dsqr)
            assert b2 == B
        except AssertionError:  # no float squares to this neighbour on this line: two floats further away
            num = down(num_on, 2) if side == "inside" else up(num_on, 2)
        got = F32(F32(num * num) / F32(1.0 + B * B))
        ok = float(got) < 3.84 * float(sig2[0])
        assert ok == (side != "outside")
        add("chi2", side, "pinhole.cpp:139-141", {"plain": 0 if ok else -1, "coarse": 0},
            {"plain": "accepted" if ok else "chi2", "coarse": "accepted"}, [dict(dist=10, x=num, y=0.0)], ur1=5.0, dsqr=got)
    add("chi2", "outside", "pinhole.cpp:134-136", {"plain": -1, "coarse": 0}, {"plain": "chi2", "coarse": "accepted"},
        [dict(dist=10, **on_line())], group="den-0", x1=-1.0)
    # distance to the epipole of mono pairs: ex * ex + ey * ey < 100 * scale[octave] rejects; on the line x = -B y
    for side, r in (("inside", up(F32(10.0))), ("on", F32(10.0)), ("outside", down(F32(10.0)))):
        if B == 0.0:
            c = dict(x=0.0, y=r)
        else:
            c = dict(x=r, y=0.0)  # off the line: these rows are for the coarse run, where the line is not asked
        ok = side != "outside"
        runs = ("plain", "coarse") if B == 0.0 else ("coarse",)
        add("epipole", side, fm + "1366-1374", {k: (0 if ok else -1) for k in runs},
            {k: ("accepted" if ok else "epipole") for k in runs}, [dict(dist=10, **c)], epi=F32(r * r))
    # a right coordinate >= 0 on either side switches the epipole test off: 0 and -0.0 are stereo
    near = dict(x=0.0, y=1.0) if B == 0.0 else dict(x=1.0, y=0.0)
    runs = ("plain", "coarse") if B == 0.0 else ("coarse",)
    add("right", "outside", fm + "1318", {k: -1 for k in runs}, {k: "epipole" for k in runs}, [dict(dist=10, **near)],
        group="right-sign")
    add("right", "inside", fm + "1318", {k: 0 for k in runs}, {k: "accepted" for k in runs}, [dict(dist=10, **near)],
        ur1=1e-30, group="right-sign")
    for ur1, ur2 in ((0.0, -1.0), (-0.0, -1.0), (-1.0, 0.0), (-1.0, -0.0)):
        add("right", "on", fm + "1318", {"plain": 0 if B == 0.0 else None, "coarse": 0, "stereo": -1},
            {"plain": "accepted" if B == 0.0 else None, "coarse": "accepted", "stereo": "stereo"},
            [dict(dist=10, ur=ur2, **(dict(x=0.0, y=1.0) if B == 0.0 else dict(x=1.0, y=0.0)))], ur1=ur1, group="right-sign")
    for ur1, ur2 in ((5.0, 5.0), (0.0, -0.0)):
        add("right", "inside", fm + "1321", dict(plain=0, coarse=0, stereo=0), dict(plain="accepted", coarse="accepted", stereo="accepted"),
            [dict(dist=10, ur=ur2, **on_line())], ur1=ur1, group="only-stereo")
    add("right", "outside", fm + "1321", {"plain": 0, "coarse": 0, "stereo": -1},
        {"plain": "accepted", "coarse": "accepted", "stereo": "stereo"}, [dict(dist=10, **on_line())], group="only-stereo")
    add("rotation", "outside", fm + "1466-1481", -1, "rotation", [dict(dist=10, **on_line())], angle=180.0)
    t.runs = [dict(name="plain", only_stereo=False, coarse=False), dict(name="coarse", only_stereo=False, coarse=True),
              dict(name="stereo", only_stereo=True, coarse=False)]
    return t


BUILDERS = dict(frame=frame, mappoints=mappoints, keyframe=keyframe, sim3proj=sim3proj, fuse=fuse, fuse_sim3=fuse_sim3,
                sim3dir=sim3dir, triangulation=triangulation)
_cache = {}


def table(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------ inputs and references
def inputs(t):
    """the arrays of a table, in the shape every implementation takes them"""
    if "in" in t.__dict__:
        return t.__dict__["in"]
    a = t.kp_arrays() if t.kps else {}
    n = len(t.rows)
    a["desc_q"] = np.stack([r["desc"] for r in t.rows])
    if t.name in ("fuse", "fuse_sim3", "sim3dir", "sim3proj"):
        p = np.zeros(n, orbo.FUSE_POINT_DTYPE)
        for i, r in enumerate(t.rows):
            for f in ("pos", "normal", "min_distance", "max_distance", "valid"):
                p[f][i] = r[f]
        a["pts"] = p
    elif t.name in ("frame", "keyframe"):
        k = np.zeros(n, orbo.KP_DTYPE)
        k["octave"] = t.col("octave", np.int32)
        k["angle"] = t.col("angle", np.float32)
        k["size"] = 31.0
        a.update(q_kps=k, flags=t.col("flags", np.uint8), x3dw=np.stack([r["pos"] for r in t.rows]).astype(np.float32),
                 mn=t.col("min_distance", np.float32), mx=t.col("max_distance", np.float32))
    elif t.name == "mappoints":
        m = np.zeros(n, orbo.MP_TRACK_DTYPE)
        for f in m.dtype.names:
            m[f] = t.col(f, m.dtype[f])
        a["mps"] = m
    elif t.name == "triangulation":
        k1 = np.zeros(n, orbo.KP_DTYPE)
        k1["x"], k1["angle"], k1["size"] = t.col("x1", np.float32), t.col("angle", np.float32), 31.0
        feat2 = [k for r in t.rows for k in r["cands"]]
        off2 = np.cumsum([0] + [len(r["cands"]) for r in t.rows]).astype(np.int32)
        nodes = np.arange(n, dtype=np.int32) * 3 + 1
        a.update(kps1=k1, mp1=t.col("mp1", np.uint8), ur1=t.col("ur1", np.float32),
                 fv1=dict(fv_nodes=nodes, fv_off=np.arange(n + 1, dtype=np.int32), fv_feat=np.arange(n, dtype=np.int32)),
                 fv2=dict(fv_nodes=nodes, fv_off=off2, fv_feat=np.array(feat2, np.int32)))
    t.__dict__["in"] = a
    return a


def frame_tlw(run):
    T = POSE.copy()
    T[2, 3] = run["tlw_z"]
    return T


CAM = (float(FX), float(FY), float(CX), float(CY))


def reference(t, run, impl, stats=None):
    """one run of a table on the CPU: impl = "orbo" (oracle/orb_oracle.cpp) or "numpy" (projection_bounds_ref, integer
    bounds) -> the raw result tuple, in the shape the device wrapper returns it"""
    a = inputs(t)
    sf, isig2, sig2 = tables()["scale"], tables()["inv_sigma2"], tables()["sigma2"]
    dbl = not run.get("gemm_float", False)
    I3, z3 = POSE[:, :3], POSE[:, 3]
    if t.name == "frame":
        cam = CAM + (float(BF), float(MB))
        if impl == "orbo":
            return orbo.search_by_projection_frame(POSE, frame_tlw(run), cam, t.th, a["q_kps"], a["flags"], a["x3dw"], a["desc_q"],
                                                   a["kps"], a["desc"], a["u_right"], sf, W, H, run["mono"], True,
                                                   a["occupied"], dbl)
        return R.search_by_projection_frame(POSE, frame_tlw(run), cam, t.th, a["q_kps"], a["flags"], a["x3dw"], a["desc_q"],
                                            a["kps"], a["desc"], a["u_right"], sf, BOUNDS, run["mono"], True, a["occupied"],
                                            dbl, stats)
    if t.name == "keyframe":
        if impl == "orbo":
            return orbo.search_by_projection_keyframe(POSE, OW, CAM, t.th, run["orb_dist"], LSF, a["q_kps"], a["flags"],
                                                      a["x3dw"], a["mn"], a["mx"], a["desc_q"], a["kps"], a["desc"], sf, W, H,
                                                      True, a["occupied"], dbl)
        return R.search_by_projection_keyframe(POSE, OW, CAM, t.th, run["orb_dist"], LSF, a["q_kps"], a["flags"], a["x3dw"],
                                               a["mn"], a["mx"], a["desc_q"], a["kps"], a["desc"], sf, BOUNDS, True,
                                               a["occupied"], dbl, stats)
    if t.name == "mappoints":
        if impl == "orbo":
            return orbo.search_by_projection_mappoints(a["mps"], a["desc_q"], a["kps"], a["desc"], a["u_right"], sf, W, H,
                                                       run["th"], t.nnratio, a["occupied"])
        return R.search_by_projection_mappoints(a["mps"], a["desc_q"], a["kps"], a["desc"], a["u_right"], sf, BOUNDS,
                                                run["th"], t.nnratio, a["occupied"], stats)
    p = a.get("pts")
    if t.name == "sim3proj":
        args = (POSE, OW, CAM, t.th, run["ratio"], LSF, p["valid"].astype(np.uint8), p["pos"], p["normal"], p["min_distance"],
                p["max_distance"], a["desc_q"], a["kps"], a["desc"], sf)
        if impl == "orbo":
            return orbo.search_by_projection_sim3(*args, W, H, run["variant"], a["occupied"], dbl)
        return R.search_by_projection_sim3(*args, BOUNDS, run["variant"], a["occupied"], dbl, stats)
    if t.name in ("fuse", "fuse_sim3"):
        args = (p, a["desc_q"], a["kps"], a["desc"], a["u_right"], sf, isig2, I3, z3, OW, CAM + (float(BF),), t.th, LSF)
        if impl == "orbo":
            return orbo.fuse_search(*args, W, H, t.name == "fuse_sim3", dbl)
        return R.fuse_search(*args, BOUNDS, t.name == "fuse_sim3", dbl, stats)
    if t.name == "sim3dir":
        if impl == "orbo":
            return (_orbo_sim3_direction(p, a, sf, dbl, t.th),)
        return (R._sim3_direction(p["valid"], p["pos"], p["min_distance"], p["max_distance"], a["desc_q"], I3, z3, I3, z3, CAM,
                                  t.th, LSF, a["kps"], a["desc"], sf, BOUNDS, dbl, stats),)
    if t.name == "triangulation":
        args = (a["kps1"], a["desc_q"], a["mp1"], a["ur1"], a["fv1"], a["kps"], a["desc"], a["occupied"], a["u_right"], a["fv2"],
                sf, sig2, t.F12, t.ep, run["only_stereo"], run["coarse"], True)
        if impl == "orbo":
            return orbo.search_for_triangulation(*args)
        return R.search_for_triangulation(*args, stats)
    raise KeyError(t.name)


def _orbo_sim3_direction(p, a, sf, dbl, th):
    """one direction of SearchBySim3 from the oracle: KeyFrame 2 holds the table's keypoints, KeyFrame 1 has none of its
    own, so vnMatch1 is what search_by_sim3's agreement check would read"""
    import ctypes as C
    from oracle.orbo import _p, lib
    va = np.ascontiguousarray(p["valid"], np.uint8)
    xx = np.ascontiguousarray(p["pos"], np.float32)
    I3 = np.ascontiguousarray(POSE[:, :3]).reshape(9)
    z3 = np.ascontiguousarray(POSE[:, 3])
    f = [np.ascontiguousarray(v, np.float32) for v in (I3, z3, I3, z3, CAM, p["min_distance"], p["max_distance"], sf)]
    md = np.ascontiguousarray(a["desc_q"], np.uint8)
    kk = np.ascontiguousarray(a["kps"], orbo.KP_DTYPE)
    kd = np.ascontiguousarray(a["desc"], np.uint8)
    out = np.full(max(len(va), 1), -1, np.int32)
    lib().orbo_search_by_sim3_direction(_p(f[0]), _p(f[1]), _p(f[2]), _p(f[3]), _p(f[4]), float(th), float(LSF), W, H, int(dbl),
                                        len(va), _p(va), _p(xx), _p(f[5]), _p(f[6]), _p(md), _p(kk), len(kk), _p(kd), _p(f[7]),
                                        len(f[7]), _p(out))
    return out[:len(va)]


def per_row(t, result):
    """the raw result of `reference` / the device -> per row the matched keypoint index or -1"""
    n = len(t.rows)
    if t.name in ("fuse", "fuse_sim3"):
        return np.asarray(result[0], np.int32)
    if t.name == "sim3dir":
        return np.asarray(result[0], np.int32)
    if t.name == "triangulation":
        return np.asarray(result[-1], np.int32)
    m = np.asarray(result[1], np.int32)  # match[keypoint] = query
    out = np.full(n, -1, np.int32)
    for k, q in enumerate(m):
        if q >= 0:
            out[q] = k
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
