"""Synthetic inputs for the Lucas-Kanade tracker's edges, shared by tests/test_lk_edge_cases_cpu.py (what each case reaches
on the yardstick tests/lk_ref.py), tests/test_gpu_featuretracker_edges.py (device against yardstick, word for word) and
tests/tools/lk_exit_census.py (profiles/lk_exit_census.txt).  The hut_long cases of tests/lk_cases.py never see a singular
Hessian, an inf or NaN inverse, a NaN position, an exit through the top edge, iteration exhaustion at patch 8, a level range
other than 0..4 or a threshold other than the default; these frames do.  Every frame comes from seeded numpy alone.

A case is a dict: det (detector kind), border (the detector's), opts (tracker options), frames (a callable -> list of at most
five images).  Shapes are (h, w): LAND 176x192 (the smallest comfortable size for five levels with the default patches: level
4 is 11x12), PORT 208x176 (portrait; 5.5 cell columns) and WIDE 160x208 (6.5 cell columns: 208 is a multiple of 16 and not
of 32, so every level's pitch differs from the hut crops' and the cell grid has a partial column).

`Census` instruments the yardstick from outside -- it wraps lk_ref.invert, load_ref_patch, perform_lk and lane_sums and
leaves their arithmetic alone -- and counts what a run reaches."""
import collections
import functools

import numpy as np

import lk_bundle_ref as lb
import lk_cases as LC
import lk_ref as lk

LAND, PORT, WIDE = (176, 192), (208, 176), (160, 208)
F = np.float32
# every cell that has a corner gets a track, and detection runs once: the tracks of frame 0 are followed to the end
OPTS = dict(reset_before_detection=False, use_best_n_features=-1, min_tracks_to_detect_new_features=2)
AFFINE = [(False, False), (True, False), (False, True), (True, True)]


# ---------------------------------------------------------------------------------------------------------------- frames
def dot_centres(shape, seed, jitter=5):
    """one dot per full 32x32 cell, around the cell's middle"""
    h, w = shape
    rng = np.random.default_rng(seed)
    out = []
    for cy in range(16, h - 12, 32):
        for cx in range(16, w - 12, 32):
            jx, jy = rng.integers(-jitter, jitter + 1, 2)
            out.append((cx + jx, cy + jy))
    return out


def put_dots(img, centres, value):
    for x, y in centres:
        img[y - 1:y + 2, x - 1:x + 2] = value
    return img


def dots_scene(shape, seed, field=100, dot=115, step=None, moves=((0, 0), (1, 0), (1, 1)), size=3):
    """Faint dots on a flat field; the dots (not the step) move by `moves`.  step = "h": everything below the middle
    row y0 is 60 brighter, full width, and the dot rows next to it lie 6 px above and below y0; "v": the same with columns.
    A bright 3x3 dot of +15 is gone two or three levels up (the half-sampler truncates: (3 * 100 + 115) >> 2 = 103,
    (3 * 100 + 103) >> 2 = 100), a straight step is a FAST corner on no level.  One step, not one per cell row: a pattern
    with a period of two coarse pixels has no central difference at all.  size = 1: single pixels, gone on level 2 for certain."""
    h, w = shape
    y0, x0 = 32 * (h // 64) + 32, 32 * (w // 64) + 32  # a cell boundary near the middle: inside the window of level 4's patch
    c = dot_centres(shape, seed)
    base = np.full(shape, field, np.uint8)
    if step == "h":
        base[y0:] = field + 60
        c = [(x, y0 - 6 if y0 - 32 <= y < y0 else y0 + 6 if y0 <= y < y0 + 32 else y) for x, y in c]
    if step == "v":
        base[:, x0:] = field + 60
        c = [(x0 - 6 if x0 - 32 <= x < x0 else x0 + 6 if x0 <= x < x0 + 32 else x, y) for x, y in c]
    out = []
    for m in moves:
        img = base.copy()
        for cx, cy in c:
            x, y = cx + m[0], cy + m[1]
            r = size // 2
            img[y - r:y + r + 1, x - r:x + r + 1] += np.uint8(dot - field)
        out.append(img)
    return out


def texture(shape, seed, block=6, box=5):
    """smooth block noise: random grey levels on a `block` grid, box-filtered with cumulative sums"""
    h, w = shape
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((h + box) // block + 2, (w + box) // block + 2))
    big = np.kron(g, np.ones((block, block), np.int64))[:h + box, :w + box]
    s = np.zeros((h + box + 1, w + box + 1), np.int64)
    s[1:, 1:] = big.cumsum(0).cumsum(1)
    out = s[box:box + h, box:box + w] - s[:h, box:box + w] - s[box:box + h, :w] + s[:h, :w]
    return (out // (box * box)).astype(np.uint8)


def drift(shape, seed, step, n=5, margin=24):
    """n windows of one texture; the content moves by `step` = (dx, dy) px per frame"""
    h, w = shape
    big = texture((h + 2 * margin, w + 2 * margin), seed)
    out = []
    for k in range(n):
        x0, y0 = margin - k * step[0], margin - k * step[1]
        assert 0 <= x0 <= 2 * margin and 0 <= y0 <= 2 * margin
        out.append(np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w]))
    return out


def faded(img, contrast):
    """128 + contrast * (pixel - 128), rounded to nearest"""
    return np.floor(128.5 + contrast * (img.astype(np.float64) - 128)).astype(np.uint8)


def fit_scene(shape, ps_levels):
    """Dots at the positions where load_ref_patch's four tests flip: for every level l with patch size ps, the top-left
    corner floor(x / 2^l) - ps/2 - 1 is 0 (last fit) or -1 (first miss), or the far corner + ps + 1 is w-1 (last fit) or
    w (first miss) -- in x at a y that fits on that level, and in y at an x that fits.  Every dot has a cell of the
    detector's grid to itself; a class for which no cell is left is skipped (the three fit cases rotate the patch sizes over
    the levels, and tests/test_lk_edge_cases_cpu.py wants every class of every patch size from them together).  Two identical
    frames."""
    h, w = shape
    img = np.full(shape, 100, np.uint8)
    used, c = set(), []

    def place(axis, v, l, ps):
        s, hf = 1 << l, ps // 2
        size = (h, w)[axis] >> l  # of the other axis
        for r in range((h, w)[axis] // 32 + 1):
            for off in (16, 9, 23):
                o = 32 * r + off
                x, y = (v, o) if axis == 0 else (o, v)
                cell = (x // 32, y // 32)
                if cell in used or not (3 <= x < w - 3 and 3 <= y < h - 3) or not (0 <= o // s - hf - 1 and o // s + hf < size):
                    continue
                used.add(cell)
                c.append((x, y))
                return
        # no free cell that fits (patch 32 on level 2 of these sizes leaves two cells): another fit case has this class

    for l, ps in ps_levels:
        s, hf = 1 << l, ps // 2
        for axis, size in ((0, w >> l), (1, h >> l)):
            for v in (s * (hf + 1), s * (hf + 1) - 1, s * (size - hf - 1), s * (size - hf)):
                place(axis, v, l, ps)
    put_dots(img, c, 140)
    return [img, img.copy()]


# ----------------------------------------------------------------------------------------------------------------- cases
def _case(frames, det="fast", border=LC.BORDER, **opts):
    return dict(det=det, border=border, opts=dict(OPTS, **opts), frames=frames)


@functools.lru_cache(None)
def cases():
    c = {"flat_coarse": _case(lambda: dots_scene(LAND, 1))}
    for off, gain in AFFINE:
        tag = "%d%d" % (off, gain)
        c["edge_h_" + tag] = _case(lambda: dots_scene(LAND, 2, step="h", moves=((0, 0), (1, 0))), affine_est_offset=off, affine_est_gain=gain)
        c["edge_v_" + tag] = _case(lambda: dots_scene(PORT, 3, step="v", moves=((0, 0), (0, 1))), affine_est_offset=off, affine_est_gain=gain)
    # A 255 field with darker dots never becomes constant under the truncating half-sampler (a dark pixel lowers its parent by
    # at least one grey level on every level), so the over-exposed scene is the other way round: single pixels clipped at 255
    # on a 243 field, (3 * 243 + 255) >> 2 = 246, (3 * 243 + 246) >> 2 = 243: levels 2 and up are exactly constant, and with
    # the gain column H = (0, 0, 0, 0, 0, sum v^2).
    c["saturated"] = _case(lambda: dots_scene(WIDE, 4, field=243, dot=255, size=1), affine_est_gain=True)
    c["saturated_11"] = _case(lambda: dots_scene(WIDE, 4, field=243, dot=255, moves=((0, 0), (1, 1)), size=1), affine_est_offset=True,
                              affine_est_gain=True)
    c["drift_left"] = _case(lambda: drift(LAND, 5, (-2, -1)), border=4)
    c["drift_right"] = _case(lambda: drift(WIDE, 6, (3, 1)), border=4)
    c["drift_top"] = _case(lambda: drift(PORT, 7, (1, -2)), border=4)
    c["drift_bottom"] = _case(lambda: drift(LAND, 8, (-1, 3)), border=4)
    c["drift_patch32"] = _case(lambda: drift(WIDE, 9, (-2, -2), n=4), border=4, klt_patch_sizes=(32, 32, 16, 8, 8))
    c["fit_8_16_32"] = _case(lambda: fit_scene(LAND, ((0, 8), (1, 16), (2, 32))), border=3, klt_patch_sizes=(8, 16, 32, 8, 8))
    c["fit_32_8_16"] = _case(lambda: fit_scene(PORT, ((0, 32), (1, 8), (2, 16))), border=3, klt_patch_sizes=(32, 8, 16, 8, 8))
    c["fit_16_32_8"] = _case(lambda: fit_scene(WIDE, ((0, 16), (1, 32), (2, 8))), border=3, klt_patch_sizes=(16, 32, 8, 8, 8))
    # identical frames: the update is exactly 0 and 0 < 0 is false, so the first level that has a template runs 30 iterations
    # and the track dies there; with levels 0..1 that level has patch size 32
    c["static_zero_threshold"] = _case(lambda: [texture(LAND, 10)] * 2, border=4, klt_min_update_squared=0.0)
    c["static_zero_threshold_32"] = _case(lambda: [texture(WIDE, 10)] * 2, border=4, klt_min_update_squared=0.0, klt_max_level=1,
                                          klt_patch_sizes=(32, 32, 16, 8, 8))
    # a frame of 0.12 of the template's contrast: without gain estimation every update is about 0.12 of what is missing, so
    # levels need 20 to 40 iterations: some converge in the last of the 30, some run out of them on a regular Hessian
    c["faded"] = _case(lambda: [f if k != 1 else faded(f, 0.12) for k, f in enumerate(drift(LAND, 21, (1, 1), n=3))])
    # every live track's template is renewed in every frame, and the disparity is measured from the first position
    c["drift_last_template"] = _case(lambda: drift(PORT, 15, (1, 1), n=4), klt_template_is_first_observation=False)
    for off in (False, True):  # gain estimation on a last frame of pixels * 0.8 + 10: alpha ends near -0.2
        c["gain_dimmed_%d1" % off] = _case(lambda: [f if k != 2 else LC.dimmed(f) for k, f in enumerate(drift(WIDE, 16, (1, 0), n=3))],
                                           affine_est_offset=off, affine_est_gain=True)
    c["inf_threshold"] = _case(lambda: drift(PORT, 11, (1, 1), n=3), klt_min_update_squared=float("inf"))
    c["levels_1_3"] = _case(lambda: drift(LAND, 12, (1, -1), n=3), klt_min_level=1, klt_max_level=3, klt_patch_sizes=(8, 8, 32, 16, 8))
    c["levels_0_1"] = _case(lambda: drift(WIDE, 13, (-1, 1), n=3), klt_min_level=0, klt_max_level=1, klt_patch_sizes=(8, 32, 16, 8, 8),
                            pyramid_levels=3)
    # more pyramid levels than the tracker uses, and a larger patch size on the unused levels than on the used ones
    c["levels_0_2_deep"] = _case(lambda: drift(PORT, 14, (1, 2), n=3), klt_min_level=0, klt_max_level=2, klt_patch_sizes=(16, 8, 8, 32, 32),
                                 pyramid_levels=5)
    return c


DEGENERATE = ("flat_coarse", "saturated", "saturated_11") + tuple("edge_%s_%d%d" % (s, o, g) for s in "hv" for o, g in AFFINE)
LEVELS = ("levels_1_3", "levels_0_1", "levels_0_2_deep")
FIT = ("fit_8_16_32", "fit_32_8_16", "fit_16_32_8")
# camera 0 leaves through the bottom: the row below its last row is camera 1's first row on every level of the pyramid
BUNDLE = dict(det="fast", border=4, opts=dict(OPTS), cameras=("drift_bottom", "edge_h_00", "drift_left"), n_calls=3)


@functools.lru_cache(None)
def frames(name):
    return cases()[name]["frames"]()


@functools.lru_cache(None)
def run_ref(name):
    """-> (the lk_ref.Tracker after the last frame, last summary, per-frame summaries)"""
    c = cases()[name]
    return LC.run_case(c["det"], c["opts"], frames(name), c["border"])


def bundle_images():
    """[call][camera] -> image"""
    return [[frames(n)[min(k, len(frames(n)) - 1)] for n in BUNDLE["cameras"]] for k in range(BUNDLE["n_calls"])]  # a short case holds its last frame


def bundle_uncached():
    """the bundle as lone yardstick trackers with one id counter (tests/lk_bundle_ref.py)
    -> (the BundleTracker, per call the per-camera summaries, per call [(tracked, detected)])"""
    seq = bundle_images()
    nc, nr = LC.grid(seq[0][0])
    B = lb.BundleTracker(lk.Options(**BUNDLE["opts"]), LC.ref_detector(BUNDLE["det"], BUNDLE["border"]), len(seq[0]), nc, nr, LC.CELL, LC.CELL)
    counts, per_call = [], []
    for imgs in seq:
        counts.append(B.track(imgs))
        per_call.append([LC.summary(T, [c[i] for c in counts]) for i, T in enumerate(B.T)])
    return B, per_call, counts


run_bundle_ref = functools.lru_cache(None)(bundle_uncached)


# ---------------------------------------------------------------------------------------------------------------- census
def inverse_class(inv, n):
    """finite | inf0 (invH[0] is an infinity) | nan0 (invH[0] is an arithmetic NaN) | nan_rest (a NaN or inf elsewhere)"""
    if np.isnan(inv[0]):
        return "nan0"
    if np.isinf(inv[0]):
        return "inf0"
    return "finite" if np.isfinite(inv[:n]).all() else "nan_rest"


class Census:
    """with Census() as c: ...run the yardstick...; c.n is a Counter of what was reached"""
    NAMES = ("invert", "load_ref_patch", "perform_lk", "lane_sums")

    def __enter__(self):
        self.n = collections.Counter()
        self.saved = {k: getattr(lk, k) for k in self.NAMES}
        self.iters = 0
        n, saved = self.n, self.saved

        def invert(H, offset, gain, ft=F):
            out, cnt = saved["invert"](H, offset, gain, ft)
            with np.errstate(all="ignore"):
                det = lk.evaluate({10: lk.DET4, 6: lk.DET3, 3: lk.DET2}[cnt], H, ft)
            n["inverse"] += 1
            n["inverse %s, %d parameters" % (inverse_class(out, cnt), lk.n_params(offset, gain))] += 1
            if det == 0:
                n["inverse singular (1/det = inf)"] += 1
            return out, cnt

        def load_ref_patch(img, px, ps):
            p = saved["load_ref_patch"](img, px, ps)
            h, w = img.shape
            ft, half = type(px[0]), ps >> 1
            tl = (lk.sat_floor(px[0] - ft(half + 1)), lk.sat_floor(px[1] - ft(half + 1)))
            fits = [0 <= t and t + ps + 1 < d for t, d in zip(tl, (w, h))]
            for ax, t, d, other in (("x", tl[0], w, fits[1]), ("y", tl[1], h, fits[0])):
                if not other:
                    continue  # the other axis already refuses: this one decides nothing
                for what, hit in (("last fit %s_tl == 0", t == 0), ("first miss %s_tl == -1", t == -1),
                                  ("last fit %s_tl + ps + 1 == size - 1", t + ps + 1 == d - 1), ("first miss %s_tl + ps + 1 == size", t + ps + 1 == d)):
                    if hit:
                        n["patch %d: %s" % (ps, what % ax)] += 1
            n["patch %d: %s" % (ps, "fits" if p is not None else "does not fit")] += 1
            return p

        def lane_sums(*a, **k):
            self.iters += 1
            return saved["lane_sums"](*a, **k)

        def perform_lk(img, ps, patch, invH, cur, ab, opt, ft=F, pairing="xor", trace=None):
            h, w = img.shape
            half = ps >> 1
            mine, self.iters = [], 0
            cur1, ab1, conv, go = saved["perform_lk"](img, ps, patch, invH, cur, ab, opt, ft, pairing, mine)
            if trace is not None:
                trace.extend(mine)
            nh = {4: 10, 3: 6, 2: 3}[lk.n_params(opt.affine_est_offset, opt.affine_est_gain)]
            n["level runs, patch %d" % ps] += 1
            if not np.isfinite(invH[:nh]).all():
                n["inf or NaN inverse used while tracking"] += 1
            if conv:
                n["converged, patch %d" % ps] += 1
                if self.iters == 1:
                    n["converged at iteration one"] += 1
                if self.iters == lk.MAX_ITER:
                    n["converged at the last iteration"] += 1
                u, v = lk.sat_floor(cur[0]), lk.sat_floor(cur[1])
                for what, hit in (("u == half", u == half), ("u == w-half-1", u == w - half - 1), ("v == half", v == half),
                                  ("v == h-half-1", v == h - half - 1)):
                    if hit:
                        n["started at %s and converged" % what] += 1
            elif go:
                (u, v, it), = mine
                kinds = [what for what, hit in (("left edge (u == half-1)", u == half - 1), ("right edge (u == w-half)", u == w - half),
                                                ("top edge (v == half-1)", v == half - 1), ("bottom edge (v == h-half)", v == h - half)) if hit]
                for k in kinds or ["further out"]:
                    n["leave-the-level exit, %s" % k] += 1
                    n["leave-the-level exit, %s, patch %d" % (k, ps)] += 1
                if u in (lk.INT_MIN, lk.INT_MAX) or v in (lk.INT_MIN, lk.INT_MAX):
                    n["ft_floor_int saturation behind an inf position"] += 1
            elif self.iters == lk.MAX_ITER and not (np.isnan(cur1[0]) or np.isnan(cur1[1])):
                n["iteration exhaustion, patch %d" % ps] += 1
            else:
                n["isnan(x) exit of the iteration loop"] += 1
            return cur1, ab1, conv, go

        for k, f in (("invert", invert), ("load_ref_patch", load_ref_patch), ("lane_sums", lane_sums), ("perform_lk", perform_lk)):
            setattr(lk, k, f)
        return self

    def __exit__(self, *exc):
        for k, f in self.saved.items():
            setattr(lk, k, f)
        return False


def census(name):
    """the case once more through the instrumented yardstick (not cached: run_ref's tracker stays as it is)"""
    c = cases()[name]
    with Census() as cen:
        T, last, _ = LC.run_case(c["det"], c["opts"], frames(name), c["border"])
    return cen.n, T, last
