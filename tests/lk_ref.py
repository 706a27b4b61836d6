"""CPU restatement, in numpy float32, of the pyramidal inverse-compositional Lucas-Kanade tracker vilib::FeatureTrackerGPU
-- the yardstick of tests/test_gpu_featuretracker.py.  What it restates (thirdparty/vilib/visual_lib/src/feature_tracker):
  1. templates + inverse Hessians   feature_tracker_cuda_tools.cu:405-690 (load_ref_patch, calc_hessian, update_tracks_kernel)
  2. tracking                       feature_tracker_cuda_tools.cu:57-304  (perform_lk, track_features_kernel)
  3. bookkeeping                    feature_tracker_gpu.cpp:85-352,496-524, feature_tracker_base.cpp:61-171
Every numpy operation below is one operation per element, rounded on its own, in the order in which the reference's
source text reads; DESIGN.md section 8 lists what the reference leaves undefined and what is chosen:
  * no contraction: a*b + c is a rounded product and a rounded sum;  1.0f / det is IEEE division;  sqrtf is correctly rounded
  * a candidate is 32 lanes; lane t owns patch pixels i*32 + t (raster order) and adds them in ascending i; Jres is
    reduced by the xor butterfly 16, 8, 4, 2, 1, H by the shift-down tree with the same offsets (lane 0 is read)
  * int u = floorf(x) saturates; NaN is tested before; a NaN output is the word 0x7fffffff
  * best-N: score descending, then cell index ascending;  track ids count from 0 per tracker
`ft` is the float type: numpy.float32 is the yardstick, numpy.float64 the same recurrences for tests/test_lk_cpu.py.
tests/test_lk_cpu.py pins this file from outside (known shifts, real motion, float64 agreement, invH * H, lane order).
"""
import numpy as np

F = np.float32
MAX_ITER = 30  # FEATURE_TRACKER_MAX_ITERATION_COUNT (feature_tracker/config.h)
NAN_WORD = 0x7FFFFFFF
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LANES = 32


def nan_marker(ft=F):
    """__int_as_float(0x7fffffff)"""
    return np.array([NAN_WORD], np.uint32).view(np.float32)[0] if ft is F else ft(np.nan)


def halfsample(img):
    """image_halfsample_gpu_kernel (pyramid_gpu.cu:76-96); level sizes are original >> l."""
    h, w = img.shape[0] >> 1, img.shape[1] >> 1
    s = img[:2 * h, :2 * w].astype(np.uint32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) >> 2).astype(np.uint8)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(halfsample(out[-1]))
    return out


def sat_floor(x):
    """int u = floorf(x) for a non-NaN x, saturating as CUDA's and gfx950's float-to-int conversions do"""
    f = float(np.floor(x))
    if f >= 2147483648.0:
        return INT_MAX
    if f <= -2147483648.0:
        return INT_MIN
    return int(f)


# ------------------------------------------------------------------------------------------------ inverse Hessians
# The closed forms of feature_tracker_cuda_tools.cu:583-620 as tables: a term is [+|-][2*]<indices into H>, a product is
# taken left to right (a leading 2 first), the terms are summed left to right.
DET4 = ("0479 +2*0568 +1188 +2*1259 +2*1367 +2*2348 +2266 +3355 -0488 -0559 -0667 -1179 -2*1358 -2*1268 -2249 "
        "-2*2356 -3347")
INV4 = ("479 +2*568 -488 -559 -667", "188 +259 +367 -179 -268 -358", "159 +266 +348 -168 -249 -356",
        "167 +248 +355 -158 -265 -347", "079 +2*238 -088 -229 -337", "068 +129 +335 -059 -236 -138",
        "058 +226 +137 -067 -128 -235", "049 +2*136 -066 -119 -334", "056 +118 +234 -048 -126 -135",
        "047 +2*125 -055 -117 -224")
DET3 = "035 +2*142 -044 -232 -115"
INV3 = ("35 -44", "24 -15", "14 -23", "05 -22", "12 -04", "03 -11")
DET2 = "02 -11"


def terms(expr):
    """-> [(negative, doubled, indices)]"""
    out = []
    for t in expr.split():
        neg = t[0] == "-"
        t = t.lstrip("+-")
        two = t.startswith("2*")
        out.append((neg, two, tuple(int(c) for c in (t[2:] if two else t))))
    return out


def evaluate(expr, H, ft=F):
    acc = None
    for neg, two, idx in terms(expr):
        p = ft(2.0) * H[idx[0]] if two else H[idx[0]]
        for k in idx[1:]:
            p = p * H[k]
        acc = p if acc is None else (acc - p if neg else acc + p)
    return acc


def n_params(offset, gain):
    return 4 if (offset and gain) else 3 if (offset or gain) else 2


def invert(H, offset, gain, ft=F):
    """lane 0 of calc_hessian (:583-620): H (10) -> invH (10; the entries the form does not write stay as they are)"""
    out = np.zeros(10, ft)
    with np.errstate(all="ignore"):
        n = n_params(offset, gain)
        if n == 4:
            inv = ft(1.0) / evaluate(DET4, H, ft)
            for k in range(10):
                out[k] = evaluate(INV4[k], H, ft) * inv
        elif n == 3:
            inv = ft(1.0) / evaluate(DET3, H, ft)
            for k in range(6):
                out[k] = evaluate(INV3[k], H, ft) * inv
        else:
            inv = ft(1.0) / evaluate(DET2, H, ft)
            out[0] = H[2] * inv
            out[1] = ft(-1.0) * H[1] * inv
            out[2] = H[0] * inv
    return out, (10 if n == 4 else 6 if n == 3 else 3)


def full_matrix(v, n):
    """the symmetric n x n matrix of the upper-triangle vector v, in the reference's numbering"""
    M = np.zeros((n, n), np.float64)
    k = 0
    for r in range(n):
        for c in range(r, n):
            M[r, c] = M[c, r] = v[k]
            k += 1
    return M


# ------------------------------------------------------------------------------------------------ lanes
def lane_pixels(ps):
    """(rows, cols) of the patch pixels i*32 + t: arrays [area/32, 32]"""
    k = np.arange(ps * ps).reshape(ps * ps // LANES, LANES)
    return k // ps, k % ps


def reduce_xor(v, pairing="xor"):
    """Jres: v[t] + v[t ^ o], o = 16, 8, 4, 2, 1 (:142-148); every lane ends with the same word.  Two other orders, for
    the test that shows the order matters: 'ascending' is the butterfly with o = 1, 2, 4, 8, 16 (neighbours first, what
    a row-wise DPP reduction would do), 'serial' adds lanes 0 .. 31 one after the other."""
    t = np.arange(LANES)
    with np.errstate(all="ignore"):
        if pairing == "serial":
            acc = v[0]
            for k in range(1, LANES):
                acc = acc + v[k]
            return np.full_like(v, acc)
        for o in ((16, 8, 4, 2, 1) if pairing == "xor" else (1, 2, 4, 8, 16)):
            v = v + v[t ^ o]
    return v


def reduce_down(v):
    """H: v[t] + v[t + o] where t + o < 32, else the lane's own value (__shfl_down_sync); lane 0 is read (:575-581)"""
    for o in (16, 8, 4, 2, 1):
        v = v + np.concatenate([v[o:], v[LANES - o:]])
    return v[0]


def load_ref_patch(img, px, ps):
    """:405-465 with REFERENCE_PATCH_INTERPOLATION 0 -> the (ps+2)^2 int patch, or None where it does not fit"""
    h, w = img.shape
    half = ps >> 1
    ft = type(px[0])
    x_tl, y_tl = sat_floor(px[0] - ft(half + 1)), sat_floor(px[1] - ft(half + 1))
    if x_tl < 0 or y_tl < 0 or x_tl + ps + 1 >= w or y_tl + ps + 1 >= h:
        return None
    return img[y_tl:y_tl + ps + 2, x_tl:x_tl + ps + 2].astype(np.int32)


def hessian(patch, ps, offset, gain, ft=F):
    """calc_hessian's accumulation and reduction (:497-581): the 10 sums of lane 0"""
    rr, cc = lane_pixels(ps)
    c = patch[rr + 1, cc + 1].astype(ft)
    J = [ft(0.5) * (patch[rr + 1, cc + 2] - patch[rr + 1, cc]).astype(ft), ft(0.5) * (patch[rr + 2, cc + 1] - patch[rr, cc + 1]).astype(ft)]
    if offset and gain:
        J += [np.ones_like(c), c]
    elif offset:
        J += [np.ones_like(c)]
    elif gain:
        J += [c]
    H = np.zeros(10, ft)
    k = 0
    for a in range(len(J)):
        for b in range(a, len(J)):
            prod = J[a] * J[b]
            acc = np.zeros(LANES, ft)
            for i in range(prod.shape[0]):
                acc = acc + prod[i]
            H[k] = reduce_down(acc)
            k += 1
    return H


def precompute(pyr, px, opt, patch_out, invh_out, ft=F):
    """update_tracks_kernel for one candidate (:646-688): writes patch_out[L, max_area] and invh_out[L, 10], max_level first"""
    for li, level in enumerate(range(opt.klt_max_level, opt.klt_min_level - 1, -1)):
        inv_scale = ft(1.0) / ft(1 << level)
        ps = opt.klt_patch_sizes[level]
        p = load_ref_patch(pyr[level], (px[0] * inv_scale, px[1] * inv_scale), ps)
        if p is None:
            invh_out[li, 0] = nan_marker(ft)
            continue
        patch_out[li, :(ps + 2) * (ps + 2)] = p.ravel()
        inv, n = invert(hessian(p, ps, opt.affine_est_offset, opt.affine_est_gain, ft), opt.affine_est_offset, opt.affine_est_gain, ft)
        invh_out[li, :n] = inv[:n]


def lane_sums(img, ps, P, cur, uv, ab, offset, gain, ft=F):
    """One iteration's Jres before the reduction (:103-139): per entry of Jres the 32 lanes' sums over their pixels.
    P is the (ps+2) x (ps+2) template, (u, v) = floor(cur) has passed the bounds test."""
    half = ps >> 1
    rr, cc = lane_pixels(ps)
    ref = P[rr + 1, cc + 1].astype(ft)
    gx, gy = (P[rr + 1, cc + 2] - P[rr + 1, cc]).astype(ft), (P[rr + 2, cc + 1] - P[rr, cc + 1]).astype(ft)
    one, hf = ft(1.0), ft(0.5)
    (x, y), (u, v), (a, b) = cur, uv, ab
    with np.errstate(all="ignore"):
        sx, sy = x - ft(u), y - ft(v)
        wTL, wTR, wBL, wBR = (one - sx) * (one - sy), sx * (one - sy), (one - sx) * sy, sx * sy
        r0, c0 = rr + (v - half), cc + (u - half)
        s = ((wTL * img[r0, c0].astype(ft) + wTR * img[r0, c0 + 1].astype(ft)) + wBL * img[r0 + 1, c0].astype(ft)) + wBR * img[
            r0 + 1, c0 + 1].astype(ft)
        res = (s - (one + a) * ref) - b
        parts = [(res * hf) * gx, (res * hf) * gy]
        if offset and gain:
            parts += [res, res * ref]
        elif offset:
            parts += [res]
        elif gain:
            parts += [res * ref]
        out = []
        for p in parts:
            acc = np.zeros(LANES, ft)
            for i in range(p.shape[0]):
                acc = acc + p[i]
            out.append(acc)
    return out


def perform_lk(img, ps, patch, invH, cur, ab, opt, ft=F, pairing="xor", trace=None):
    """:57-187 -> (cur, ab, converged, go_to_next_level)"""
    h, w = img.shape
    half = ps >> 1
    offset, gain = opt.affine_est_offset, opt.affine_est_gain
    P = patch[:(ps + 2) * (ps + 2)].reshape(ps + 2, ps + 2)
    x, y = cur
    a, b = ab
    min_update = ft(opt.klt_min_update_squared)
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            if np.isnan(x) or np.isnan(y):
                return (x, y), (a, b), False, False
            u, v = sat_floor(x), sat_floor(y)
            if u < half or v < half or u >= w - half or v >= h - half:
                if trace is not None:
                    trace.append((u, v, it))
                return (x, y), (a, b), False, True
            J = [reduce_xor(acc, pairing)[0] for acc in lane_sums(img, ps, P, (x, y), (u, v), (a, b), offset, gain, ft)]
            if offset and gain:
                up = [((invH[0] * J[0] + invH[1] * J[1]) + invH[2] * J[2]) + invH[3] * J[3],
                      ((invH[1] * J[0] + invH[4] * J[1]) + invH[5] * J[2]) + invH[6] * J[3],
                      ((invH[2] * J[0] + invH[5] * J[1]) + invH[7] * J[2]) + invH[8] * J[3],
                      ((invH[3] * J[0] + invH[6] * J[1]) + invH[8] * J[2]) + invH[9] * J[3]]
            elif offset or gain:
                up = [(invH[0] * J[0] + invH[1] * J[1]) + invH[2] * J[2], (invH[1] * J[0] + invH[3] * J[1]) + invH[4] * J[2],
                      (invH[2] * J[0] + invH[4] * J[1]) + invH[5] * J[2]]
            else:
                up = [invH[0] * J[0] + invH[1] * J[1], invH[1] * J[0] + invH[2] * J[1]]
            x, y = x - up[0], y - up[1]
            if offset and gain:
                a, b = a + up[3], b + up[2]
            elif offset:
                b = b + up[2]
            elif gain:
                a = a + up[2]
            if up[0] * up[0] + up[1] * up[1] < min_update:
                return (x, y), (a, b), True, False
    return (x, y), (a, b), False, False


def track_one(pyr, patches, invh, cur, ab, first, opt, ft=F, pairing="xor", trace=None):
    """track_features_kernel for one candidate (:204-303) -> (converged, cur, ab, disparity)"""
    converged, go = False, True
    x, y = cur
    level, li = opt.klt_max_level, 0
    with np.errstate(all="ignore"):
        while (converged or go) and level >= opt.klt_min_level:
            scale = ft(1 << level)
            inv_scale = ft(1.0) / scale
            x, y = x * inv_scale, y * inv_scale
            if not np.isnan(invh[li, 0]):  # the reference's `continue` still runs the loop increment below
                (x, y), ab, converged, go = perform_lk(pyr[level], opt.klt_patch_sizes[level], patches[li], invh[li], (x, y), ab, opt,
                                                       ft, pairing, trace)
            x, y = x * scale, y * scale
            level -= 1
            li += 1
        if not converged:
            return False, (nan_marker(ft), nan_marker(ft)), ab, None
        dx, dy = x - first[0], y - first[1]
        return True, (x, y), ab, np.sqrt(dx * dx + dy * dy)


# ------------------------------------------------------------------------------------------------ bookkeeping
class Options:
    """vilib::FeatureTrackerOptions (feature_tracker_options.h:50-98) + Frame's n_pyr_levels"""

    def __init__(self, klt_min_level=0, klt_max_level=4, klt_patch_sizes=(16, 16, 16, 8, 8), klt_min_update_squared=0.0005,
                 min_tracks_to_detect_new_features=100, reset_before_detection=True, use_best_n_features=-1,
                 klt_template_is_first_observation=True, affine_est_offset=False, affine_est_gain=False, pyramid_levels=5):
        self.klt_min_level, self.klt_max_level = klt_min_level, klt_max_level
        self.klt_patch_sizes = tuple(klt_patch_sizes)
        self.klt_min_update_squared = klt_min_update_squared
        self.min_tracks_to_detect_new_features = min_tracks_to_detect_new_features
        self.reset_before_detection = reset_before_detection
        self.use_best_n_features = use_best_n_features
        self.klt_template_is_first_observation = klt_template_is_first_observation
        self.affine_est_offset, self.affine_est_gain = affine_est_offset, affine_est_gain
        self.pyramid_levels = pyramid_levels


def max_ftr_count(opt, cells):
    """feature_tracker_gpu.cpp:404-411"""
    return (opt.min_tracks_to_detect_new_features - 1) + ((cells if opt.use_best_n_features == -1 else opt.use_best_n_features) - 1)


class Track:
    def __init__(self, x, y, level, score, track_id, buffer_id):
        self.first_pos, self.first_level, self.first_score = (x, y), level, score
        self.cur_pos, self.cur_disparity = (x, y), F(0.0)
        self.track_id, self.buffer_id, self.life = track_id, buffer_id, 0


class Book:
    """Steps 02 and 03 of FeatureTrackerGPU::track and what they call: the track list, the buffer-id LIFO, the frame's
    feature list, the occupancy grid, best-N selection, getDisparity.  No pixels are touched here."""

    def __init__(self, opt, n_cols, n_rows, cell_w, cell_h):
        self.opt, self.n_cols, self.n_rows, self.cw, self.ch = opt, n_cols, n_rows, cell_w, cell_h
        self.cells = n_cols * n_rows
        self.max_ftr = max_ftr_count(opt, self.cells)
        self.avail = [self.max_ftr - i - 1 for i in range(self.max_ftr)]  # initBufferIds: decreasing, popped from the back
        self.tracks, self.features, self.next_id = [], [], 0
        self.tracked = self.detected = 0

    def add_feature(self, t):
        self.features.append((t.cur_pos[0], t.cur_pos[1], t.first_score, t.first_level, t.track_id))

    def results(self, res):
        """step 02 (:137-186).  res[i] = (x, y, disparity) of track i; a NaN x ends the track."""
        self.features, self.tracked = [], 0
        keep = []
        for t, (x, y, d) in zip(self.tracks, res):
            if np.isnan(x):
                self.avail.append(t.buffer_id)
                continue
            t.life += 1
            t.cur_pos, t.cur_disparity = (x, y), d
            self.tracked += 1
            self.add_feature(t)
            keep.append(t)
        self.tracks = keep

    def need_detect(self):
        return self.tracked < self.opt.min_tracks_to_detect_new_features

    def detect(self, pos, score, level):
        """step 03 (:188-267) on a detector grid -> the new tracks.  Positions outside the grid mark no cell; no buffer
        id left ends the loop (the reference asserts in both cases)."""
        self.detected = 0
        occ = np.zeros(self.cells, bool)
        if self.opt.reset_before_detection:
            self.tracked = 0
            for t in self.tracks:
                self.avail.append(t.buffer_id)
            self.tracks, self.features = [], []
        else:
            for f in self.features:
                x, y = int(f[0]), int(f[1])  # Eigen::Vector2d -> int: truncation
                if 0 <= x < self.n_cols * self.cw and 0 <= y < self.n_rows * self.ch:
                    occ[(y // self.ch) * self.n_cols + x // self.cw] = True
        if self.opt.use_best_n_features == -1:
            order, limit = range(self.cells), self.cells
        else:
            order = sorted(range(self.cells), key=lambda i: (-float(score[i]), i))
            limit = max(0, self.opt.use_best_n_features - self.tracked)
        new = []
        for c in order:
            if self.detected >= limit or not self.avail:
                break
            if not occ[c] and score[c] > 0.0:
                t = Track(F(pos[c][0]), F(pos[c][1]), int(level[c]), F(score[c]), self.next_id, self.avail.pop())
                self.next_id += 1
                self.tracks.append(t)
                self.add_feature(t)
                new.append(t)
                self.detected += 1
        return new

    def update_count(self):
        """step 04 (:272-279): the last n tracks get templates"""
        return self.detected if self.opt.klt_template_is_first_observation else self.detected + self.tracked

    def reset(self):
        for t in self.tracks:
            self.avail.append(t.buffer_id)
        self.tracks, self.tracked, self.detected = [], 0, 0

    def disparity(self, pivot_ratio):
        """FeatureTrackerBase::getDisparity (feature_tracker_base.cpp:137-171) for one camera"""
        d = []
        for t in self.tracks:
            if t.life <= 0:
                break
            d.append(t.cur_disparity)
        if not d:
            return 0.0
        return float(sorted(d)[int(pivot_ratio * len(d))])


class Tracker:
    """FeatureTrackerGPU for one camera.  detect(image) -> (pos[cells, 2], score[cells], level[cells]) is the bound
    detector's raw grid (the callback overload: no threshold step)."""

    def __init__(self, opt, detect, n_cols, n_rows, cell_w=32, cell_h=32, ft=F, pairing="xor"):
        self.opt, self.detect, self.ft, self.pairing = opt, detect, ft, pairing
        self.book = Book(opt, n_cols, n_rows, cell_w, cell_h)
        n, L = self.book.max_ftr, opt.klt_max_level - opt.klt_min_level + 1
        self.max_area = (max(opt.klt_patch_sizes) + 2) ** 2
        self.patches = np.zeros((n, L, self.max_area), np.int32)
        self.invh = np.zeros((n, L, 10), ft)
        self.template_px, self.first_px, self.cur_px = [None] * n, [None] * n, [None] * n
        self.ab = [None] * n
        self.trace = []      # (u, v, iteration) of every position that failed a level's bounds test
        self.redetected = 0  # detections that ran with at least one occupied cell

    def track(self, img):
        ft, B, opt = self.ft, self.book, self.opt
        pyr = pyramid(img, opt.pyramid_levels)
        res = []
        for t in B.tracks:
            b = t.buffer_id
            ok, cur, ab, d = track_one(pyr, self.patches[b], self.invh[b], self.cur_px[b], self.ab[b], self.first_px[b], opt, ft,
                                       self.pairing, self.trace)
            self.cur_px[b] = cur
            if ok:
                a0, b0 = self.ab[b]
                self.ab[b] = (ab[0] if opt.affine_est_gain else a0, ab[1] if opt.affine_est_offset else b0)
            res.append((cur[0], cur[1], d))
        B.results(res)
        if not opt.klt_template_is_first_observation:
            for t in B.tracks:
                self.template_px[t.buffer_id] = t.cur_pos
        if B.need_detect():
            if B.tracks and not opt.reset_before_detection:
                self.redetected += 1
            for t in B.detect(*self.detect(img)):
                p = (ft(t.first_pos[0]), ft(t.first_pos[1]))
                b = t.buffer_id
                self.template_px[b] = self.first_px[b] = self.cur_px[b] = p
                self.ab[b] = (ft(0.0), ft(0.0))
        else:
            B.detected = 0
        n = B.update_count()
        for t in B.tracks[len(B.tracks) - n:]:
            precompute(pyr, self.template_px[t.buffer_id], opt, self.patches[t.buffer_id], self.invh[t.buffer_id], ft)
        return B.tracked, B.detected

    # ---- what the tests compare, as arrays
    def track_table(self):
        T = self.book.tracks
        return dict(first_pos=np.array([t.first_pos for t in T], F).reshape(-1, 2), cur_pos=np.array([t.cur_pos for t in T], F).reshape(-1, 2),
                    cur_disparity=np.array([t.cur_disparity for t in T], F), life=np.array([t.life for t in T], np.int32),
                    track_id=np.array([t.track_id for t in T], np.int32), buffer_id=np.array([t.buffer_id for t in T], np.int32))

    def feature_table(self):
        f = self.book.features
        return dict(px=np.array([(a[0], a[1]) for a in f], F).reshape(-1, 2), score=np.array([a[2] for a in f], F),
                    level=np.array([a[3] for a in f], np.int32), track_id=np.array([a[4] for a in f], np.int32))
