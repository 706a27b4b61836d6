"""CPU reference for the distorted-pinhole tests: numpy restatements of

  * cv::undistortPoints(src, dst, K, D, noArray(), K) of OpenCV 4.2 (cvUndistortPointsInternal, TermCriteria(MAX_ITER,
    5, 0.01): five iterations, no EPS test, FP64 in OpenCV's literal order) as Frame::UndistortKeyPoints applies it
    (frame.cpp:758-790: k1 == 0 -> unchanged) and Frame::ComputeImageBounds (frame.cpp:793-821);
  * FMatcher::SearchForInitialization (fmatcher.cpp:983-1098) over a Frame grid with float bounds
    (frame.cpp:322-323, 678-756).

numpy float64 / float32 element-wise operations are IEEE operations without contraction, so these are bit-exact
references for the device and host builds of vi_slam_amd/csrc/vslam_undistort.h.
"""
import math

import numpy as np

# radtan (pinhole) calibrations: fx, fy, cx, cy | k1, k2, p1, p2[, k3]
ZED_CAM0 = ((669.2387507702717, 669.6062139634853, 647.4136147885813, 348.40757297218505),
            (0.0018645604002542789, -0.009206711115906055, -0.001490842343490958, 0.0047045781898403))
ZED_CAM1 = ((669.7077049723667, 669.7830132578491, 648.2500643003343, 348.45508924255745),
            (-0.0011120079644645446, -0.006192062533471337, -0.0011416874899672696, 0.004836945809987094))
# EuRoC MAV cam0 strength (k1 = -0.28) with intrinsics for a 1280 x 720 image
EUROC_LIKE = ((700.0, 699.5, 641.3, 361.7), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05))
WITH_K3 = ((690.0, 689.0, 635.5, 355.25), (-0.21, 0.035, 0.0004, -0.0007, 0.012))
NEG_ICDIST = ((650.0, 650.0, 640.0, 360.0), (-2.0, 0.0, 0.001, 0.001))  # 1 + k1*r2 < 0 for r2 > 0.5
K1_ZERO = ((669.0, 669.0, 647.0, 348.0), (0.0, -0.01, 0.002, 0.003))      # k1 == 0: the reference does nothing
CAMERAS = {"zed0": ZED_CAM0, "zed1": ZED_CAM1, "euroc": EUROC_LIKE, "k3": WITH_K3, "neg_icdist": NEG_ICDIST,
           "k1_zero": K1_ZERO}


def _f32(v):
    return np.asarray(v, np.float32)


def undistort_points(pts, K, D):
    """cv::undistortPoints with P = K (CV_32F K and D, CV_32FC2 points) -> float32 [n, 2].  No k1 test."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    k = np.zeros(14)
    for i, v in enumerate(D):
        k[i] = float(np.float32(v))
    ifx, ify = 1. / fx, 1. / fy
    u = pts[:, 0].astype(np.float64)
    v = pts[:, 1].astype(np.float64)
    x = (u - cx) * ifx
    y = (v - cy) * ify
    x0, y0 = x.copy(), y.copy()
    live = np.ones(len(x), bool)
    with np.errstate(all="ignore"):
        x, y = _iterate(x, y, x0, y0, u, v, cx, cy, ifx, ify, k, live)
    xx = fx * x + 0. * y + cx
    yy = 0. * x + fy * y + cy
    ww = 1. / (0. * x + 0. * y + 1.)
    return np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], 1)


def _iterate(x, y, x0, y0, u, v, cx, cy, ifx, ify, k, live):
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        stop = live & (icdist < 0)  # OpenCV issue 14583: restart from the normalised input and leave the loop
        x = np.where(stop, (u - cx) * ifx, x)
        y = np.where(stop, (v - cy) * ify, y)
        live &= ~stop
        deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = np.where(live, (x0 - deltaX) * icdist, x)
        y = np.where(live, (y0 - deltaY) * icdist, y)
    return x, y


def frame_undistort(pts, K, D):
    """Frame::UndistortKeyPoints' arithmetic: only k1 decides (frame.cpp:762)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if np.float32(D[0]) == 0:
        return pts.copy()
    return undistort_points(pts, K, D)


def undistort_keypoints(kps, K, D):
    out = kps.copy()
    u = frame_undistort(np.stack([kps["x"], kps["y"]], 1), K, D)
    out["x"], out["y"] = u[:, 0], u[:, 1]
    return out


def image_bounds(K, D, cols, rows):
    """Frame::ComputeImageBounds -> float32 (minX, maxX, minY, maxY)"""
    if np.float32(D[0]) == 0:
        return _f32([0, cols, 0, rows])
    c = undistort_points([(0, 0), (cols, 0), (0, rows), (cols, rows)], K, D)
    mn = lambda a, b: b if b < a else a  # std::min
    mx = lambda a, b: b if a < b else a  # std::max
    return _f32([mn(c[0, 0], c[2, 0]), mx(c[1, 0], c[3, 0]), mn(c[0, 1], c[1, 1]), mx(c[2, 1], c[3, 1])])


def distort_points(pts, K, D):
    """the radtan forward model (for the round-trip property only)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = K
    d = list(D) + [0.0] * (5 - len(D))
    k1, k2, p1, p2, k3 = d
    x = (pts[:, 0] - cx) / fx
    y = (pts[:, 1] - cy) / fy
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], 1)


# ---------------------------------------------------------------- Frame grid + SearchForInitialization
COLS, ROWS = 64, 48  # FRAME_GRID_COLS / ROWS, frame.h:42-43


def _round_half_away(v):
    """std::round(float): half away from zero (exact in double for float inputs)"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


class Grid:
    """Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea with float bounds, all float arithmetic in float32"""

    def __init__(self, kps, bounds):
        self.kps = kps
        self.minX, self.maxX, self.minY, self.maxY = (np.float32(b) for b in bounds)
        self.invW = np.float32(COLS) / np.float32(self.maxX - self.minX)
        self.invH = np.float32(ROWS) / np.float32(self.maxY - self.minY)
        self.cells = {}
        for i in range(len(kps)):
            px = _round_half_away(np.float32(np.float32(kps["x"][i]) - self.minX) * self.invW)
            py = _round_half_away(np.float32(np.float32(kps["y"][i]) - self.minY) * self.invH)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.cells.setdefault((px, py), []).append(i)

    def query(self, x, y, r, min_level, max_level):
        x, y, r = np.float32(x), np.float32(y), np.float32(r)
        out = []
        nMinCellX = max(0, math.floor(np.float32(np.float32(x - self.minX) - r) * self.invW))
        if nMinCellX >= COLS:
            return out
        nMaxCellX = min(COLS - 1, math.ceil(np.float32(np.float32(x - self.minX) + r) * self.invW))
        if nMaxCellX < 0:
            return out
        nMinCellY = max(0, math.floor(np.float32(np.float32(y - self.minY) - r) * self.invH))
        if nMinCellY >= ROWS:
            return out
        nMaxCellY = min(ROWS - 1, math.ceil(np.float32(np.float32(y - self.minY) + r) * self.invH))
        if nMaxCellY < 0:
            return out
        check = min_level > 0 or max_level >= 0
        for ix in range(nMinCellX, nMaxCellX + 1):
            for iy in range(nMinCellY, nMaxCellY + 1):
                for i in self.cells.get((ix, iy), ()):
                    o = int(self.kps["octave"][i])
                    if check and (o < min_level or (max_level >= 0 and o > max_level)):
                        continue
                    if abs(np.float32(self.kps["x"][i] - x)) < r and abs(np.float32(self.kps["y"][i] - y)) < r:
                        out.append(i)
        return out


def hamming(d1, d2):
    """dense DescriptorDistance matrix (fmatcher.cpp:2859-2875)"""
    a = np.unpackbits(np.asarray(d1, np.uint8), axis=1).astype(np.int32)
    b = np.unpackbits(np.asarray(d2, np.uint8), axis=1).astype(np.int32)
    return a.shape[1] - (a @ b.T + (1 - a) @ (1 - b).T)


def _three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_for_initialization(kps1, desc1, kps2, desc2, bounds, prev_matched=None, window=100, nnratio=0.9,
                              check_ori=True):
    """FMatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) with F2's grid over `bounds`
    (minX, maxX, minY, maxY).  -> (nmatches, vnMatches12 int32, updated vbPrevMatched float32 [n1, 2])"""
    TH_LOW, HISTO = 50, 30
    n1, n2 = len(kps1), len(kps2)
    pm = (np.stack([kps1["x"], kps1["y"]], 1) if prev_matched is None else np.asarray(prev_matched)) \
        .astype(np.float32).reshape(-1, 2).copy()
    dist = hamming(desc1, desc2) if n1 and n2 else np.zeros((n1, n2), np.int32)
    grid = Grid(kps2, bounds)
    m12 = np.full(n1, -1, np.int32)
    m21 = np.full(n2, -1, np.int32)
    matched = np.full(n2, 2**31 - 1, np.int64)
    rot_hist = [[] for _ in range(HISTO)]
    factor = np.float32(1.0) / np.float32(HISTO)
    ratio = np.float32(nnratio)
    nm = 0
    for i1 in range(n1):
        level1 = int(kps1["octave"][i1])
        if level1 > 0:
            continue
        idx2 = grid.query(pm[i1, 0], pm[i1, 1], window, level1, level1)
        if not idx2:
            continue
        best, best2, best_i = 2**31 - 1, 2**31 - 1, -1
        for i2 in idx2:
            d = int(dist[i1, i2])
            if matched[i2] <= d:
                continue
            if d < best:
                best2, best, best_i = best, d, i2
            elif d < best2:
                best2 = d
        if best <= TH_LOW and np.float32(best) < np.float32(best2) * ratio:
            if m21[best_i] >= 0:
                m12[m21[best_i]] = -1
                nm -= 1
            m12[i1] = best_i
            m21[best_i] = i1
            matched[best_i] = best
            nm += 1
            if check_ori:
                rot = np.float32(kps1["angle"][i1] - kps2["angle"][best_i])
                if rot < 0.0:
                    rot = np.float32(rot + np.float32(360.0))
                b = _round_half_away(np.float32(rot * factor))
                if b == HISTO:
                    b = 0
                rot_hist[b].append(i1)
    if check_ori:
        keep = _three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO):
            if i in keep:
                continue
            for j in rot_hist[i]:
                if m12[j] >= 0:
                    m12[j] = -1
                    nm -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            pm[i1, 0] = kps2["x"][m12[i1]]
            pm[i1, 1] = kps2["y"][m12[i1]]
    return nm, m12, pm
