"""CPU restatement, in numpy float32, of the grid Harris / Shi-Tomasi detector vilib::HarrisGPU -- the yardstick of
tests/test_gpu_harrisgrid.py.  What it restates (thirdparty/vilib/visual_lib/src):
  1. derivatives   preprocess/conv_filter.cpp:124-160, conv_filter_row.cu:58-146, conv_filter_col.cu; harris_gpu.cpp:119-140
  2. products      feature_detection/harris/harris_gpu.cpp:141-170
  3. response      feature_detection/harris/harris_gpu_cuda_tools.cu:174-260
  4. grid          feature_detection/detector_base_gpu_cuda_tools.cu:700-878, as oracle/fastgrid_oracle.cpp's fg_grid_nms
  5. threshold     feature_detection/detector_base_gpu.cpp:228-248
Every numpy operation below is one float32 operation per element, rounded on its own, in the order in which the
reference's source text reads; DESIGN.md section 8 lists what the reference leaves undefined and what is chosen.
tests/test_harrisgrid_cpu.py pins grid_nms to the oracle's fg_detect and checks the filter taps, borders and tie order.
"""
import numpy as np

BORDER_SKIP, BORDER_ZERO, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(6)
F = np.float32
_Z, _Q, _H, _ONE, _NEG = F(0.0), F(0.25), F(0.5), F(1.0), F(-1.0)
SMOOTH = (_Q, _H, _Q)    # sobel_filter_1x3 (conv_filter.cpp:80)
DIFF = (_NEG, _Z, _ONE)  # diff_filter_1x3 (conv_filter.cpp:78)
INV255 = _ONE / F(255.0)
INV9 = _ONE / F(9.0)


def halfsample(img):
    """image_halfsample_gpu_kernel (pyramid_gpu.cu:76-96); level sizes are original >> l."""
    h, w = img.shape[0] >> 1, img.shape[1] >> 1
    s = img[:2 * h, :2 * w].astype(np.uint32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) >> 2).astype(np.uint8)


def border_index(n, border):
    """Source indices of positions -1 .. n of an axis of n pixels (conv_filter_row.cu:81-123); -1 stands for the
    value 0 (BORDER_ZERO, and BORDER_SKIP which runs the same kernels)."""
    idx = np.arange(-1, n + 1)
    if border in (BORDER_SKIP, BORDER_ZERO):
        lo, hi = -1, -1
    elif border == BORDER_REPLICATE:   # aaaaaa|abcdefgh|hhhhhhh
        lo, hi = 0, n - 1
    elif border == BORDER_REFLECT:     # fedcba|abcdefgh|hgfedcb
        lo, hi = 0, n - 1
    elif border == BORDER_WRAP:        # cdefgh|abcdefgh|abcdefg
        lo, hi = n - 1, 0
    elif border == BORDER_REFLECT_101:  # gfedcb|abcdefgh|gfedcba
        lo, hi = 1, n - 2
    else:
        raise ValueError("border type")
    idx[0], idx[-1] = lo, hi
    return idx


def pad(img, border):
    """The image with the ring one step outside it, float32, (h + 2, w + 2).  The rule is applied per axis and per
    pass in the reference; for a 3-tap separable filter that is this ring (rows below the image included: the border
    rule, as the column kernel's comments intend, not the unbounded load of conv_filter_col.cu:78-82)."""
    h, w = img.shape
    iy, ix = border_index(h, border), border_index(w, border)
    out = img[np.clip(iy, 0, h - 1)][:, np.clip(ix, 0, w - 1)].astype(F)
    out[iy < 0, :] = _Z
    out[:, ix < 0] = _Z
    return out


def _tap3(f, v0, v1, v2):
    """sum = 0.0f; sum += f[j] * v[j] for j = 0, 1, 2 (conv_filter_row.cu:131-136)."""
    s = np.zeros(v0.shape, F)
    s = s + f[0] * v0
    s = s + f[1] * v1
    s = s + f[2] * v2
    return s


def derivatives(img, border, scale=True):
    """(Dx, Dy), float32, image-sized.  Dx: column pass {.25,.5,.25} then row pass {-1,0,1}; Dy: column pass {-1,0,1}
    then row pass {.25,.5,.25}; the column pass is scaled by 1.0f, the row pass by 1.0f/255.f (scale=False: by 1.0f)."""
    h, w = img.shape
    P = pad(img, border)
    out = []
    for fcol, frow in ((SMOOTH, DIFF), (DIFF, SMOOTH)):
        T = _tap3(fcol, P[0:h, :], P[1:h + 1, :], P[2:h + 2, :]) * _ONE
        D = _tap3(frow, T[:, 0:w], T[:, 1:w + 1], T[:, 2:w + 2])
        out.append(D * (INV255 if scale else _ONE))
    return out[0], out[1]


def _fma(a, b, c):
    """float64 emulation of a fused multiply-add of float32 operands (the product is exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def response(img, border, use_harris=True, k=0.04, fused=False):
    """The corner response of one level: computed in [m, w-1-m] x [m, h-1-m] (m = 2 for BORDER_SKIP, else 1), 0.0f
    elsewhere.  fused=True contracts the last formula into FMAs the way a CUDA compiler may; it is there to show that
    the choice matters, not as a yardstick."""
    h, w = img.shape
    m = 2 if border == BORDER_SKIP else 1
    out = np.zeros((h, w), F)
    if w < 2 * m + 1 or h < 2 * m + 1:
        return out
    dx, dy = derivatives(img, border)
    dxdy, dx2, dy2 = dx * dy, dx * dx, dy * dy
    sums = []
    for p in (dx2, dxdy, dy2):
        s = np.zeros((h - 2, w - 2), F)
        for j in range(3):          # raster order from 0.0f (harris_gpu_cuda_tools.cu:183-205)
            for i in range(3):
                s = s + p[j:j + h - 2, i:i + w - 2]
        sums.append(s * INV9)
    a, b, c = sums
    kf = F(k)
    if use_harris:                  # r = a*c - b*b - k*(a+c)*(a+c)
        if fused:
            r = _fma(-(kf * (a + c)), a + c, _fma(a, c, -(b * b)))
        else:
            r = ((a * c) - (b * b)) - ((kf * (a + c)) * (a + c))
    else:                           # r = (a+c) - sqrtf((a-c)*(a-c) + 4*b*b)
        if fused:
            r = (a + c) - np.sqrt(_fma(a - c, a - c, (F(4.0) * b) * b))
        else:
            r = (a + c) - np.sqrt(((a - c) * (a - c)) + ((F(4.0) * b) * b))
    r = r.astype(F)
    out[m:h - m, m:w - m] = r[m - 1:h - 1 - m, m - 1:w - 1 - m]
    return out


def nms3x3(resp):
    """K3's suppression at every pixel: c *= -0.5f * (-1.0f + copysignf(1.0f, neighbour - c)) over the 8 neighbours in
    raster order (strictly greater survives; anything else becomes +-0); neighbours outside the image are 0."""
    h, w = resp.shape
    P = np.zeros((h + 2, w + 2), F)
    P[1:h + 1, 1:w + 1] = resp
    c = resp.astype(F).copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            nb = P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            c = c * (F(-0.5) * (_NEG + np.copysign(_ONE, nb - c)))
    return c


def grid_nms(level, min_level, resp, hb, vb, cw, ch, n_cols, n_rows, pos, score, lvl, tie_rule):
    """Port of oracle/fastgrid_oracle.cpp's fg_grid_nms: K3 for one level, merged into pos / score / lvl in place.
    tie_rule 0 walks the kernel's own threads (a thread per column keeps its topmost maximum), 32-lane shfl_down tree
    and warps; tie_rule 1 is raster order inside the cell.  Only pixels that survive the suppression with a positive
    value can change anything, so only those are walked."""
    h, w = resp.shape
    cwl, chl = cw >> level, ch >> level
    if cwl < 1 or chl < 1:
        return
    ncell = n_cols * n_rows
    if level == min_level:
        score[:] = _Z
    bdx, bdy = cwl, max(1, min(128 // cwl, chl))
    warp_cnt = (bdx * bdy + 31) >> 5
    scale = F(1 << level)
    v = nms3x3(resp)
    ys, xs = np.nonzero(v > 0)      # raster order
    ok = (xs >= hb) & (xs < w - hb) & (ys >= vb) & (ys < h - vb)
    ys, xs = ys[ok], xs[ok]
    bx, by = xs // cwl, ys // chl
    ok = (bx < n_cols) & (by < n_rows)
    ys, xs, bx, by = ys[ok], xs[ok], bx[ok], by[ok]
    cells = (by * n_cols + bx).tolist()
    vals = v[ys, xs]
    best_r, best_x, best_y = np.zeros(ncell, F), np.zeros(ncell, F), np.zeros(ncell, F)
    if tie_rule == 1:
        for i, cell in enumerate(cells):
            if vals[i] > best_r[cell]:
                best_r[cell], best_x[cell], best_y[cell] = vals[i], xs[i], ys[i]
    else:
        th_r = np.zeros((ncell, warp_cnt * 32), F)  # lanes beyond the block contribute nothing
        th_x, th_y = np.zeros_like(th_r), np.zeros_like(th_r)
        yoff = np.maximum(0, vb - chl * by)
        line = ys - chl * by
        t = ((xs - cwl * bx) + bdx * ((line - yoff) % bdy)).tolist()
        for i, cell in enumerate(cells):            # rows ascend: a thread keeps its topmost maximum
            if line[i] >= yoff[i] and vals[i] > th_r[cell, t[i]]:
                th_r[cell, t[i]], th_x[cell, t[i]], th_y[cell, t[i]] = vals[i], xs[i], ys[i]
        R, X, Y = (a.reshape(ncell, warp_cnt, 32) for a in (th_r, th_x, th_y))
        for off in (16, 8, 4, 2, 1):                # __shfl_down_sync tree
            take = np.zeros(R.shape, bool)
            take[..., :32 - off] = R[..., off:] > R[..., :32 - off]
            sh = [np.concatenate([a[..., off:], a[..., :off]], axis=-1) for a in (R, X, Y)]
            R, X, Y = (np.where(take, s, a) for s, a in zip(sh, (R, X, Y)))
        best_r, best_x, best_y = R[:, 0, 0].copy(), X[:, 0, 0].copy(), Y[:, 0, 0].copy()
        for wi in range(1, warp_cnt):               # warps in ascending order, strict
            better = R[:, wi, 0] > best_r
            best_r = np.where(better, R[:, wi, 0], best_r)
            best_x = np.where(better, X[:, wi, 0], best_x)
            best_y = np.where(better, Y[:, wi, 0], best_y)
    upd = score < best_r                            # levels in ascending order, strict
    score[upd] = best_r[upd]
    pos[upd, 0] = best_x[upd] * scale
    pos[upd, 1] = best_y[upd] * scale
    lvl[upd] = level


def minimum_border(filter_border):
    """MINIMUM_BORDER (harris_gpu.cpp:58-59): NMS + box sum (+ 1 for BORDER_SKIP)."""
    return 3 if filter_border == BORDER_SKIP else 2


def threshold(score, quality_level):
    """processGridAndThreshold (detector_base_gpu.cpp:228-248) -> (keep[cells], n_keep)."""
    keep = score > (score.max() * F(quality_level))
    return keep, int(keep.sum())


def detect(img, cell=(32, 32), min_level=0, max_level=1, border=(0, 0), filter_border=BORDER_SKIP, use_harris=True,
           k=0.04, quality_level=0.1, tie_rule=0):
    """HarrisGPU::detect on one image -> (pos[cells, 2], score[cells], level[cells], keep[cells], n_keep); cells
    without a corner carry pos (0, 0), score 0, level -1."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    n_cols, n_rows = (w + cell[0] - 1) // cell[0], (h + cell[1] - 1) // cell[1]
    mb = minimum_border(filter_border)
    hb, vb = max(mb, border[0]), max(mb, border[1])
    pos = np.zeros((n_cols * n_rows, 2), F)
    score = np.zeros(n_cols * n_rows, F)
    lvl = np.full(n_cols * n_rows, -1, np.int32)
    cur = img
    for l in range(max_level):
        if l:
            cur = halfsample(cur)
        if l < min_level:
            continue
        grid_nms(l, min_level, response(cur, filter_border, use_harris, k), hb, vb, cell[0], cell[1], n_cols, n_rows,
                 pos, score, lvl, tie_rule)
    keep, n_keep = threshold(score, quality_level)
    return pos, score, lvl, keep, n_keep
