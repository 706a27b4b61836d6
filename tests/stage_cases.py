"""Frames of the stage-wise parity tests (tests/test_gpu_stages.py) and the edge classes of the blur and FAST kernels
that each of their pyramid levels hits; tests/test_stage_cases_cpu.py asserts that the frames jointly hit every class.
Pure CPU: level sizes are restated here, the FAST plan (cells, bands, column-table classes) comes from libvslam_host.so.

Blur classes, from k_blur7_v2 (vi_slam_amd/csrc/vslam_image_kernels.hip:63-170) and its task list
(vslam_context.hip:248-254: ns = max(1, (w + 247) / 248) strips, nc = ceil(h / R) row chunks per level):
  - strip s starts at ox0 = min(248 s, max(w - 248, 0)) (:84) and lane k owns columns ox0 - 4 + 4k .. +3 (:85); lanes 1..62
    with x < w store (:132).  w < 248: one strip whose last lanes lie past the image.  w == 248: one full strip.  w == 249:
    the second strip starts at column 1, so 247 columns are written twice.  250..496: two strips.  >= 497: three or more.
  - the last strip of a level with w > 248 starts at w - 248, so its lanes' first column is congruent to w mod 4: for
    w % 4 != 0 every dword store (:160) of that strip is unaligned ("shifted w%4=k").  A lane's quad straddles the image
    edge only on a one-strip level, where x = 4k - 4: the byte stores (:161-165) run for w % 4 = 1, 2, 3 ("tail w%4=k");
    w % 4 == 0 there ends on a full dword.
  - rows: chunk c covers rows cR .. min(cR + R, h) (:86-87).  The prologue reads rows y0 - 3 .. y0 + 2 and the prefetch ring
    rows y0 + 3 .. y0 + 8 (:118-137), reflected at the level's edge (:101): with a last chunk of 1..6 rows every ring entry
    past row h - 1 is a reflected row ("last<=6"), with h % R == 1 the chunk is a single row whose whole lower window is
    reflected.  The row loop is unrolled by six (:138-142): nlast % 6 == 1 and == 5 leave one and five rows to the
    partial trip, where nlast = h % R or R is the last chunk's height.  "one chunk": h <= R.
  - vslam_fe_create takes no level below 40 px either way (vslam_context.hip:78), so "one chunk" cannot occur with R = 8
    (contexts of one or two images) or R = 32 (batches): only a blur_rows override of at least a level's height reaches it,
    and test_gpu_stages.py carries one.  Every other height class is required for both R = 8 and R = 32.

FAST classes, from vslam::build_cells / build_bands / pack_bands (vslam_host.cpp), which feed both
k_fast_cells_v3 (one workgroup per cell) and k_fast_bands (one per band):
  - one cell row / one cell column on a level (30 <= side - 32 < 60);
  - the last cell of a row / column narrower or shorter than the others (clipped at the border, in build_cells);
  - a band of four cells; a band cut short because a fourth (or third ...) interior would pass 128 px, i.e. a cell row of
    pitch > 32 with more cells than 128 / pitch (build_bands);
  - a level with more than one column-table class (pitch, interior width) among its bands (pack_bands);
  - the smallest candidate segment ceil(iw / 2) * ceil(ih / 2) of a cell (vslam_context.hip:204).  The clipped last cell
    of a row is narrowest where the level is just too narrow for one more column; among levels of at most 520 x 300 px
    that is 10 x 18 px (a level of 513 x 273), found by smallest_segment() below rather than written down;
  - a cell without a corner at iniThFAST, which reruns at minThFAST, beside one of the same cell row that has one.
The paths inside the two FAST kernels that depend on a frame's largest window (LDS pitch, staged sweeps, quad columns,
row chunks of a band) are classes of a frame: fast_path_classes() below.
"""
import ctypes as C
import os

import numpy as np

BV_OUTW = 248
MIN_LEVEL = 40     # vslam_context.hip:78
FAST_BORDER = 16   # EDGE_THRESHOLD - 3

# (w, h, nlevels, scale, nfeatures, iniThFAST, minThFAST); level 0 at most about 520 x 300
FRAMES = [
    (298, 166, 8, 1.2, 300, 20, 7),
    (299, 167, 8, 1.2, 300, 35, 12),
    (517, 149, 8, 1.2, 500, 20, 7),
    (497, 290, 6, 1.2, 120, 20, 7),
    (513, 273, 4, 1.2, 400, 20, 7),
    (69, 69, 4, 1.2, 60, 20, 7),
    (331, 140, 4, 1.5, 200, 20, 7),
    (250, 93, 5, 1.2, 150, 20, 7),
    (446, 201, 8, 1.2, 400, 30, 10),
    (110, 90, 2, 1.2, 80, 20, 7),
    (160, 69, 2, 1.2, 100, 30, 10),   # the smallest level 0 whose ramp overflows a band list first at minThFAST (band_overflow_classes)
]


def frame_id(f):
    return "%dx%d_l%d_s%.1f_n%d_t%d_%d" % f


def level_sizes(w, h, nlevels, scale):
    """[(lw, lh)] as vslam::build_tables / level_size have them (vslam_host.cpp): the scale factors are floats
    multiplied up in double, the inverse is a float division, the size is cvRound (to nearest, ties to even) of a float
    product."""
    s = np.float32(1.0)
    out = []
    for l in range(nlevels):
        if l:
            s = np.float32(float(s) * float(np.float32(scale)))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


_H = None


def host():
    global _H
    if _H is None:
        import vi_slam_amd as V
        _H = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(V.__file__)), "libvslam_host.so"))
    return _H


def cells(level, lw, lh):
    """rows (level, x0, y0, x1, y1) of vslam::build_cells"""
    out = np.zeros((4096, 5), np.uint16)
    n = host().vslamh_cells(level, lw, lh, out.ctypes.data_as(C.c_void_p), len(out))
    assert 0 <= n <= len(out)
    return out[:n].astype(int)


def bands(level, lw, lh):
    """rows (cell0, level, ncell, wcell, x0, y0, ww, wh) of vslam::build_bands as vslam_fe_create calls it (4 cells, 128 px)"""
    out = np.zeros((4096, 8), np.uint32)
    n = host().vslamh_bands(level, lw, lh, 4, 128, out.ctypes.data_as(C.c_void_p), len(out))
    assert 0 <= n <= len(out)
    return out[:n].astype(int)


def band_plan_ok(sizes):
    """vslam::pack_bands over all levels says the band words can hold the list and the limits of vk_fast_bands_check hold
    (128 interior columns, windows of at most 133 rows, 4 cells): the context then runs k_fast_bands where it is chosen
    instead of falling back to k_fast_cells_v3 (vslam_context.hip:228, vslam_fe.hip:100)"""
    cl = np.concatenate([cells(l, w, h) for l, (w, h) in enumerate(sizes)]).astype(np.uint16)
    if len(cl) == 0:
        return False
    cl = np.ascontiguousarray(cl)
    words = np.zeros((4096, 4), np.uint32)
    classes = np.zeros(272 * 256, np.uint8)
    info = np.zeros(5, np.int32)
    vp = C.c_void_p
    nb = host().vslamh_band_tables(cl.ctypes.data_as(vp), len(cl), len(sizes), 4, 128, words.ctypes.data_as(vp), len(words),
                                   classes.ctypes.data_as(vp), len(classes), info.ctypes.data_as(vp))
    return nb > 0 and info[4] == 1 and info[2] <= 128 and info[1] <= 133 and info[3] <= 4


def accepted(w, h, nlevels, scale):
    """vslam_fe_create's geometry checks (vslam_context.hip:78-86, :193): every level 40..4127 px both ways and no portrait
    level (round((lw - 32) / (lh - 32)) >= 1 in float), and a FAST cell on some level"""
    sizes = level_sizes(w, h, nlevels, scale)
    for lw, lh in sizes:
        if lw < MIN_LEVEL or lh < MIN_LEVEL or lw > 4127 or lh > 4127:
            return False
        if int(np.rint(np.float32(lw - 32) / np.float32(lh - 32))) < 1:
            return False
    return any(len(cells(l, lw, lh)) for l, (lw, lh) in enumerate(sizes))


BLUR_WIDTH_CLASSES = (["w<248", "w==248", "w==249", "250<=w<=496", "w>=497"] + ["tail w%%4=%d" % k for k in range(4)] +
                      ["shifted w%%4=%d" % k for k in range(4)] + ["w==40"])
BLUR_HEIGHT_CLASSES = ["h%R==0", "h%R==1", "last<=6", "nlast%6==1", "nlast%6==5", "h==40"]
BLUR_ONE_CHUNK = "one chunk"


def blur_width_classes(lw):
    out = set()
    if lw < BV_OUTW:
        out |= {"w<248", "tail w%%4=%d" % (lw % 4)}
    else:
        out.add("w==248" if lw == 248 else "w==249" if lw == 249 else "250<=w<=496" if lw <= 496 else "w>=497")
        if lw > BV_OUTW:
            out.add("shifted w%%4=%d" % (lw % 4))
    if lw == MIN_LEVEL:
        out.add("w==40")
    return out


def blur_height_classes(lh, R):
    out = set()
    nlast = lh % R or R
    if lh % R == 0:
        out.add("h%R==0")
    if lh % R == 1:
        out.add("h%R==1")
    if nlast <= 6:
        out.add("last<=6")
    if nlast % 6 in (1, 5):
        out.add("nlast%%6==%d" % (nlast % 6))
    if lh <= R:
        out.add(BLUR_ONE_CHUNK)
    if lh == MIN_LEVEL:
        out.add("h==40")
    return out


def last_chunk_rows(lh, R):
    return lh % R or R


FAST_PLAN_CLASSES = ["one cell row", "one cell column", "last cell narrower", "last cell shorter", "band of four",
                     "band cut at 128 px", "two band classes", "smallest segment"]
FAST_IMAGE_CLASS = "minTh cell beside iniTh cell"


def fast_plan_classes(level, lw, lh):
    cl = cells(level, lw, lh)
    out = set()
    if len(cl) == 0:
        return out
    bd = bands(level, lw, lh)
    rows, cols = sorted(set(cl[:, 2])), sorted(set(cl[:, 1]))
    if len(rows) == 1:
        out.add("one cell row")
    if len(cols) == 1:
        out.add("one cell column")
    cw, ch = cl[:, 3] - cl[:, 1], cl[:, 4] - cl[:, 2]
    last_col, last_row = cl[:, 1] == cols[-1], cl[:, 2] == rows[-1]
    if len(cols) > 1 and cw[last_col].max() < cw[~last_col].min():
        out.add("last cell narrower")
    if len(rows) > 1 and ch[last_row].max() < ch[~last_row].min():
        out.add("last cell shorter")
    if (bd[:, 2] == 4).any():
        out.add("band of four")
    for y0 in rows:
        b = bd[bd[:, 5] == y0]
        per = max(1, min(4, 128 // max(int(b[0, 3]), 1)))
        if per < 4 and len(b) > 1 and (b[:-1, 2] == per).all():
            out.add("band cut at 128 px")
    if len({(int(b[3]), int(b[6]) - 6) for b in bd}) > 1:
        out.add("two band classes")
    if ((cw - 5) // 2 * ((ch - 5) // 2)).min() == smallest_segment():
        out.add("smallest segment")
    return out


FAST_PATH_CLASSES = ["cells: pitch 48", "cells: pitch 72", "cells: pitch 48, rows past the staged sweeps",
                     "cells: pitch 72, rows past the staged sweeps", "cells: 8 quad columns", "cells: 16 quad columns",
                     "bands: 8 quad slots", "bands: 16 quad slots", "bands: 32 quad slots", "bands: one row chunk",
                     "bands: several row chunks", "bands: rows past the staged sweeps"]


def fast_path_classes(f):
    """The paths inside the two FAST kernels that a frame's cells and bands take.  Their shapes follow the frame's largest
    window, so these are classes of a frame, not of a level.
    k_fast_cells_v3 (128 threads): LDS pitch 48 if the widest window, rounded up to 4, is at most 42 px, else 72
    (vslam_context.hip:208, vslam_image_kernels.hip:897); two sweeps of 21 rows (pitch 48) or four of 14 (pitch 72) are
    staged through registers and taller windows take the row loop behind them (:630-659); interiors of more than 32 px
    take 16 quad columns per sweep, the others 8 (:664-665).
    k_fast_bands (256 threads, pitch 136): 8, 16 or 32 quad slots per row by the band's interior width (:1097); the
    survivor list gets what 20 KB leave beside the tallest window of the frame, and a band taller than lcap >> 7 rows is
    swept in several row chunks (:1043, :1088, :1330-1359); windows of more than 52 rows take the staging row loop
    (:1048, :1078-1080)."""
    sizes = level_sizes(*f[:4])
    cl = np.concatenate([cells(l, lw, lh) for l, (lw, lh) in enumerate(sizes)])
    bd = np.concatenate([bands(l, lw, lh) for l, (lw, lh) in enumerate(sizes)])
    out = set()
    cw, ch = cl[:, 3] - cl[:, 1], cl[:, 4] - cl[:, 2]
    pitch = 48 if ((cw.max() + 3) & ~3) <= 42 else 72
    out.add("cells: pitch %d" % pitch)
    if ch.max() > (42 if pitch == 48 else 56):
        out.add("cells: pitch %d, rows past the staged sweeps" % pitch)
    out |= {"cells: %d quad columns" % (16 if iw > 32 else 8) for iw in cw - 6}
    out |= {"bands: %d quad slots" % (32 if iw > 64 else 16 if iw > 32 else 8) for iw in bd[:, 6] - 6}
    max_wh = int(bd[:, 7].max())
    lds = band_lds(max_wh)
    for wh in bd[:, 7]:
        out.add("bands: one row chunk" if (band_list_capacity(lds, int(wh)) >> 7) >= wh - 6 else "bands: several row chunks")
    if max_wh > 52:
        out.add("bands: rows past the staged sweeps")
    return out


def _band_fixed_lds(wh):
    """fast_band_fixed_lds (vslam_image_kernels.hip:1330): window, score tile, keep words, column tables"""
    ih, whe = wh - 6, (wh + 1) & ~1
    return whe * 136 + (((ih + 2) * 136 + 15) & ~15) + ih * 4 * 4 + 136 + 136 + 32


def band_lds(max_wh):
    """LDS bytes of a k_fast_bands workgroup in a context whose tallest band window has max_wh rows (vk_fast_bands, :1356-1359)"""
    lds = max(20480 - 64, _band_fixed_lds(max_wh) + 2 * 8 * 2 * 128, (max_wh + 256 // 8 + 1) * 136 + 256)
    return (lds + 15) & ~15


def band_list_capacity(lds, wh):
    """entries of the survivor list of a band whose window has wh rows (:1043)"""
    return ((lds - _band_fixed_lds(wh)) >> 1) & ~1


def frame_max_band_rows(f):
    sizes = level_sizes(*f[:4])
    return int(max(b[:, 7].max() for b in (bands(l, lw, lh) for l, (lw, lh) in enumerate(sizes)) if len(b)))


FAST_OVERFLOW_CLASS = "bands: survivor list overflows, rows swept again"


def band_list_overflows(level_img, level, th, lds):
    """bands of a level whose first row chunk lists more survivors of the compass pre-test at threshold th than the list
    holds, so that k_fast_bands sweeps these rows again, half as many at a time (:1188-1191).  A pixel is listed once per
    polarity it passes (:1137-1138): dark if max(min(down, up), min(right, left)) < v - th, bright if min(max(down, up),
    max(right, left)) > v + th, with the four compass pixels three away.  -> [(band index, entries, capacity)]"""
    img = level_img.astype(np.int64)
    lh, lw = img.shape
    v, u, d, l, r = img[3:-3, 3:-3], img[:-6, 3:-3], img[6:, 3:-3], img[3:-3, :-6], img[3:-3, 6:]
    dark = np.maximum(np.minimum(d, u), np.minimum(r, l)) < v - th
    bright = np.minimum(np.maximum(d, u), np.maximum(r, l)) > v + th
    n = dark.astype(np.int64) + bright  # [y - 3, x - 3] of level pixel (x, y)
    out = []
    for i, (_, _, _, _, x0, y0, ww, wh) in enumerate(bands(level, lw, lh)):
        lcap = band_list_capacity(lds, int(wh))
        rows = min(wh - 6, lcap >> 7)
        entries = int(n[y0:y0 + rows, x0:x0 + ww - 6].sum())  # interior pixel (ix, iy) is level pixel (x0 + 3 + ix, y0 + 3 + iy)
        if entries > lcap:
            out.append((i, entries, lcap))
    return out


FAST_OVERFLOW_CLASSES = ["bands: list overflows in the first chunk of the first stage",
                         "bands: list overflows first at minThFAST, behind a chunk that listed something"]


def band_overflow_classes(level_img, level, ini_th, min_th, lds):
    """Where the first overflow of a band's survivor list falls.  Before the first chunk of the first stage both of the
    kernel's two counters are zero; behind any other chunk one of them still holds that chunk's totals, which the retry must
    not count from (it once did: level 0 of the 446 x 201 ramp at thresholds 30 / 10 came out with 22549 candidates for
    none).  The second class asks for what made that visible: no overflow at iniThFAST, entries listed there, every cell
    of the band empty so that the whole band is swept again at minThFAST, an overflow there, and half as many rows plus the
    earlier entries past the capacity again."""
    lh, lw = level_img.shape
    at_ini = {i: (e, c) for i, e, c in band_list_overflows(level_img, level, ini_th, lds)}
    at_min = {i: (e, c) for i, e, c in band_list_overflows(level_img, level, min_th, lds)}
    out = set()
    if at_ini:
        out.add(FAST_OVERFLOW_CLASSES[0])
    low = min_threshold_cells(level_img, level, ini_th)
    img = level_img.astype(np.int64)
    v, u, d, l, r = img[3:-3, 3:-3], img[:-6, 3:-3], img[6:, 3:-3], img[3:-3, :-6], img[3:-3, 6:]

    def entries(th, x0, y0, ww, rows):
        n = (np.maximum(np.minimum(d, u), np.minimum(r, l)) < v - th).astype(np.int64) + \
            (np.minimum(np.maximum(d, u), np.maximum(r, l)) > v + th)
        return int(n[y0:y0 + rows, x0:x0 + ww - 6].sum())
    for i, (cell0, _, ncell, _, x0, y0, ww, wh) in enumerate(bands(level, lw, lh)):
        if i in at_ini or i not in at_min or not low[cell0:cell0 + ncell].all():
            continue
        lcap = band_list_capacity(lds, int(wh))
        if (lcap >> 7) < wh - 6:
            continue  # several chunks at iniThFAST: the counter behind the last one is not worked out here
        stale = entries(ini_th, x0, y0, ww, wh - 6)
        if stale > 0 and stale + entries(min_th, x0, y0, ww, max(2, lcap >> 8)) > lcap:
            out.add(FAST_OVERFLOW_CLASSES[1])
    return out


MAX_W, MAX_H = 520, 300
_smallest = []


def smallest_segment():
    """the smallest ceil(iw / 2) * ceil(ih / 2) of any cell of any level of at most MAX_W x MAX_H px: interior widths depend
    on the level's width alone and heights on its height alone, so the two are searched separately"""
    if not _smallest:
        iw = min((c[:, 3] - c[:, 1] - 6).min() for c in (cells(0, lw, 100) for lw in range(62, MAX_W + 1)))
        ih = min((c[:, 4] - c[:, 2] - 6).min() for c in (cells(0, 200, lh) for lh in range(62, MAX_H + 1)))
        _smallest.append(int((iw + 1) // 2 * ((ih + 1) // 2)))
    return _smallest[0]


def min_threshold_cells(level_img, level, ini_th):
    """per cell of the level, in cell order: True where cv::FAST at iniThFAST finds nothing in the cell's window, so the cell
    is detected again at minThFAST (fextractor.cpp:803-807)"""
    from oracle import orbo
    lh, lw = level_img.shape
    return np.array([len(orbo.fast_detect(level_img[y0:y1, x0:x1], ini_th)) == 0
                     for _, x0, y0, x1, y1 in cells(level, lw, lh)], bool)


def fast_image_classes(level_img, level, ini_th):
    lh, lw = level_img.shape
    cl = cells(level, lw, lh)
    if len(cl) < 2:
        return set()
    low = min_threshold_cells(level_img, level, ini_th)
    same_row = cl[1:, 2] == cl[:-1, 2]
    return {FAST_IMAGE_CLASS} if (same_row & (low[1:] != low[:-1])).any() else set()


DENSE = ["ramp", "noise3", "checker3"]


def dense_image(f, name):
    """Images that fill the kernels' lists.  ramp: a diagonal ramp of 10 per pixel that wraps at 256 -- away from the wrap
    lines every pixel passes the compass pre-test in BOTH polarities (up and left darker, down and right brighter by 30)
    and none is a corner, along them corners crowd; noise3: three grey levels, the densest mix of dark, bright and both;
    checker3: the same corner all over a level."""
    w, h = f[0], f[1]
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "ramp":
        return ((10 * (xx + yy)) & 255).astype(np.uint8)
    if name == "noise3":
        return (np.random.default_rng(1000 * w + h).integers(0, 3, (h, w)) * 127).astype(np.uint8)
    if name == "checker3":
        return (((xx // 3 + yy // 3) & 1) * 255).astype(np.uint8)
    raise KeyError(name)


def frame_image(f, k=0):
    """image k of a frame: the scenes of tests/test_gpu_extract.py (seed = w + nfeatures), other steps for the other slots;
    a name of DENSE: that pattern at the frame's size"""
    if isinstance(k, str):
        return dense_image(f, k)
    from vi_slam_amd import synth
    return synth.make_frame(f[0], f[1], seed=f[0] + f[4], step=k)


def blur_rows_overrides(f):
    """blur_rows values for the override contexts of a frame: the smallest R >= 8 that leaves a last chunk of one row on
    some level, the same for five rows, and one R of at least the last level's height (a level with one row chunk)"""
    sizes = level_sizes(*f[:4])
    out = []
    for want in (1, 5):
        out.append(next(R for R in range(8, 513) if any(lh > R and lh % R == want for _, lh in sizes)))
    out.append(min(512, ((sizes[-1][1] + 7) // 8) * 8))
    return out
