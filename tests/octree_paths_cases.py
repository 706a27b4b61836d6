"""Frames and CPU-side facts for tests/test_gpu_octree_paths.py: what the oracle's quadtree did on a frame, stated from the
oracle's own candidates and selected keys and the geometry of the device kernel's fine grid (no GPU call here)."""
import numpy as np

from oracle import orbo

BORDER = 16  # the FAST border: candidates are relative to it, a level's selected keys are not


def grid_depth(w, h, quota):
    """depth of k_octree_v4's fine grid below the initial nodes (vslam::plan_octree, small frames: no LDS limit binds): one
    more than the depth at which a full quadtree has `quota` nodes"""
    n_ini = int(np.float32(w) / np.float32(h) + np.float32(0.5))
    d = 1
    while (n_ini << (2 * d)) < quota:
        d += 1
    return d + 1


def fine_cell(x, y, w, h, depth):
    """the node of depth `depth` that DivideNode's halvings (half = ceil(extent / 2), key < middle goes left / up) put (x, y) in"""
    n_ini = int(np.float32(w) / np.float32(h) + np.float32(0.5))
    hx = np.float32(w) / np.float32(n_ini)
    b = min(int(np.float32(x) / hx), n_ini - 1)
    x0, x1, y0, y1 = int(hx * np.float32(b)), int(hx * np.float32(b + 1)), 0, h
    code = b
    for _ in range(depth):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        qx, qy = int(x >= mx), int(y >= my)
        code = code * 4 + qx + 2 * qy
        x0, x1 = (mx, x1) if qx else (x0, mx)
        y0, y1 = (my, y1) if qy else (y0, my)
    return code


def _levels(img, nf):
    e = orbo.Extractor(nf)
    e.compute(img)
    q = e.tables()["quota"]
    for l in range(8):
        lh, lw = e.level(l).shape
        w, h = lw - 2 * BORDER, lh - 2 * BORDER
        yield l, w, h, grid_depth(w, h, int(q[l])), e.candidates(l), e.level_keys(l)


def level_candidates(img, nf):
    return [c for _, _, _, _, c, _ in _levels(img, nf)]


def candidate_cells(img, nf):
    """per level: the number of distinct fine cells that hold the level's candidates"""
    return [len({fine_cell(int(c["x"]), int(c["y"]), w, h, d) for c in cand}) for _, w, h, d, cand, _ in _levels(img, nf)]


def levels_below_grid(img, nf):
    """levels on which two SELECTED keys share a fine cell: each final node holds one selected key, so two of them inside one
    cell of the grid means final nodes deeper than the grid"""
    out = []
    for l, w, h, d, _, sel in _levels(img, nf):
        cells = [fine_cell(int(k["x"]) - BORDER, int(k["y"]) - BORDER, w, h, d) for k in sel]
        if len(set(cells)) < len(cells):
            out.append(l)
    return out


def tie_levels(img, nf):
    """levels on which "first key in order wins" decided a node: no two selected keys share a fine cell (every final node is
    a whole number of cells), and some selected key has a LATER candidate of the same response in its own cell, which is
    therefore in its node"""
    out = []
    for l, w, h, d, cand, sel in _levels(img, nf):
        ccell = np.asarray([fine_cell(int(c["x"]), int(c["y"]), w, h, d) for c in cand])
        scell = [fine_cell(int(k["x"]) - BORDER, int(k["y"]) - BORDER, w, h, d) for k in sel]
        if len(set(scell)) < len(scell):
            continue
        for k, f in zip(sel, scell):
            i = np.flatnonzero((cand["x"] == k["x"] - BORDER) & (cand["y"] == k["y"] - BORDER))
            assert len(i) == 1
            later = np.flatnonzero((ccell == f) & (cand["response"] == k["response"]))
            if np.any(later > i[0]):
                out.append(l)
                break
    return out


def clustered_dots(w=256, h=192, at=(115, 90)):
    """several bright dots three pixels apart on a flat frame: isolated dots are FAST corners, so the dots ARE the candidates"""
    img = np.full((h, w), 40, np.uint8)
    for a in range(3):
        for b in range(2):
            img[at[1] + 3 * b, at[0] + 3 * a] = 220 + 5 * (a + 3 * b)
    return img


def checker(period, w=320, h=240):
    """a periodic checkerboard: every inner crossing is the same corner, so responses repeat all over a level"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // period) + (yy // period)) & 1, 200, 60).astype(np.uint8)
