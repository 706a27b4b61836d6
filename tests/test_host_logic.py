"""CPU: the product's host-side logic (vi_slam_amd/csrc/vslam_host.cpp, built GPU-free into
libvslam_host.so) against the oracle, and the C ABI library's export table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(V.HOST_LIB_PATH)
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_octree(H, xyr, W, Hh, N):
    xyr = np.ascontiguousarray(xyr, np.int32).reshape(-1, 3)
    out = np.zeros((len(xyr) + 8, 3), np.int32)
    n = H.vslamh_octree(_p(xyr), len(xyr), W, Hh, N, _p(out), len(out))
    assert n >= 0
    return out[:n]


@pytest.mark.parametrize("nf", [500, 1000, 2000, 4000, 10000])
def test_tables_equal_oracle(H, nf):
    sf, isf, s2, is2 = (np.zeros(8, np.float32) for _ in range(4))
    q = np.zeros(8, np.int32)
    um = np.zeros(16, np.int32)
    dn = C.c_int()
    H.vslamh_tables(nf, C.c_float(1.2), 8, _p(sf), _p(isf), _p(s2), _p(is2), _p(q), _p(um), C.byref(dn))
    t = orbo.Extractor(nf).tables()
    assert np.array_equal(sf, t["scale"]) and np.array_equal(isf, t["inv_scale"])
    assert np.array_equal(s2, t["sigma2"]) and np.array_equal(is2, t["inv_sigma2"])
    assert np.array_equal(q, t["quota"]) and np.array_equal(um, t["umax"])
    assert dn.value == 749  # pixels of the radius-15 disc


@pytest.mark.parametrize("size", [(1241, 376), (1920, 1080), (752, 480), (321, 203)])
def test_resize_tables_reproduce_oracle_resize(H, size):
    w, h = size
    e = orbo.Extractor(1000)
    img = synth.make_frame(w, h, seed=w)
    e.pyramid_only(img)
    for l in range(1, 8):
        src, want = e.level(l - 1), e.level(l)
        lw, lh = C.c_int(), C.c_int()
        H.vslamh_level_size(1000, C.c_float(1.2), 8, w, h, l, C.byref(lw), C.byref(lh))
        assert (lw.value, lh.value) == want.shape[::-1]
        got = np.zeros_like(want)
        H.vslamh_resize_with_tables(_p(src), src.shape[1], src.shape[0], C.c_size_t(src.shape[1]), _p(got),
                                    lw.value, lh.value, C.c_size_t(lw.value))
        assert np.array_equal(got, want)


def test_cell_grid_counts_kitti(H):
    # executed cells per level after the skip rules of fextractor.cpp:785,794
    sizes = [(1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126), (346, 105)]
    counts = []
    for l, (w, h) in enumerate(sizes):
        out = np.zeros((4096, 5), np.uint16)
        n = H.vslamh_cells(l, w, h, _p(out), 4096)
        counts.append(n)
        c = out[:n]
        # interiors (window minus the 3-px ring) tile [19, w-19) x [19, h-19) exactly
        cover = np.zeros((h, w), np.int32)
        for _, x0, y0, x1, y1 in c:
            cover[y0 + 3:y1 - 3, x0 + 3:x1 - 3] += 1
        assert np.all(cover[19:h - 19, 19:w - 19] == 1)
        cover[19:h - 19, 19:w - 19] = 0
        assert not cover.any()
    assert counts == [429, 297, 189, 132, 72, 45, 36, 20] and sum(counts) == 1220


@pytest.mark.parametrize("size", [(1241, 376), (1920, 1080), (752, 480), (640, 360), (512, 512), (179, 100), (143, 143), (95, 70)])
@pytest.mark.parametrize("per", [1, 2, 3, 4])
def test_bands_cover_every_cell_once(H, size, per):
    """k_fast_bands' work list (vslam::build_bands): consecutive cells of one cell row, constant pitch, interiors of a
    band at most 128 px wide, every cell in exactly one band, band windows = the union of their cells' windows"""
    w0, h0 = size
    for l in range(8):
        w, h = int(round(w0 / 1.2 ** l)), int(round(h0 / 1.2 ** l))
        cells = np.zeros((8192, 5), np.uint16)
        nc = H.vslamh_cells(l, w, h, _p(cells), 8192)
        bands = np.zeros((8192, 8), np.uint32)
        maxw = 128  # k_fast_bands' interior columns (vslam_fe.hip)
        nb = H.vslamh_bands(l, w, h, per, maxw, _p(bands), 8192)
        if nc == 0:
            assert nb == 0
            continue
        cells, bands = cells[:nc].astype(int), bands[:nb].astype(int)
        seen = np.zeros(nc, int)
        for cell0, lev, ncell, wcell, x0, y0, ww, wh in bands:
            assert 1 <= ncell <= per and lev == l and ww - 6 <= maxw
            for k in range(ncell):
                c = cells[cell0 + k]
                seen[cell0 + k] += 1
                assert c[2] == y0 and c[4] == y0 + wh            # one cell row
                assert c[1] == x0 + k * wcell                    # constant pitch
                # cell k's interior columns inside the band's interior: [k * wcell, min((k + 1) * wcell, iw))
                assert c[3] - c[1] - 6 == min((k + 1) * wcell, ww - 6) - k * wcell > 0
            assert cells[cell0 + ncell - 1][3] == x0 + ww
            assert (wcell * ((65536 + wcell - 1) // wcell)) >> 16 >= 1  # the kernel's x / wcell by multiplication ...
            rc = (65536 + wcell - 1) // wcell
            assert all((x * rc) >> 16 == x // wcell for x in range(256))   # ... is exact on its domain
        assert np.all(seen == 1)
        assert np.all(np.diff(bands[:, 0]) > 0)


def test_octree_equals_oracle_on_extractor_candidates(H):
    for (w, h, nf) in [(1241, 376, 2000), (1241, 376, 1000), (752, 480, 500), (640, 480, 10000)]:
        e = orbo.Extractor(nf)
        e.compute(synth.make_frame(w, h, seed=7 + w))
        q = e.tables()["quota"]
        for l in range(8):
            c = e.candidates(l)
            lw, lh = e.level(l).shape[::-1]
            xyr = np.stack([c["x"], c["y"], c["response"]], 1).astype(np.int32)
            r = host_octree(H, xyr, lw - 32, lh - 32, int(q[l]))
            o = orbo.distribute_octree(c, 16, lw - 16, 16, lh - 16, int(q[l]))
            O = np.stack([o["x"], o["y"], o["response"]], 1).astype(np.int32).reshape(-1, 3)
            assert np.array_equal(O, r), (w, h, nf, l)


@pytest.mark.parametrize("W,Hh", [(1209, 344), (1002, 281), (314, 73), (1888, 1048), (720, 448), (178, 102), (766, 766), (65, 40)])
def test_quadtree_path_tables_equal_the_literal_halvings(H, W, Hh):
    """k_octree_v4 finds a key's leaf of the implicit quadtree as xs[x] | ys[y] (vslam::build_oct_lut) instead of walking D
    halvings per key: every (x, y) of the level, depths 1..7, against DivideNode's arithmetic spelled out (oct_key_path)"""
    for D in range(1, 8):
        assert H.vslamh_oct_lut_check(W, Hh, D) == 0, D
    # the literal walk itself: two keys in the same leaf at depth d share every shallower leaf
    rng = np.random.default_rng(4)
    H.vslamh_oct_key_path.restype = C.c_uint
    for _ in range(200):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, Hh))
        prev = None
        for d in range(0, 13):
            pth = H.vslamh_oct_key_path(x, y, W, Hh, d)
            if prev is not None:
                assert pth >> 2 == prev
            prev = pth


def test_octree_random_and_edge_cases(H):
    rng = np.random.default_rng(9)
    assert len(host_octree(H, np.zeros((0, 3)), 1209, 344, 100)) == 0
    assert H.vslamh_octree(None, 0, 100, 400, 10, None, 0) == -1  # nIni == 0 (portrait): unsupported
    for trial in range(40):
        W, Hh = int(rng.integers(60, 1900)), int(rng.integers(40, 400))
        if round(W / Hh) < 1:
            continue
        n = int(rng.integers(1, 3000))
        N = int(rng.integers(1, 600))
        pts = np.unique(np.stack([rng.integers(0, W, n), rng.integers(0, Hh, n)], 1), axis=0)
        rng.shuffle(pts)
        # few distinct responses -> many ties: exercises first-wins and the equal-size node tie-break
        resp = rng.integers(7, 12 if trial % 2 else 250, len(pts))
        k = np.zeros(len(pts), orbo.KP_DTYPE)
        k["x"], k["y"], k["response"] = pts[:, 0], pts[:, 1], resp
        o = orbo.distribute_octree(k, 16, 16 + W, 16, 16 + Hh, N)
        O = np.stack([o["x"], o["y"], o["response"]], 1).astype(np.int32).reshape(-1, 3)
        r = host_octree(H, np.column_stack([pts, resp]), W, Hh, N)
        assert np.array_equal(O, r), trial


def test_grid_query_equals_oracle(H):
    e = orbo.Extractor(1000)
    k, d, _ = e.compute(synth.make_frame(1241, 376), lap=(0, 1000))
    rng = np.random.default_rng(3)
    for _ in range(50):
        x, y = float(rng.uniform(-50, 1300)), float(rng.uniform(-50, 420))
        r = float(rng.choice([10, 50, 100]))
        lv = int(rng.integers(-1, 3))
        want = orbo.grid_query(k, 1241, 376, x, y, r, max(lv, 0), lv)
        out = np.zeros(len(k) + 1, np.int32)
        n = H.vslamh_grid_query(_p(k), len(k), 1241, 376, C.c_float(x), C.c_float(y), C.c_float(r),
                                max(lv, 0), lv, _p(out), len(out))
        assert np.array_equal(out[:n], want)


def test_search_init_replay_equals_oracle(H):
    e = orbo.Extractor(1000)
    k1, d1, _ = e.compute(synth.make_frame(1241, 376, step=0), lap=(0, 1000))
    k2, d2, _ = e.compute(synth.make_frame(1241, 376, step=1), lap=(0, 1000))
    dm = np.minimum(orbo.hamming_matrix(d1, d2), 255).astype(np.uint8)
    for window, ratio, ori in [(100, 0.9, 1), (30, 0.9, 0), (100, 0.6, 1)]:
        nm_o, m_o, pm_o = orbo.search_for_initialization(k1, d1, k2, d2, 1241, 376, window=window,
                                                         nnratio=ratio, check_ori=bool(ori))
        pm = np.stack([k1["x"], k1["y"]], 1).astype(np.float32).copy()
        m = np.zeros(len(k1), np.int32)
        nm = H.vslamh_search_init(_p(k1), len(k1), _p(k2), len(k2), _p(dm), 1241, 376, _p(pm), _p(m), window,
                                  C.c_float(ratio), ori)
        assert nm == nm_o and np.array_equal(m, m_o) and np.array_equal(pm, pm_o)
        assert nm > 20


# ---------------------------------------------------------------- C ABI library (no GPU needed)
def _declared_functions(header="vslam_fe.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vslam_\w+)\s*\(", src)))


def test_header_and_python_mirror_agree():
    assert _declared_functions() == sorted(V.ABI_SYMBOLS)


def test_product_library_exports_every_declared_symbol():
    assert os.path.exists(V.LIB_PATH), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(V.LIB_PATH)
    for name in _declared_functions() + _declared_functions("vslam_fastgrid.h"):
        assert hasattr(L, name), name


def test_fastgrid_create_rejects_bad_parameters_and_has_no_cpu_fallback():
    """include/vslam_fastgrid.h: parameter checks mirror the reference's assertions (fast_gpu.cpp:75,
    detector_base_gpu.cpp:61-62, pyramid_pool.cpp:58-59); without a device the constructor fails."""
    import torch
    from vi_slam_amd import fastgrid
    assert _declared_functions("vslam_fastgrid.h") == sorted(
        ["vslam_fg_create", "vslam_fg_destroy", "vslam_fg_grid", "vslam_fg_detect", "vslam_fg_detect_batch",
         "vslam_fg_level_copy", "vslam_fg_response_copy"])
    for bad in (dict(cell_size_width=48), dict(min_arc_length=8), dict(min_arc_length=13), dict(max_level=0), dict(score=3),
                dict(max_level=3, image_width=130), dict(max_batch=0), dict(threshold=-1.0)):
        kw = dict(image_width=128, image_height=64)
        kw.update(bad)
        with pytest.raises(V.VslamError) as ei:
            fastgrid.FASTGPU(**kw)
        assert ei.value.code == V.ERR_INVALID
    if torch.cuda.device_count() == 0:
        with pytest.raises(V.VslamError):
            fastgrid.FASTGPU(128, 64)


def test_create_rejects_bad_parameters_and_missing_gpu():
    import torch
    L = V.lib()
    h = C.c_void_p()
    bad = V._Params(0, 376, 1000, 1.2, 8, 20, 7, 0, 1, 0, (C.c_int32 * 7)(*[0] * 7))
    assert L.vslam_fe_create(C.byref(bad), C.byref(h)) == V.ERR_INVALID and not h.value
    bad = V._Params(1241, 376, 1000, 1.2, 8, 20, 7, 0, 99, 0, (C.c_int32 * 7)(*[0] * 7))
    assert L.vslam_fe_create(C.byref(bad), C.byref(h)) == V.ERR_INVALID
    if torch.cuda.device_count() == 0:
        # no CPU fallback: without a device the product refuses to construct
        with pytest.raises(V.VslamError) as ei:
            V.FExtractor(1000, 1.2, 8, 20, 7, 1241, 376)
        assert ei.value.code == V.ERR_NO_DEVICE


@pytest.mark.parametrize("weighting,norm", [(0, 1), (0, 0), (1, 2), (2, 1), (3, 0)])
def test_bow_assemble_equals_dbow3_restatement(weighting, norm):
    """vslam_bow_assemble (host half of Frame::ComputeBoW, GPU-free) vs the oracle's restatement of
    DBoW3::Vocabulary::transform: BowVector / FeatureVector identical, doubles bit for bit."""
    import vi_slam_amd as V
    from oracle import orbo
    from vi_slam_amd import synth
    voc = synth.make_vocabulary(6, 3, seed=3, stop_fraction=0.1, weighting=weighting, norm=norm)
    rng = np.random.default_rng(5)
    leaves = np.nonzero(voc["child_count"] == 0)[0]
    d = voc["desc"][rng.choice(leaves, 400)].copy()
    for i in range(len(d)):
        for f in rng.integers(0, 256, 8):
            d[i, f >> 3] ^= np.uint8(1 << (f & 7))
    want = orbo.bow_transform(voc, d, 2)
    got = V.bow_assemble(weighting, norm, want["word"], want["weight"], want["nid"])
    for k in ("bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat"):
        assert np.array_equal(got[k], want[k]), k
    assert len(got["bow_ids"]) > 20 and (want["weight"] == 0).any()


def test_worker_pool_stress_under_thread_sanitizer(tmp_path):
    """The context's worker pool (vslam_pool.h): alternating small/large parallel_for calls with stack lambdas;
    every index runs exactly once and ThreadSanitizer reports nothing (stale-index race)."""
    import subprocess
    exe = str(tmp_path / "pool_stress")
    src = os.path.join(ROOT, "tests", "cpp", "pool_stress.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread", "-o", exe, src])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    env.pop("LD_PRELOAD", None)  # run_sanitizers.sh preloads ASan for the Python process; TSan cannot share a process with it
    r = subprocess.run([exe, "6000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pool_stress ok" in r.stdout and "WARNING: ThreadSanitizer" not in r.stderr


def test_owning_buffer_over_a_counting_space(tmp_path):
    """The owning buffer of vslam_mem.h (generic part, no HIP) over a space that records every live block, fails on
    demand and aborts on a free of a block that is not live: grow-only ensure, the failed allocation, move, swap,
    release twice, the zero-length upload, a vector of buffer-holding structs; nothing is live at exit."""
    import subprocess
    exe = str(tmp_path / "mem_owner")
    src = os.path.join(ROOT, "tests", "cpp", "mem_owner.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mem_owner ok" in r.stdout and "0 live" in r.stdout


@pytest.mark.parametrize("size,nlevels,scale", [((1241, 376), 8, 1.2), ((1920, 1080), 8, 1.2), ((752, 480), 8, 1.2),
                                                ((321, 203), 6, 1.2), ((640, 480), 5, 1.1), ((1241, 376), 12, 1.1),
                                                ((128, 128), 2, 1.2), ((500, 400), 4, 1.5)])
def test_fused_pyramid_plan_emulation_equals_oracle_cascade(H, size, nlevels, scale):
    """The tile plan of the fused pyramid kernel (k_pyramid_group: groups of levels computed in LDS with recomputed
    halos) evaluated on the CPU with the kernel's own indexing: every level equals the oracle's cv::resize cascade,
    no tile reads a byte that was neither staged nor computed, and the plan fits LDS."""
    w, h = size
    img = synth.make_frame(w, h, seed=w * 3 + nlevels)
    e = orbo.Extractor(500, scale=scale, nlevels=nlevels)
    e.pyramid_only(img)
    sizes = [e.level(l).shape for l in range(nlevels)]
    out = np.zeros(sum(a * b for a, b in sizes[1:]) + 16, np.uint8)
    lds, ntiles = C.c_int(), C.c_int()
    H.vslamh_pyramid_fused.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    ng = H.vslamh_pyramid_fused(_p(img), w, h, img.strides[0], 500, scale, nlevels, _p(out), C.byref(lds), C.byref(ntiles))
    assert ng == (0 if nlevels == 1 else 1 + max(0, (nlevels - 1 - 3 + 3) // 4)), ng
    assert 0 < lds.value <= 64 * 1024
    o = 0
    for l in range(1, nlevels):
        hh, ww = sizes[l]
        assert np.array_equal(out[o:o + hh * ww].reshape(hh, ww), e.level(l)), l
        o += hh * ww


# ---- what vslam_fe_create decides without a GPU call: keypoint capacity, the quadtree plan, the band tables
BENCH_GEOMS = [(1241, 376), (752, 480), (1920, 1080)]
OCT_NODE_BYTES = (56, 64)   # vk_octree_lds_bytes: 56 bytes a node + 64 (vslam_octree_kernel.hip)
OCT_BUDGET = 128 * 1024     # vslam_tuning.oct_lds_budget_kb's default
# fe->oct of the PARENT of the change that moved the plan to the host side (its create_impl arithmetic compiled on its own),
# at the six bench workloads' (width, height, nfeatures): fine depth per level, maxNodes, selStride, keypoint capacity
PARENT_OCT = {
    (1241, 376, 1000): ([4, 4, 4, 4, 4, 4, 4, 3], 224, 1032, 1040),   # kitti00_mono n1000
    (1241, 376, 2000): ([5, 5, 5, 4, 4, 4, 4, 4], 448, 2032, 2040),   # kitti00_mono n2000, kitti00_stereo, kitti00_stereo_track
    (1920, 1080, 4000): ([6, 6, 6, 5, 5, 5, 5, 5], 880, 4032, 4040),  # synthetic_stereo
    (752, 480, 1200): ([5, 5, 5, 5, 4, 4, 4, 4], 272, 1232, 1240),    # hut_stereo
}
# and its band list: (bands, column classes, tallest window, widest interior, most cells of a band)
PARENT_BANDS = {(1241, 376): (323, 10, 46, 128, 4), (752, 480): (263, 12, 40, 128, 4), (1920, 1080): (1625, 10, 40, 128, 4)}


def _context_geometry(H, w, h, nf, nlevels=8):
    """what vslam_fe_create hands the planners: quotas, level sizes, the cell list of all levels and each level's first cell"""
    sf, isf, s2, is2 = (np.zeros(nlevels, np.float32) for _ in range(4))
    quota, um, dn = np.zeros(nlevels, np.int32), np.zeros(16, np.int32), C.c_int()
    H.vslamh_tables(nf, C.c_float(1.2), nlevels, _p(sf), _p(isf), _p(s2), _p(is2), _p(quota), _p(um), C.byref(dn))
    lw, lh, first, cells = np.zeros(nlevels, np.int32), np.zeros(nlevels, np.int32), np.zeros(nlevels + 1, np.int32), []
    for l in range(nlevels):
        a, b = C.c_int(), C.c_int()
        H.vslamh_level_size(nf, C.c_float(1.2), nlevels, w, h, l, C.byref(a), C.byref(b))
        lw[l], lh[l] = a.value, b.value
        buf = np.zeros((8192, 5), np.uint16)
        nc = H.vslamh_cells(l, a.value, b.value, _p(buf), 8192)
        assert 0 < nc <= 8192
        cells.append(buf[:nc])
        first[l + 1] = first[l] + nc
    return quota, lw, lh, first, np.ascontiguousarray(np.concatenate(cells))


def _oct_plan(H, w, h, nf, forced=-1, budget=OCT_BUDGET):
    quota, lw, lh, first, _ = _context_geometry(H, w, h, nf)
    ctx, lvl = np.zeros(6, np.int32), np.zeros((8, 4), np.int32)
    assert H.vslamh_oct_plan(_p(quota), _p(lw), _p(lh), _p(first), 8, forced, budget, OCT_NODE_BYTES[0], OCT_NODE_BYTES[1],
                             _p(ctx), _p(lvl)) == 0
    cap = H.vslamh_keypoint_capacity(_p(quota), _p(lw), _p(lh), 8, nf)
    return [int(v) for v in ctx], lvl.astype(int), (quota.astype(int), lw.astype(int), lh.astype(int)), cap


def test_quadtree_plan_invariants_and_parent_values(H):
    for (w, h) in BENCH_GEOMS:
        for nf in (500, 1000, 2000, 4000, 20000):
            for forced in (-1, 1, 3):
                (maxNodes, selStride, ldsOff, ldsBytes, fits, lut_bad), lvl, (quota, lws, lhs), cap = _oct_plan(H, w, h, nf, forced)
                tag = (w, h, nf, forced)
                assert lut_bad == 0, tag  # every (x, y) of every level: table path == oct_key_path at the level's depth
                assert maxNodes % 16 == 0 and ldsOff % 16 == 0 and ldsOff >= OCT_NODE_BYTES[0] * maxNodes + OCT_NODE_BYTES[1], tag
                assert not fits or ldsOff + ldsBytes <= OCT_BUDGET, tag
                assert not fits or (ldsOff + ldsBytes <= 160 * 1024 and ldsOff <= 150 * 1024 + 16), tag
                assert fits == (nf <= 4000), tag  # 20000 features: level 0's node list alone is 238 KB
                off = 0
                for l in range(8):
                    nIni, selOff, D, lutW = lvl[l]
                    assert nIni == int(np.float32(lws[l] - 32) / np.float32(lhs[l] - 32) + np.float32(0.5)) >= 1, tag
                    cap_l = max(quota[l] + 3, 4 * nIni) + 1  # what DistributeOctTree can leave on the level, + 1
                    assert selOff == off and cap_l <= maxNodes and lutW == lws[l] - 32 + 1, tag
                    off += cap_l
                    assert 1 <= D <= 11 and nIni << (2 * D) <= 16384, (tag, l)
                    assert 2 * ((nIni << (2 * D)) + 1) * 4 + 16 <= ldsBytes, (tag, l)
                    if forced >= 0 and fits:
                        assert D == forced, (tag, l)  # admissible at these sizes
                assert off == selStride and cap >= max(selStride - 8, nf + 40) and cap % 4 == 0, tag
    for (w, h, nf), (D, maxNodes, selStride, cap) in PARENT_OCT.items():
        ctx, lvl, _, got_cap = _oct_plan(H, w, h, nf)
        assert list(lvl[:, 2]) == D and ctx[0] == maxNodes and ctx[1] == selStride and ctx[4] == 1, (w, h, nf)
        assert got_cap == cap, (w, h, nf)
    # tiny quota: the exact DistributeOctTree bound exceeds nfeatures + 4 * nlevels + 8
    assert _oct_plan(H, 1241, 376, 10)[3] > (10 + 32 + 8 + 3) & ~3


def test_band_tables_encode_the_bands(H):
    for (w, h) in BENCH_GEOMS:
        for per in (4, 2):
            cells16 = _context_geometry(H, w, h, 1000)[4]
            cells = cells16.astype(int)
            words, classes, info = np.zeros((4096, 4), np.uint32), np.zeros(64 * 272, np.uint8), np.zeros(5, np.int32)
            nb = H.vslamh_band_tables(_p(cells16), len(cells16), 8, per, 128, _p(words), 4096, _p(classes), len(classes), _p(info))
            assert nb > 0 and info[4] == 1
            if per == 4:
                assert (nb,) + tuple(int(v) for v in info[:4]) == PARENT_BANDS[(w, h)]
            words = words[:nb].astype(int)
            ncls = int(info[0])
            seen = np.zeros(len(cells), int)
            assert np.all(np.diff(words[:, 0]) > 0)
            for cell0, lnw, xy, wh in words:
                lev, ncell, wcell, ci = lnw & 15, (lnw >> 4) & 15, (lnw >> 8) & 255, lnw >> 16
                x0, y0, ww, bh = xy & 0xFFFF, xy >> 16, wh & 0xFFFF, wh >> 16
                assert 1 <= ncell <= per and bh <= info[1]
                assert ci < ncls
                bit, fl = classes[ci * 272:ci * 272 + 136].astype(int), classes[ci * 272 + 136:ci * 272 + 272].astype(int)
                iw = ww - 6
                assert iw <= info[2] <= 128 and not bit[iw:].any() and not fl[iw:].any()
                want_fl = np.zeros(iw, int)
                for k in range(ncell):
                    c = cells[cell0 + k]  # (level, x0, y0, x1, y1): interior columns x0 + 3 .. x1 - 4 of the level
                    assert c[0] == lev and (c[1], c[2], c[4]) == (x0 + k * wcell, y0, y0 + bh)  # the cell build_bands put there
                    a, b = c[1] - x0, c[3] - 6 - x0  # ... are the band's interior columns [a, b)
                    assert 0 <= a < b <= iw and np.all(bit[a:b] == 1 << k), (w, h, cell0, k)
                    want_fl[a] |= 1
                    want_fl[b - 1] |= 2
                    seen[cell0 + k] += 1
                assert np.array_equal(fl[:iw], want_fl) and np.all(bit[:iw] != 0)
            assert np.all(seen == 1)


# ---- the carving of a staging block (vslam::layout_parts, vslam_staging.h) ----
def _layout(H, align, sizes):
    H.vslamh_layout.restype = C.c_uint64
    H.vslamh_layout.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
    s = np.asarray(sizes, np.uint64)
    off = np.zeros(len(s), np.uint64)
    total = H.vslamh_layout(align, _p(s), len(s), _p(off))
    return [int(o) for o in off], int(total)


def test_staging_layout_properties(H):
    rng = np.random.default_rng(7)
    assert _layout(H, 16, []) == ([], 0)
    for align in (16, 256):
        for _ in range(300):
            n = int(rng.integers(1, 20))
            sizes = [int(v) for v in rng.integers(0, 5000, n) * (rng.random(n) > 0.3)]
            if rng.random() < 0.2:
                sizes[int(rng.integers(n))] = int(rng.integers(1 << 20, 1 << 33))
            off, total = _layout(H, align, sizes)
            assert off[0] == 0 and all(o % align == 0 for o in off) and total % align == 0
            assert all(a <= b for a, b in zip(off, off[1:]))
            assert all(off[i] + sizes[i] <= off[i + 1] for i in range(n - 1))
            assert off[-1] + sizes[-1] <= total < off[-1] + sizes[-1] + align
            # a part of no bytes takes no room, and no part takes more than its size rounded up
            assert all(off[i + 1] - off[i] < sizes[i] + align for i in range(n - 1))
            assert all(off[i + 1] == off[i] for i in range(n - 1) if sizes[i] == 0)


SZ_KP, SZ_MAP_POINT, SZ_MP_TRACK = V.KP_DTYPE.itemsize, V.MAP_POINT_DTYPE.itemsize, V.MP_TRACK_DTYPE.itemsize
SBP_M = 8


def _sbp_scratch(n):  # vk_sbp_scratch_bytes: an SbpProj (32 bytes) and M candidate words per point
    return n * (32 + 4 * SBP_M)


def _parent_sbp_frame(n_last, n_cur, kf, normals):
    """The offset chain sbp_frame_impl had before vslam::layout, restated."""
    def al(v):
        return (v + 15) & ~15
    o_kps = 0
    o_x = al(o_kps + n_last * SZ_KP)
    o_d = al(o_x + n_last * 12)
    o_f = al(o_d + n_last * 32)
    o_u = al(o_f + n_last)
    o_o = al(o_u + n_cur * 4)
    o_mn = al(o_o + n_cur)
    o_mx = al(o_mn + (n_last * 4 if kf else 0))
    o_nr = al(o_mx + (n_last * 4 if kf else 0))
    in_bytes = al(o_nr + (n_last * 12 if (kf and normals) else 0))
    o_scr = in_bytes
    o_m = al(o_scr + _sbp_scratch(n_last))
    o_n = al(o_m + n_cur * 4)
    return [o_kps, o_x, o_d, o_f, o_u, o_o, o_mn, o_mx, o_nr, o_scr, o_m, o_n], o_n + 16


def _parent_local_points(n_mp, n_cur, from_host):
    """The offset chain vslam_search_local_points_async had before vslam::layout, restated."""
    def al(v):
        return (v + 255) & ~255
    cap, nchunks = min(n_mp, 4096), (n_mp + 255) // 256  # VSLAM_FRUSTUM_MAX_KEPT, VSLAM_FRUSTUM_CHUNK
    o_u = 0
    o_o = o_u + al(n_cur * 4)
    o_pts = o_o + al(n_cur)
    o_desc = o_pts + (al(n_mp * SZ_MAP_POINT) if from_host else 0)
    in_bytes = o_desc + (al(n_mp * 32) if from_host else 0)
    o_track = in_bytes
    o_depth = o_track + al(n_mp * SZ_MP_TRACK)
    o_cv = o_depth + al(n_mp * 4)
    o_ck = o_cv + al(nchunks * 4)
    o_tc = o_ck + al(nchunks * 4)
    o_dc = o_tc + al(cap * SZ_MP_TRACK)
    o_fc = o_dc + al(cap * 32)
    o_scr = o_fc + al(cap)
    o_m = o_scr + al(_sbp_scratch(cap))
    o_cnt = o_m + al(n_cur * 4)
    o_idx = o_cnt + 256
    total = o_idx + al(cap * 4)
    return [o_u, o_o, o_pts, o_desc, o_track, o_depth, o_cv, o_ck, o_tc, o_dc, o_fc, o_scr, o_m, o_cnt, o_idx], total


STAGING_N = (1, 3, 15, 16, 17, 4096)


def test_staging_layout_equals_parent_chain_of_search_by_projection_frame(H):
    for n_last in STAGING_N:
        for n_cur in STAGING_N:
            for kf, normals in ((False, False), (True, False), (True, True)):
                kfn = n_last if kf else 0
                sizes = [n_last * SZ_KP, n_last * 12, n_last * 32, n_last, n_cur * 4, n_cur, kfn * 4, kfn * 4,
                         n_last * 12 if (kf and normals) else 0, _sbp_scratch(n_last), n_cur * 4, 16]
                assert _layout(H, 16, sizes) == _parent_sbp_frame(n_last, n_cur, kf, normals), (n_last, n_cur, kf, normals)


def test_staging_layout_equals_parent_chain_of_search_local_points(H):
    for n_mp in (1, 255, 256, 257, 65536):
        for n_cur in STAGING_N:
            for from_host in (True, False):
                cap, nchunks, host_mp = min(n_mp, 4096), (n_mp + 255) // 256, n_mp if from_host else 0
                sizes = [n_cur * 4, n_cur, host_mp * SZ_MAP_POINT, host_mp * 32, n_mp * SZ_MP_TRACK, n_mp * 4, nchunks * 4,
                         nchunks * 4, cap * SZ_MP_TRACK, cap * 32, cap, _sbp_scratch(cap), n_cur * 4, 256, cap * 4]
                assert _layout(H, 256, sizes) == _parent_local_points(n_mp, n_cur, from_host), (n_mp, n_cur, from_host)

