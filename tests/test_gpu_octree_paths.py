"""GPU (-m gpu): the paths of k_octree_v4 -- one key walk with the best key per fine cell, the sort that only a problem
below the grid builds, the passes' ways to stop, ties inside a node -- each against oracle.orbo.Extractor: keypoints in
order and descriptors of every slot.  Contexts of four images run the 256-thread batch kernel; the fourth slot holds another
image than the first three."""
import os

import numpy as np
import pytest

import vi_slam_amd as V
from oracle import orbo
from vi_slam_amd import synth

import octree_paths_cases as oc

pytestmark = pytest.mark.gpu


def _same_feats(res, ref, tag=""):
    k, d = res[0], res[1]
    ko, do = ref[0], ref[1]
    assert len(k) == len(ko), tag
    for f in k.dtype.names:
        assert np.array_equal(k[f], ko[f]), (tag, f)
    assert np.array_equal(d, do), tag


def _batch_of_four_equals_oracle(a, b, nf, tag):
    """slots [a, a, a, b] through one context of four; -> octree_stats() of the pass"""
    h, w = a.shape
    ref = {}
    for name, im in (("a", a), ("b", b)):
        ko, do, _ = orbo.Extractor(nf).compute(im)
        ref[name] = (ko, do)
    fe = V.FExtractor(nf, 1.2, 8, 20, 7, w, h, max_batch=4)
    try:
        res = fe.compute_batch([a, a, a, b])
        stats = fe.octree_stats()
        for s in range(4):
            _same_feats(res[s], ref["b" if s == 3 else "a"], "%s N=%d slot %d" % (tag, nf, s))
    finally:
        fe.close()
    return stats


@pytest.fixture(scope="module")
def hut(golden_dir):
    g = np.load(os.path.join(golden_dir, "pipeline_hut_320x240.npz"))
    return np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])


def test_real_frame_with_final_nodes_below_the_grid(hut):
    """At N = 500 the oracle ends with two selected keys inside one cell of the fine grid on a top level of either image:
    final nodes deeper than the grid, so those problems sort their keys on demand while the others of the launch do not."""
    L, R = hut
    below_l, below_r = oc.levels_below_grid(L, 500), oc.levels_below_grid(R, 500)
    assert below_l and below_r, (below_l, below_r)
    prob, deep, masks = _batch_of_four_equals_oracle(L, R, 500, "hut")
    assert prob == 32
    for l in below_l:
        assert all(masks[s] >> l & 1 for s in range(3)), (l, masks[:4])
    for l in below_r:
        assert masks[3] >> l & 1, (l, masks[:4])


def test_real_frame_one_image_context(hut):
    """the same frames through a context of one image: the 1024-thread workgroup"""
    fe = V.FExtractor(500, 1.2, 8, 20, 7, 320, 240, max_batch=1)
    try:
        for im, tag in zip(hut, "LR"):
            k, d, _ = fe.compute(im)
            ko, do, _ = orbo.Extractor(500).compute(im)
            _same_feats((k, d), (ko, do), "hut %s, one image" % tag)
    finally:
        fe.close()


def test_dots_inside_one_fine_cell():
    """Six dots three pixels apart on a flat frame, N = 100: on every level all candidates lie in ONE fine cell (or there is
    one, or none), the only split leaves one child and the passes stop on size == size0 with the list far below its quota."""
    a = oc.clustered_dots(at=(115, 90))
    b = oc.clustered_dots(at=(200, 140))  # the fourth slot: one cell on the bottom levels, two on level 3
    ncand = [len(c) for c in oc.level_candidates(a, 100)]
    assert max(oc.candidate_cells(a, 100)) == 1 and ncand[0] > 1 and min(ncand) == 0 and 1 in ncand, ncand
    assert oc.candidate_cells(b, 100)[:3] == [1, 1, 1]
    _batch_of_four_equals_oracle(a, b, 100, "dots")


@pytest.mark.parametrize("nf", [300, 1500])
def test_quota_reached_by_the_cut_and_never_reached(nf):
    """synth.make_frame(320, 240): with N = 300 every level has several times its quota of candidates and phase 2 cuts the
    list at the quota; with N = 1500 the top levels hold fewer candidates than their quota, every node is split down to
    single keys and the passes end on an unchanged list."""
    a, b = synth.make_frame(320, 240), synth.make_frame(320, 240, step=1)
    e = orbo.Extractor(nf)
    e.compute(a)
    quota = [int(q) for q in e.tables()["quota"]]
    ncand = [len(e.candidates(l)) for l in range(8)]
    nsel = [len(e.level_keys(l)) for l in range(8)]
    if nf == 300:
        # every level: candidates to spare, and the list stopped AT the quota: at least N nodes, and fewer than the N + 3 that
        # one more whole split could leave, which is what the cut inside phase 2's sorted walk gives (fextractor.cpp:664-729)
        assert all(n > 2 * q for n, q in zip(ncand, quota)), (ncand, quota)
        assert all(q <= s <= q + 2 for s, q in zip(nsel, quota)), (nsel, quota)
    else:
        # the two top levels: fewer candidates than the quota, and every one of them selected (nodes of single keys);
        # the levels below still reach their quota
        assert all(ncand[l] < quota[l] and nsel[l] == ncand[l] for l in (6, 7)), (ncand, nsel, quota)
        assert all(quota[l] <= nsel[l] <= quota[l] + 2 for l in range(5)), (nsel, quota)
    _batch_of_four_equals_oracle(a, b, nf, "synth")


def test_equal_responses_inside_a_node():
    """A periodic checkerboard: the same corner all over a level, so many candidates share a response.  On the levels
    named by tie_levels the oracle's winner of some final node has a LATER candidate of the same response in that node:
    "first key in order wins" decided, which the kernel expresses as the smaller position in the cell's best key."""
    a, b = oc.checker(10), np.ascontiguousarray(oc.checker(10)[:, ::-1])
    ties = oc.tie_levels(a, 300)
    assert len(ties) >= 3 and oc.tie_levels(b, 300), ties
    _batch_of_four_equals_oracle(a, b, 300, "checker")
