"""Vocabulary::create / save without a GPU: the host twin (vslamh_voc_train in libvslam_host.so) against the numpy
yardstick tests/voc_train_ref.py on every case of tests/voc_train_cases.py, the preconditions of those cases, and
vslam_voc_file_save against the writer of tests/vocfile.py.  Everything is integer arithmetic or a libm double: every
comparison is exact, weights as uint64."""
import ctypes as C
import math

import numpy as np
import pytest

import vi_slam_amd as V

import voc_train_cases as cases
import voc_train_ref as ref
import vocfile


@pytest.fixture(scope="module")
def H():
    return V.host_lib()


def twin(H, name, **override):
    desc, off, kw = cases.inputs(name)
    return V.train_vocabulary(desc, off, library=H, **dict(kw, **override))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_twin_equals_the_yardstick(H, name):
    want = cases.expected(name)
    got = twin(H, name)
    ref.assert_same(got, want, name)
    assert got["format"] == "trained" and got["norm"] == 1
    assert got["stats"]["hit_max_iter"] == 0 and want["stats"]["hit_max_iter"] == 0   # the bound hides nothing


def test_case_list_reaches_every_branch():
    """precondition: the yardstick alone takes every counted branch on the case list, and the cases the issue names
    reach what they are there for"""
    st = {name: cases.expected(name)["stats"] for name in cases.CASES}
    for key in ("early_stops", "redraws", "small_nodes", "single_leaves", "empty_groups"):
        assert any(s[key] > 0 for s in st.values()), key
    assert st["rand3000"]["max_passes"] >= 10                      # long Lloyd loops
    assert st["clu3000"]["empty_groups"] > 0
    assert st["clu4000_k35"]["empty_groups"] > 0 and st["clu4000_k35"]["early_stops"] == 0
    assert st["dups600"]["early_stops"] > 0
    assert st["rand500_deep"]["small_nodes"] > 0 and st["rand500_deep"]["single_leaves"] > 0
    assert st["rand500_deep"]["deepest_level"] == 5
    assert st["mix900_mask3"]["redraws"] > 0 and st["mix900"]["redraws"] == 0
    for key in ("early_stops", "small_nodes", "single_leaves", "empty_groups"):
        assert st["mix900"][key] > 0, key
    assert st["clu70000"]["max_passes"] >= 3
    # a leaf above level L: a child that did not recurse
    voc = cases.expected("rand500_deep")
    leaves = np.flatnonzero(voc["child_count"][1:] == 0) + 1
    assert (voc["level"][leaves] < voc["L"]).any()
    # ties: some feature of the duplicates case is equally near to two centres of its node
    assert cases.expected("dups600")["n_words"] < 6 ** 3


def test_dist_sum_is_exact_in_float64():
    """the claim that frees the summation order: every dist_sum of mix900's seedings, summed in float64, is the integer"""
    sums = cases.expected("mix900")["dist_sums"]
    assert len(sums) > 10
    for node in sums:
        for as_int, as_double in node:
            assert as_double == float(as_int) and int(as_double) == as_int and as_int < 2 ** 53


def test_max_iter_bound(H):
    name, bound = cases.MAX_ITER_CASE, cases.MAX_ITER_BOUND
    want = cases.expected(name, max_iter=bound)
    got = twin(H, name, max_iter=bound)
    ref.assert_same(got, want, name)
    assert got["stats"]["hit_max_iter"] > 0 and got["stats"]["max_passes"] == bound
    assert not np.array_equal(want["desc"], cases.expected(name)["desc"])   # the bound changed the tree


def test_other_weightings_and_scoring(H):
    desc, off, kw = cases.inputs("mix900")
    for weighting, scoring in ((1, 1), (2, 5), (3, 0)):
        kw2 = dict(kw, weighting=weighting, scoring=scoring)
        got = V.train_vocabulary(desc, off, library=H, **kw2)
        ref.assert_same(got, ref.train(desc, off, **kw2), "weighting %d" % weighting)
        assert got["norm"] == {1: 2, 5: 0, 0: 1}[scoring]
    leaves = got["child_count"][1:] == 0
    assert np.array_equal(got["weight"][1:][leaves], np.ones(int(leaves.sum())))   # BINARY: weight 1


def test_weights_are_log_of_document_ratios():
    voc = cases.expected("clu3000")
    w = voc["weight"][voc["weight"] != 0]
    assert len(w) and all(any(x == math.log(13.0 / ni) for ni in range(1, 13)) for x in w)


def test_node_order_is_the_order_of_the_recursion(H):
    got = twin(H, "mix900")
    kids = {i: vocfile.children(got, i) for i in range(len(got["child_start"]))}
    order = ref.simulate_node_order(kids)
    assert all(order[i] == i for i in kids)
    # neither breadth-first nor preorder: some node has a smaller id than a node of a shallower level
    level = cases.expected("mix900")["level"]
    assert (np.diff(level) < 0).any() and not np.array_equal(np.sort(level), level)
    first_inner = next(c for c in kids[0] if kids[c])
    assert kids[first_inner][0] == len(kids[0]) + 1   # children of the root's first inner child follow the root's block


def test_save_writes_the_stream_of_the_reference(tmp_path, H):
    for name in ("mix900", "tiny1"):
        got = twin(H, name, scoring=1)
        path = str(tmp_path / (name + ".dbow3"))
        V.save_vocabulary_file(got, path, library=H)
        with open(path, "rb") as f:
            data = f.read()
        assert data == vocfile.binary_bytes(got, compressed=False, scoring=1)
        back = V.read_vocabulary_file(path, H)
        assert back["format"] == "dbow3-binary" and back["scoring"] == 1 and back["norm"] == 2
        for key in ref.TABLE_KEYS:
            assert np.array_equal(back[key], got[key]), key
        assert np.array_equal(back["weight"].view(np.uint64), got["weight"].view(np.uint64))


def test_save_of_a_loaded_file(tmp_path, H):
    """tools/convertVoc: a text vocabulary re-saved as the binary stream"""
    from vi_slam_amd import synth
    voc = synth.make_vocabulary(4, 3, seed=9, weighting=0)
    src, dst = str(tmp_path / "voc.txt"), str(tmp_path / "voc.dbow3")
    vocfile.write_text(src, voc)
    loaded = V.read_vocabulary_file(src, H)
    V.save_vocabulary_file(loaded, dst, library=H)
    with open(dst, "rb") as f:
        assert f.read() == vocfile.binary_bytes(loaded, compressed=False)


def _raw_train(H, k=4, L=2, weighting=0, scoring=0, rand_mask=0x7fffffff, max_iter=0, offsets=(0, 3, 6), desc=True):
    P = V._VocTrainParams(k, L, weighting, scoring, 1, rand_mask, max_iter)
    off = np.array(offsets, np.int64)
    d = np.zeros((8, 32), np.uint8)
    h = C.c_void_p()
    rc = H.vslamh_voc_train(C.byref(P), V._p(d) if desc else None, V._p(off), len(off) - 1, C.byref(h), None)
    if h:
        H.vslam_voc_file_close(h)
    return rc


def test_invalid_parameters(H):
    assert _raw_train(H) == V.VSLAM_OK
    for bad in (dict(k=1), dict(k=65), dict(L=0), dict(L=11), dict(weighting=4), dict(weighting=-1), dict(scoring=6),
                dict(rand_mask=0), dict(rand_mask=0x80000000), dict(max_iter=-1), dict(offsets=(0, 4, 3)),
                dict(offsets=(1, 3)), dict(offsets=(0, 0)), dict(offsets=(0,)), dict(desc=False)):
        assert _raw_train(H, **bad) == V.ERR_INVALID, bad
    assert b"" != H.vslam_voc_file_last_error()
    with pytest.raises(V.VslamError):
        V.train_vocabulary(np.zeros((2, 32), np.uint8), [0, 3], 4, 2, library=H)   # fewer rows than the offsets claim
