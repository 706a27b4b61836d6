"""Vocabulary::create on the device (vslam_voc_train) against the numpy yardstick tests/voc_train_ref.py -- never
against itself -- on every case of tests/voc_train_cases.py, from host memory and from HBM; then the whole loop on real
pixels: extract, train from the slots' descriptors, save, load, ComputeBoW.  Every comparison is exact."""
import os

import numpy as np
import pytest

import vi_slam_amd as V
from oracle import orbo

import voc_train_cases as cases
import voc_train_ref as ref

pytestmark = pytest.mark.gpu


class _DevView:
    """n bytes of device memory at ptr, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="|u1", data=(int(ptr), False), version=2)


def dev_bytes(ptr, n):
    import torch
    return torch.as_tensor(_DevView(ptr, n), device="cuda")


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_equals_the_yardstick(name, where):
    """clu70000: 274 chunks of the 256-position seeding / partition kernels and 69 of the 1024-position mean kernel, so
    the root segment and every level-2 segment (about 8750 features) span many workgroups; the deep cases put many nodes
    under one workgroup"""
    desc, off, kw = cases.inputs(name)
    want = cases.expected(name)
    if where == "hbm":
        import torch
        d = torch.from_numpy(np.array(desc)).cuda()
        torch.cuda.synchronize()
        got = V.train_vocabulary(d, off, **kw)
    else:
        got = V.train_vocabulary(desc, off, **kw)
    ref.assert_same(got, want, "%s from %s" % (name, where))
    assert got["format"] == "trained" and got["stats"]["hit_max_iter"] == 0
    assert got["stats"]["ms_total"] > 0


def test_max_iter_bound():
    name, bound = cases.MAX_ITER_CASE, cases.MAX_ITER_BOUND
    desc, off, kw = cases.inputs(name)
    got = V.train_vocabulary(desc, off, **dict(kw, max_iter=bound))
    ref.assert_same(got, cases.expected(name, max_iter=bound), name)
    assert got["stats"]["hit_max_iter"] > 0 and got["stats"]["max_passes"] == bound


def test_other_weightings():
    desc, off, kw = cases.inputs("mix900")
    for weighting, scoring in ((1, 1), (2, 5), (3, 0)):
        kw2 = dict(kw, weighting=weighting, scoring=scoring)
        ref.assert_same(V.train_vocabulary(desc, off, **kw2), ref.train(desc, off, **kw2), "weighting %d" % weighting)


def test_seeds():
    desc, off, kw = cases.inputs("clu3000")
    a = V.train_vocabulary(desc, off, **kw)
    b = V.train_vocabulary(desc, off, **kw)
    c = V.train_vocabulary(desc, off, **dict(kw, seed=cases.SEED + 1))
    for key in ref.TABLE_KEYS + ("weight",):
        assert np.array_equal(a[key], b[key]), key
    assert a["desc"].shape != c["desc"].shape or not np.array_equal(a["desc"], c["desc"])
    ref.assert_same(a, cases.expected("clu3000"), "clu3000")


def test_invalid_arguments_launch_nothing():
    d = np.zeros((8, 32), np.uint8)
    for bad in (dict(k=1), dict(k=65), dict(L=0), dict(L=11), dict(weighting=4), dict(scoring=6), dict(rand_mask=0),
                dict(max_iter=-1)):
        with pytest.raises(V.VslamError) as e:
            V.train_vocabulary(d, [0, 4, 8], **dict(dict(k=4, L=2), **bad))
        assert e.value.code == V.ERR_INVALID, bad
    for off in ([0, 5, 4], [1, 8], [0, 0]):
        with pytest.raises(V.VslamError) as e:
            V.train_vocabulary(d, off, 4, 2)
        assert e.value.code == V.ERR_INVALID, off


def test_uploaded_tree_transforms_the_training_set():
    """vslam_voc_file_upload + vslam_bow_transform over the training descriptors: the yardstick's word of every feature"""
    import torch
    desc, off, kw = cases.inputs("mix900")
    want = cases.expected("mix900")
    fe = V.FExtractor(300, 1.2, 8, 20, 7, 320, 240, device=0, max_batch=1)
    d = torch.from_numpy(np.array(desc)).cuda()
    torch.cuda.synchronize()
    vv = V.Vocabulary.from_trained(d, off, **kw)
    try:
        ref.assert_same(vv.trained, want, "mix900")
        assert (vv.L, vv.weighting, vv.norm, vv.n_nodes) == (4, 0, 1, len(want["child_start"]))
        got = vv.transform(fe, d.data_ptr(), len(desc), 2)
        assert np.array_equal(got["word"], want["word_of"])
        leaves = np.flatnonzero(want["child_count"][1:] == 0) + 1          # word w is the w-th leaf in node-id order
        assert np.array_equal(got["weight"].view(np.uint64), want["weight"][leaves[want["word_of"]]].view(np.uint64))
    finally:
        vv.close()
        fe.close()


def test_real_pixels_extract_train_save_load_compute_bow(tmp_path, golden_dir):
    """the loop the feature closes: the hut frames -> ORB descriptors in HBM -> Vocabulary::create (k = 5, L = 3, one
    document per frame) -> save -> Vocabulary::load -> ComputeBoW of one frame == the oracle's transform over the table"""
    import torch
    z = np.load(os.path.join(golden_dir, "real_images.npz"))
    names = sorted(n for n in z.files if n.startswith("hut"))
    assert len(names) >= 2
    ims = [z[n] for n in names]
    fe = V.FExtractor(1000, 1.2, 8, 20, 7, 752, 480, device=0, max_batch=len(ims))
    try:
        res = fe.compute_batch(ims)
        parts, off = [], [0]
        for s in range(len(ims)):
            _, pd, n = fe.slot_buffers(s)
            assert n == len(res[s][0]) > 500
            parts.append(dev_bytes(pd, n * 32))
            off.append(off[-1] + n)
        d = torch.cat(parts)                      # one N x 32 block in HBM, document d = frame d
        torch.cuda.synchronize()
        host = np.concatenate([res[s][1] for s in range(len(ims))])
        assert np.array_equal(d.cpu().numpy().reshape(-1, 32), host)
        voc = V.train_vocabulary(d, off, k=5, L=3, seed=7)
        ref.assert_same(voc, ref.train(host, off, 5, 3, seed=7), "hut frames")
        assert voc["n_words"] > 60 and voc["stats"]["deepest_level"] == 3
        path = str(tmp_path / "hut.dbow3")
        V.save_vocabulary_file(voc, path)
        vv = V.Vocabulary.load(path)
        try:
            assert (vv.L, vv.weighting, vv.norm, vv.n_nodes) == (3, 0, 1, len(voc["child_start"]))
            _, pd, n = fe.slot_buffers(1)
            got = vv.transform(fe, pd, n, 2)
            want = orbo.bow_transform(voc, res[1][1], 2)
            for key in ("word", "weight", "nid", "bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat"):
                assert np.array_equal(got[key], want[key]), key
            # a word seen in every frame weighs log(1) = 0 and stays out of the BowVector (Vocabulary.cpp:807)
            assert len(np.unique(got["word"])) > 30 and 0 < len(got["bow_ids"]) <= len(np.unique(got["word"]))
        finally:
            vv.close()
    finally:
        fe.close()
