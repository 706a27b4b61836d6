"""The one stage-by-stage comparison of the HIP extractor with the CPU oracle: pyramid level, blurred level and FAST
candidate list of every level of every used slot, then keypoints, descriptors and mono index.  Used by
tests/test_gpu_stages.py and tests/tools/gpu_check_extract.py.  Everything is compared with array_equal."""
import numpy as np

from oracle import orbo


class Reference:
    """what the oracle computes for one image, read-only: pyramid[l], blurred[l], candidates[l], (keypoints, descriptors,
    mono index).  compute() blurs only the levels that keep a keypoint (fextractor.cpp:1078); the device blurs every level,
    so the others are blurred here by the same oracle function (orbo.blur7 = gaussian_blur7) with the same taps."""

    def __init__(self, e, img, taps=None, lap=(0, 0)):
        self.result = e.compute(img, lap=lap)
        self.pyramid, self.blurred, self.candidates = [], [], []
        for l in range(e.nlevels):
            lv = e.level(l)
            bl = e.level(l, blurred=True)
            if bl is None:
                bl = orbo.blur7(lv, taps)
            ca = e.candidates(l).copy()
            for a in (lv, bl, ca):
                a.setflags(write=False)
            self.pyramid.append(lv)
            self.blurred.append(bl)
            self.candidates.append(ca)
        for a in self.result[:2]:
            a.setflags(write=False)


def _image_difference(got, want):
    if got.shape != want.shape:
        return "shape %s instead of %s" % (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    r, c = (int(v) for v in bad[0])
    return "%d bytes differ, first at (row %d, column %d): %d instead of %d; rows %d..%d, columns %d..%d" % (
        len(bad), r, c, got[r, c], want[r, c], bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


def stage_differences(fe, results, refs, tag=""):
    """fe: the context after compute_batch; results: what compute_batch returned; refs: one Reference per used slot.
    -> list of messages, each naming slot, level and stage; empty if every stage of every slot equals the oracle."""
    out = []
    assert len(results) == len(refs)
    for s, ref in enumerate(refs):
        where = "%sslot %d" % (tag and tag + " ", s)
        for l in range(fe.nlevels):
            for stage, got, want in (("pyramid", fe.mvImagePyramid(l, slot=s), ref.pyramid[l]),
                                     ("blur", fe.mvImagePyramid(l, slot=s, blurred=True), ref.blurred[l])):
                d = _image_difference(got, want)
                if d:
                    out.append("%s level %d %s (%dx%d): %s" % (where, l, stage, want.shape[1], want.shape[0], d))
            ca, cb = fe.candidates(l, slot=s), ref.candidates[l]
            if len(ca) != len(cb):
                out.append("%s level %d candidates: %d instead of %d" % (where, l, len(ca), len(cb)))
            else:
                for f in ("x", "y", "response"):
                    if not np.array_equal(ca[f], cb[f]):
                        i = int(np.nonzero(ca[f] != cb[f])[0][0])
                        out.append("%s level %d candidates: %s differs from entry %d on (%d of %d): (%g, %g, %g) instead of "
                                   "(%g, %g, %g)" % (where, l, f, i, int((ca[f] != cb[f]).sum()), len(ca), ca["x"][i], ca["y"][i],
                                                     ca["response"][i], cb["x"][i], cb["y"][i], cb["response"][i]))
                        break
        k, d, m = results[s]
        ko, do, mo = ref.result
        if len(k) != len(ko):
            out.append("%s keypoints: %d instead of %d" % (where, len(k), len(ko)))
        else:
            for f in k.dtype.names:
                if not np.array_equal(k[f], ko[f]):
                    out.append("%s keypoints: %s differs on %d of %d" % (where, f, int((k[f] != ko[f]).sum()), len(k)))
            if not np.array_equal(d, do):
                out.append("%s descriptors: %d of %d rows differ" % (where, int((d != do).any(1).sum()), len(d)))
        if m != mo:
            out.append("%s mono index: %d instead of %d" % (where, m, mo))
    return out


def compare_stages(fe, images, e, taps=None, refs=None, tag="", **batch_args):
    """compute_batch(images) on the context, then every stage of every used slot against the oracle Extractor `e` (refs: the
    images' References if the caller keeps them).  -> (results, refs); raises AssertionError listing every difference."""
    results = fe.compute_batch(images, **batch_args)
    if refs is None:
        refs = [Reference(e, im, taps) for im in images]
    diffs = stage_differences(fe, results, refs, tag)
    assert not diffs, "\n" + "\n".join(diffs)
    return results, refs
