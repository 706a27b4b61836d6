"""A BoW scene whose two FeatureVectors do NOT hold the same nodes, with the preconditions that prove it.  No GPU in
here: the CPU precondition test and the GPU tests import the same builders.

The regular scenes have ~2000 features against at most 100 vocabulary nodes at the chosen level, so both frames hold
every node and the node lists are identical: the lower_bound advance of either list in SearchByBoW /
SearchForTriangulation (fmatcher.cpp:733-741, :1225-1233, :1463-1471) -- on the device the binary search for the driver's
node in the other list and its miss exit -- never decides anything.  Here 200 features meet 1000 (levelsup 1) or 10000
(levelsup 0) nodes: most nodes of one frame are missing from the other, at the head and at the tail of the lists too."""
import numpy as np

from oracle import orbo
from vi_slam_amd import synth

W, H, NF = 320, 240, 200
LEVELSUP = (1, 0)
VOC_ARGS = (10, 4, 17)   # k, L, seed
# the synthetic scene moves by (+3, +1) px per step: epipolar lines are parallel to (3, 1)
F12 = np.array([[0, 0, 1], [0, 0, -3], [-1, 3, 0]], np.float32)
EPIPOLE = (-5000.0, -5000.0)


def frames():
    return [synth.make_frame(W, H, seed=3, step=s) for s in range(2)]


def vocabulary():
    return synth.make_vocabulary(VOC_ARGS[0], VOC_ARGS[1], seed=VOC_ARGS[2])


def oracle_features(imgs):
    """-> [(keypoints, descriptors)] of the oracle's extractor"""
    out = []
    for im in imgs:
        k, d, _ = orbo.Extractor(NF).compute(im)
        out.append((k, d))
    return out


def oracle_fvs(voc, feats, levelsup):
    return [orbo.bow_transform(voc, d, levelsup) for _, d in feats]


def flags(n0, n1):
    """random MapPoint flags for both sides (the same for every test that uses the scene)"""
    rng = np.random.default_rng(12)
    return (rng.random(n0) < 0.8).astype(np.uint8), (rng.random(n1) < 0.8).astype(np.uint8)


def u_right(kps, seed):
    """a stereo coordinate for about half of the keypoints (bStereo = mvuRight >= 0), -1 for the rest"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(len(kps)) < 0.5, np.maximum(kps["x"] - 5.0, 0.0), -1.0).astype(np.float32)


def node_census(fva, fvb):
    a, b = fva["fv_nodes"], fvb["fv_nodes"]
    shared = np.intersect1d(a, b)
    return dict(na=len(a), nb=len(b), shared=len(shared), only_a=len(a) - len(shared), only_b=len(b) - len(shared),
                ends_shared=[int(x in shared) for x in (a[0], a[-1], b[0], b[-1])])


def check_sparse(fva, fvb, levelsup):
    """the preconditions on the oracle's FeatureVectors: both lists advance by lower_bound, at both ends too.
    At levelsup 0 the first and the last node of each list are exclusive to it.  At levelsup 1 the scene does not
    give that: node 30, the first of frame b, is also in frame a (a starts at node 2, b at 30) -- so there the
    head miss (lower_bound lands on position 0 and finds another node) happens with a as the driver only, the first
    node of b hits; both last nodes are exclusive in either case, so the past-the-end exit is taken at both levels."""
    c = node_census(fva, fvb)
    assert c["only_a"] >= 30 and c["only_b"] >= 30, c
    assert c["shared"] >= 20, c
    assert c["ends_shared"] == ([0, 0, 0, 0] if levelsup == 0 else [0, 0, 1, 0]), c
    return c
