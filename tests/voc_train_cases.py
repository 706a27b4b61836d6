"""TEST INFRASTRUCTURE: the training sets of the vocabulary-training tests, and the yardstick's result for each, computed
once per process and shared (never modified) by the tests that need it.

Descriptors are uniform random bytes or "clustered": c random centres, every feature one of them with f random single-bit
flips.  Documents: 12 roughly equal runs plus one empty document.  The mixed cases draw from one rng stream, first the
duplicate block, then the clustered block."""
import numpy as np

import voc_train_ref as ref


def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def clustered_desc(rng, n, c, f):
    centres = rng.integers(0, 256, (c, 32), dtype=np.uint8)
    out = centres[rng.integers(0, c, n)].copy()
    for _ in range(f):
        bit = rng.integers(0, 256, n)
        out[np.arange(n), bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
    return out


def documents(n):
    """12 roughly equal runs plus one empty document (the 7th)"""
    cuts = [int(round(i * n / 12.0)) for i in range(13)]
    return np.array(cuts[:7] + cuts[6:], np.int64)


def _mix900(rng):
    return np.concatenate([clustered_desc(rng, 500, 7, 0), clustered_desc(rng, 400, 20, 8)])


#: name -> (rng seed, builder, k, L, extra train arguments)
CASES = {
    "rand3000": (101, lambda r: random_desc(r, 3000), 5, 3, {}),
    "clu3000": (102, lambda r: clustered_desc(r, 3000, 40, 12), 5, 3, {}),
    "clu4000_k35": (103, lambda r: clustered_desc(r, 4000, 300, 10), 35, 2, {}),
    "dups600": (104, lambda r: clustered_desc(r, 600, 9, 0), 6, 3, {}),
    "rand500_deep": (105, lambda r: random_desc(r, 500), 4, 5, {}),
    "mix900": (106, _mix900, 6, 4, {}),
    "mix900_mask3": (106, _mix900, 6, 4, dict(rand_mask=3)),
    # 70000 features are 274 chunks of the 256-position seeding / partition kernels and 69 of the 1024-position
    # mean kernel: the root segment, and every level-2 segment (about 8750 features), spans far more than three chunks
    "clu70000": (107, lambda r: clustered_desc(r, 70000, 64, 16), 8, 2, {}),
    "tiny1": (108, lambda r: random_desc(r, 1), 4, 2, {}),
    "tiny2": (109, lambda r: random_desc(r, 2), 4, 2, {}),
    "tiny_k": (110, lambda r: random_desc(r, 4), 4, 2, {}),
    "tiny_k1": (111, lambda r: random_desc(r, 5), 4, 2, {}),
}
SEED = 20240607
#: the bound of the max_iter tests, and the case they run on (its longest Lloyd loop is far above 2)
MAX_ITER_CASE, MAX_ITER_BOUND = "rand3000", 2

_inputs, _expected = {}, {}


def inputs(name):
    """-> (desc, doc_offsets, train keyword arguments); read-only arrays"""
    if name not in _inputs:
        rs, build, k, L, extra = CASES[name]
        desc = build(np.random.default_rng(rs))
        desc.setflags(write=False)
        off = documents(len(desc))
        off.setflags(write=False)
        _inputs[name] = (desc, off, dict(k=k, L=L, weighting=0, scoring=0, seed=SEED, **extra))
    return _inputs[name]


def expected(name, **override):
    """the yardstick's vocabulary for a case (cached per argument set)"""
    key = (name, tuple(sorted(override.items())))
    if key not in _expected:
        desc, off, kw = inputs(name)
        kw = dict(kw, **override)
        _expected[key] = ref.train(desc, off, **kw)
    return _expected[key]
