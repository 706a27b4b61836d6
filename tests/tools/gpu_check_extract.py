#!/usr/bin/env python3
"""Stage-by-stage parity probe (GPU box): HIP extractor vs the CPU oracle on synthetic frames, through the comparison of
tests/stage_compare.py (pyramid, blurred level and candidate list of every level and slot, then keypoints and descriptors).
usage: gpu_check_extract.py [W H NFEATURES]"""
import sys, time
import os
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import vi_slam_amd as V
from vi_slam_amd import synth
from oracle import orbo
from stage_compare import Reference, stage_differences

def main():
    W, H, NF = 1241, 376, 2000
    if len(sys.argv) > 3:
        W, H, NF = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    e = orbo.Extractor(NF)
    fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, max_batch=4)
    diffs = []
    for name, imgs in (("one image", [synth.make_frame(W, H)]), ("batch of 4", [synth.make_frame(W, H, step=s) for s in range(4)])):
        t0 = time.time()
        res = fe.compute_batch(imgs)
        print("%s: %.1f ms, keypoints %s" % (name, (time.time() - t0) * 1e3, [len(r[0]) for r in res]))
        d = stage_differences(fe, res, [Reference(e, im) for im in imgs], tag=name)
        print("%s: %s" % (name, "every stage of every slot equals the oracle" if not d else "%d differences" % len(d)))
        diffs += d
    for d in diffs:
        print("  ", d)
    fe.close()
    print("ALL OK" if not diffs else "MISMATCH")
    return 0 if not diffs else 1

if __name__ == "__main__":
    sys.exit(main())
