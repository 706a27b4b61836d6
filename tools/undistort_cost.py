#!/usr/bin/env python3
"""Target for `rocprofv3 --kernel-trace --stats`: batched extraction passes on HBM-resident frames by a context WITH a
distorted camera (k1 != 0), so that every pass also runs k_undistort_kps.
    undistort_cost.py [iters=20] [B=32] [NF=1000] [W=1241] [H=376]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import vi_slam_amd as V  # noqa: E402
from vi_slam_amd import synth  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
NF = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
W = int(sys.argv[4]) if len(sys.argv) > 4 else 1241
H = int(sys.argv[5]) if len(sys.argv) > 5 else 376
fe = V.FExtractor(NF, 1.2, 8, 20, 7, W, H, max_batch=B)
# ZED cam0's radtan coefficients (reference config/zed_camera.yaml), intrinsics centred on this image
fe.set_camera(669.2387507702717, 669.6062139634853, W / 2.0, H / 2.0,
              dist=(0.0018645604002542789, -0.009206711115906055, -0.001490842343490958, 0.0047045781898403))
pitch = (W + 127) & ~127
dev = torch.zeros((B, H, pitch), dtype=torch.uint8, device="cuda")
for s in range(B):
    dev[s, :, :W] = torch.from_numpy(synth.make_frame(W, H, step=s)).cuda()
ptrs = [dev[s].data_ptr() for s in range(B)]
torch.cuda.synchronize()
n = 0
for _ in range(iters):
    fe.compute_batch_async(ptrs, pitch, (0, 0), to_host=False)
    n = sum(c for c, _ in fe.wait())
u = fe.ukeypoints(B - 1)
print("undistort_cost: %d passes of %d slots, %d keypoints per pass, last slot %d ukeypoints" % (iters, B, n, len(u)))
fe.close()
