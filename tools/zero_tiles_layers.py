"""A few full-plan SCNet forwards of MASKED views at the bench batch -- target for a rocprofv3 --kernel-trace run of the zero-tile passes.
python tools/zero_tiles_layers.py [images] [forwards] [precision] [zero_tiles]   (zero_tiles: RELPOSE_TUNE_ZERO_TILES, default 0 = skip)

The input is bench.py's configs[1] batch (synth.make_pairs(pairs, 2000, 'suncg'), 'second' mask) with the partner views warped at the
ground-truth relative poses; prints the read-out (workgroups computed / dropped per layer)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from types import SimpleNamespace

import numpy as np
import torch

from relativepose_amd import _lib, synth, weights
from relativepose_amd.model import SCNet
from relativepose_amd.util import build_view_dev, warp_pairs_dev

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=15))
net.load_state_dict(weights.make_state_dict(7, 15))
net.set_precision(sys.argv[3] if len(sys.argv) > 3 else "bf16x6")
if len(sys.argv) > 4 and "zero_tiles" in _lib.TUNE_KEYS:
    _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["zero_tiles"], int(sys.argv[4]))
d = synth.make_pairs(n // 2, 2000, "suncg")
h = d["depth"].shape[-2]
dev = torch.device("cuda:0")
x = torch.zeros(n, 16, h, 4 * h, device=dev)
x[:, :8] = build_view_dev(torch.from_numpy(d["rgb"]).reshape(n, 3, h, 4 * h).to(dev), torch.from_numpy(d["norm"]).reshape(n, 3, h, 4 * h).to(dev),
                          torch.from_numpy(d["depth"]).reshape(n, h, 4 * h).to(dev), "second")
pose = np.zeros((n, 4, 4))
for b in range(n // 2):
    R = np.linalg.inv(d["R"][b, 1]) @ d["R"][b, 0]
    pose[2 * b], pose[2 * b + 1] = np.linalg.inv(R), R
warp_pairs_dev(x, torch.from_numpy(pose).to(dev), "suncg")
for _ in range(reps):
    y = net(x)
torch.cuda.synchronize()
print("ok", float(y.abs().mean()), "nonzero input share", float((x != 0).float().mean()), net.zero_tiles() if hasattr(net, "zero_tiles") else None)
