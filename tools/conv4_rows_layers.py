"""Three steps of bench.py configs[1]'s SCNet forwards on one workspace -- level 0 (zero warp, tagged, pose outputs) and two self-cached
levels with the partner views warped at the ground-truth poses -- as the target of a rocprofv3 --kernel-trace run of conv4's row lists.
python tools/conv4_rows_layers.py [images] [steps] [precision] [conv4_rows] [dense]   (conv4_rows: RELPOSE_TUNE_CONV4_ROWS, default 0;
dense: full-plan forwards of a randn input instead, for the per-row rates of the two conv4 kernels)

Prints per level the read-out (rows computed / dropped / list path per K slice), the HIP-event time of each forward and a checksum of the
outputs' bit patterns, which must be the same on every arm (and on a build without the knob, which ignores the last argument)."""
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
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=15))
net.load_state_dict(weights.make_state_dict(7, 15))
net.set_precision(sys.argv[3] if len(sys.argv) > 3 else "bf16x6")
knob = int(sys.argv[4]) if len(sys.argv) > 4 else 0
if "conv4_rows" in _lib.TUNE_KEYS:
    _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["conv4_rows"], knob)
d = synth.make_pairs(n // 2, 2000, "suncg")
h = d["depth"].shape[-2]
dev = torch.device("cuda:0")
x0 = torch.zeros(n, 16, h, 4 * h, device=dev)
x0[:, :8] = build_view_dev(torch.from_numpy(d["rgb"]).reshape(n, 3, h, 4 * h).to(dev), torch.from_numpy(d["norm"]).reshape(n, 3, h, 4 * h).to(dev),
                           torch.from_numpy(d["depth"]).reshape(n, h, 4 * h).to(dev), "second")
pose = np.zeros((n, 4, 4))
for b in range(n // 2):
    R = np.linalg.inv(d["R"][b, 1]) @ d["R"][b, 0]
    pose[2 * b], pose[2 * b + 1] = np.linalg.inv(R), R
x1 = x0.clone()
warp_pairs_dev(x1, torch.from_numpy(pose).to(dev), "suncg")
if len(sys.argv) > 5 and sys.argv[5] == "dense":
    # the per-row rates of the two conv4 kernels: full-plan forwards of a dense input (knob 2: every row listed, knob 1: every row on the strip kernel)
    xd = torch.randn(n, 16, h, 4 * h, device=dev)
    for _ in range(steps + 1):
        y = net.forward(xd)
    torch.cuda.synchronize()
    print("dense", "knob", knob, "checksum", int(y.view(torch.int32).to(torch.int64).sum()), net.conv4_rows() if hasattr(net, "conv4_rows") else None)
    sys.exit(0)
ms = [[], [], []]
for step in range(steps + 1):                                 # (step 0 warms up: plans, workspace)
    tag = net.new_self_tag()
    sums, rows = [], []
    for level in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = net.forward(x0 if level == 0 else x1, zero_warp=level == 0, outputs="pose", self_tag=tag)
        e1.record()
        torch.cuda.synchronize()
        if step:
            ms[level].append(e0.elapsed_time(e1))
        sums.append(int(y.view(torch.int32).to(torch.int64).sum()))
        rows.append(net.conv4_rows() if hasattr(net, "conv4_rows") else None)
for level in range(3):
    r = rows[level]
    print(f"level {level}: forward ms {' '.join('%.3f' % v for v in ms[level])}  checksum {sums[level]}")
    if r:
        print("   rows computed / dropped / list path per slice:", " ".join(f"{c}/{dr}/{int(lp)}" for c, dr, lp in r),
              f" dropped share {sum(dr for _, dr, _ in r) / max(sum(c + dr for c, dr, _ in r), 1):.3f}")
print("conv4_rows knob", knob if "conv4_rows" in _lib.TUNE_KEYS else "absent", "images", n)
