"""The SCNet forwards of a few bench steps, one after the other on one workspace -- target for a rocprofv3 --kernel-trace run of the input
resize, the occupancy pass and conv1.
python tools/conv1_zero_layers.py [images] [steps] [precision] [conv1_zero]   (conv1_zero: RELPOSE_TUNE_CONV1_ZERO, default 0 = skip)

A step = the level-0 plan (tagged, warped channels zero) and two self-cached forwards.  The inputs are bench.py's configs[1] batches
(synth.make_pairs(pairs, 2000 + step, 'suncg'), 'second' mask: another batch per step, like the rotating batches of the bench) with the
partner views warped at the ground-truth relative poses (level 1) and at those poses turned by 2 degrees (level 2).  Prints the conv1
read-out of every forward (launched, skipped without a store, stored as zeros), in launch order = the order of the kernel trace.

python tools/conv1_zero_layers.py --summarise TRACE.csv [forwards]   -> per forward the durations (us) of the three kernels, from the
kernel trace of such a run (forwards = 3 x steps, in launch order)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(path, forwards):
    import csv
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))), key=lambda r: r[0])
    per = []
    for s, e, name in rows:
        us = (e - s) / 1000.0
        if "resize_in" in name:
            per.append({"resize_in": us, "x0_occupancy": 0.0, "conv1": 0.0})
        elif "x0_occupancy_kernel" in name and per:
            per[-1]["x0_occupancy"] += us
        elif "conv1_mfma_kernel" in name and per:
            per[-1]["conv1"] += us
    per = per[-forwards:] if forwards else per
    print("forward  level   resize_in  x0_occupancy  conv1_mfma     sum   (us)")
    for i, p in enumerate(per):
        print(f"  {i:3d}      {i % 3}    {p['resize_in']:8.1f}    {p['x0_occupancy']:8.1f}    {p['conv1']:8.1f}  {sum(p.values()):8.1f}")


def main():
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
    if len(sys.argv) > 4 and "conv1_zero" in _lib.TUNE_KEYS:
        _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["conv1_zero"], int(sys.argv[4]))
    dev = torch.device("cuda:0")
    c, s = np.cos(np.radians(2.0)), np.sin(np.radians(2.0))
    turn = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    batches = []
    for st in range(steps):
        d = synth.make_pairs(n // 2, 2000 + st, "suncg")
        h = d["depth"].shape[-2]
        x = torch.zeros(n, 16, h, 4 * h, device=dev)
        x[:, :8] = build_view_dev(torch.from_numpy(d["rgb"]).reshape(n, 3, h, 4 * h).to(dev), torch.from_numpy(d["norm"]).reshape(n, 3, h, 4 * h).to(dev),
                                  torch.from_numpy(d["depth"]).reshape(n, h, 4 * h).to(dev), "second")
        levels = [x]
        for extra in (np.eye(4), turn):
            pose = np.zeros((n, 4, 4))
            for b in range(n // 2):
                R = extra @ (np.linalg.inv(d["R"][b, 1]) @ d["R"][b, 0])
                pose[2 * b], pose[2 * b + 1] = np.linalg.inv(R), R
            xl = x.clone()
            warp_pairs_dev(xl, torch.from_numpy(pose).to(dev), "suncg")
            levels.append(xl)
        batches.append(levels)
    torch.cuda.synchronize()
    chk = 0.0
    for st, levels in enumerate(batches):
        tag = net.new_self_tag()
        for lvl, x in enumerate(levels):
            y = net.forward(x, zero_warp=(lvl == 0), self_tag=tag)
            chk += float(y.abs().mean())
            print(f"step {st} level {lvl}: conv1 units (launched, skipped, zero-stored) =", net.conv1_zero() if hasattr(net, "conv1_zero") else None)
    torch.cuda.synchronize()
    print("ok checksum", chk)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    else:
        main()
