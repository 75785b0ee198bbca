"""Milliseconds of relpose_fgr (csrc/fgr.hip): 32 SUNCG-shaped pairs (the observed 160x160 block of synth.make_pairs) and
single 480x640 kinect pairs: the median of --reps whole calls (eight kernels and the one status read-back) after a warm-up, timed
with events on the current stream.  The split over the eight kernels is what a rocprofv3 --kernel-trace run of this script shows.
Writes profiles/fgr_time.txt.

  python tools/fgr_time.py [--reps 10]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ts))


def main():
    import torch
    from relativepose_amd import baselines, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    d = synth.make_pairs(32, 900, "suncg")
    pc, valid = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(64, *d["depth"].shape[2:])).to(dev), "suncg")
    _, st, stg = baselines.fast_global_registration_dev(pc, valid, stages=True)
    ms = timed(lambda: baselines.fast_global_registration_dev(pc, valid), args.reps)
    cnt = stg["down_count"].cpu().numpy()
    lines.append(f"suncg 32 pairs (P = {pc.shape[1]} per cloud, voxels per cloud {int(cnt.min())}..{int(cnt.max())}): {ms:.2f} ms per call, "
                 f"{ms / 32:.3f} ms per pair; statuses {np.bincount(st.cpu().numpy(), minlength=4).tolist()}")
    # single kinect pairs: full 480x640 depth back-projected (util.depth2pc's 480x640 branch) of a planar-and-box scene
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    for k in range(2):
        dep = (2.0 + 0.6 * np.sin(xx / 90.0 + k) * np.cos(yy / 70.0) + 0.002 * rs.randn(480, 640)).astype(np.float32)
        dd = torch.from_numpy(np.stack([dep, np.roll(dep, 12, axis=1)])).to(dev)
        from relativepose_amd import _lib
        P = 480 * 640
        pcf = torch.empty(2, P, 3, dtype=torch.float64, device=dev)
        vf = torch.empty(2, P, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().relpose_depth2pc_full(_lib.ptr(dd), _lib.ptr(pcf), _lib.ptr(vf), 2, 480, 640, _lib.stream_ptr()), "depth2pc_full")
        _, st, stg = baselines.fast_global_registration_dev(pcf, vf, stages=True)
        ms = timed(lambda: baselines.fast_global_registration_dev(pcf, vf), args.reps)
        lines.append(f"kinect 480x640 pair {k} (voxels {stg['down_count'].cpu().numpy().tolist()}): {ms:.2f} ms per call; status {int(st[0])}")
    out = os.path.join(ROOT, "profiles", "fgr_time.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
