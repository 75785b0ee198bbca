"""Milliseconds of relpose_ransac (csrc/ransac.hip) at the reference's settings (4 M iterations, 500 validations) on the shapes of
tools/fgr_time.py: 32 SUNCG-shaped pairs (the observed 160x160 block of synth.make_pairs) and single 480x640 kinect pairs: the median
of --reps whole calls (front end, screen rounds, validation, selection and the one status read-back) after a warm-up, timed with
events on the current stream.  The split over the kernels is what a rocprofv3 --kernel-trace --stats run of this script shows.
Writes profiles/ransac_time.txt (--out to write elsewhere).

  python tools/ransac_time.py [--reps 5] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fgr_time import timed  # noqa: E402


def main():
    import torch
    from relativepose_amd import _lib, baselines, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    d = synth.make_pairs(32, 900, "suncg")
    pc, valid = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(64, *d["depth"].shape[2:])).to(dev), "suncg")
    _, st, out = baselines.global_registration_dev(pc, valid, stages=True)
    ms = timed(lambda: baselines.global_registration_dev(pc, valid), args.reps)
    fms = timed(lambda: baselines.fast_global_registration_dev(pc, valid), args.reps)
    cnt, nit = out["down_count"].cpu().numpy(), out["n_iterations"].cpu().numpy()
    lines.append(f"suncg 32 pairs (P = {pc.shape[1]} per cloud, voxels per cloud {int(cnt.min())}..{int(cnt.max())}): {ms:.2f} ms per call, "
                 f"{ms / 32:.3f} ms per pair; statuses {np.bincount(st.cpu().numpy(), minlength=5).tolist()}; iterations screened per pair "
                 f"{int(nit.min())}..{int(nit.max())} (median {int(np.median(nit))}); relpose_fgr on the same batch {fms:.2f} ms")
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    for k in range(2):
        dep = (2.0 + 0.6 * np.sin(xx / 90.0 + k) * np.cos(yy / 70.0) + 0.002 * rs.randn(480, 640)).astype(np.float32)
        dd = torch.from_numpy(np.stack([dep, np.roll(dep, 12, axis=1)])).to(dev)
        P = 480 * 640
        pcf = torch.empty(2, P, 3, dtype=torch.float64, device=dev)
        vf = torch.empty(2, P, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().relpose_depth2pc_full(_lib.ptr(dd), _lib.ptr(pcf), _lib.ptr(vf), 2, 480, 640, _lib.stream_ptr()), "depth2pc_full")
        _, st, out = baselines.global_registration_dev(pcf, vf, stages=True)
        ms = timed(lambda: baselines.global_registration_dev(pcf, vf), args.reps)
        lines.append(f"kinect 480x640 pair {k} (voxels {out['down_count'].cpu().numpy().tolist()}): {ms:.2f} ms per call; status {int(st[0])}, "
                     f"iterations screened {int(out['n_iterations'][0])}, fitness {float(out['fitness'][0]):.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
