"""Milliseconds of relpose_cicp (csrc/cicp.hip) and of the whole cgs baseline (relpose_ransac, then relpose_cicp) on 1 and 32
SUNCG-shaped pairs (the observed 160x160 block of synth.make_pairs, coloured by the observed block of its rgb): whole calls -- every
launch and the one status read-back -- after a warm-up of the same shape, timed with events on the current stream.  The coloured ICP
alone starts from the RANSAC pose of the same pairs, as the cgs baseline does.  Reported per case: the median, the minimum and the
maximum of --reps calls (the spread), and how many iterations the levels ran.  No time is gated.  The split over the kernels is what a
rocprofv3 --kernel-trace --stats run of this script shows.  Writes profiles/cicp_time.txt (--out to write elsewhere).

  python tools/cicp_time.py [--reps 7] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(fn, reps):
    """-> (median, min, max) ms of `reps` calls after one warm-up call."""
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    import torch
    from relativepose_amd import baselines, evaluation, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cicp_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# python tools/cicp_time.py --reps {args.reps}, 1x MI355X: whole calls (median, min .. max of {args.reps} after a warm-up); voxel cap 32768, "
             "lambda_geometric 0.968"]
    d = synth.make_pairs(32, 900, "suncg")
    pc32, valid32 = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(64, *d["depth"].shape[2:])).to(dev), "suncg")
    col32 = torch.from_numpy(evaluation.observed_colors(d["rgb"].reshape(64, *d["rgb"].shape[2:]))).to(dev)
    for B in (1, 32):
        pc, col, valid = pc32[:2 * B], col32[:2 * B], valid32[:2 * B]
        init, s0, _ = baselines.global_registration_dev(pc, valid)
        _, st, out = baselines.colored_icp_dev(pc, col, valid, init=init, stages=True)
        cnt, nit = out["down_count"].cpu().numpy(), out["n_iterations"].cpu().numpy()
        del out
        icp = spread(lambda: baselines.colored_icp_dev(pc, col, valid, init=init), args.reps)
        gs = spread(lambda: baselines.global_registration_dev(pc, valid), args.reps)
        cgs = spread(lambda: baselines.color_registration_dev(pc, col, valid), args.reps)
        f = lambda t: f"{t[0]:.2f} ms ({t[1]:.2f} .. {t[2]:.2f})"
        lines.append(f"suncg {B} pair{'s' if B > 1 else ''} (P = {pc.shape[1]} per cloud; voxels per cloud at 4 / 2 / 1 cm up to "
                     f"{int(cnt[:, 0].max())} / {int(cnt[:, 1].max())} / {int(cnt[:, 2].max())}): coloured ICP alone {f(icp)}, "
                     f"{icp[0] / B:.3f} ms per pair; RANSAC alone {f(gs)}; the full cgs {f(cgs)}, {cgs[0] / B:.3f} ms per pair; "
                     f"ICP statuses {np.bincount(st.cpu().numpy(), minlength=4).tolist()}, RANSAC statuses "
                     f"{np.bincount(s0.cpu().numpy(), minlength=5).tolist()}; evaluations per level: median "
                     f"{np.median(nit, 0).astype(int).tolist()}, max {nit.max(0).tolist()} of 50 / 30 / 14")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
