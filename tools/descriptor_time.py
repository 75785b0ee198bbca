"""Milliseconds of the descriptor-evaluation kernels (csrc/descriptor.hip) at the sizes a user runs: relpose_dense_nn at B = 32 pairs of
160 x 640 panoramas with 5000 queries each (the loaders' setting, datasets/SUNCG.py:324), and relpose_descriptor_rank at B = 32, C = 32
with E = 100 (the reference's sample, mainPanoCompletion2view.py:398) and E = 2000 (every correspondence) slots per pair: the median
of --reps whole calls after a warm-up, timed with events on the current stream.  For the rank kernel the achieved share of the fp32
vector peak (3 operations per channel, pixel and slot -- subtract, multiply, add, none fused -- against 157.3 TFLOP/s, which counts a
fused multiply-add as two), and the same expression evaluated by PyTorch on the same GPU, chunked to fit memory, with the ratio.
Writes profiles/descriptor_time.txt (--out to write elsewhere).

  python tools/descriptor_time.py [--reps 5] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fgr_time import timed  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12


def torch_rank(f, off, C, idx_src, idx_tgt, chunk=32):
    """The reference's expression (mainPanoCompletion2view.py:401-405) per pair, `chunk` slots at a time -> count [B,E] i64."""
    import torch
    B = f.shape[0] // 2
    out = []
    for b in range(B):
        xs, ys, xt, yt = (idx_src[b, :, 0].long(), idx_src[b, :, 1].long(), idx_tgt[b, :, 0].long(), idx_tgt[b, :, 1].long())
        featSrc = f[2 * b, off:off + C][:, ys, xs]
        featTgt = f[2 * b + 1, off:off + C][:, yt, xt]
        dist = (featSrc - featTgt).pow(2).sum(0)
        tgt = f[2 * b + 1, off:off + C].reshape(C, 1, -1)
        cnt = [((featSrc[:, e:e + chunk].unsqueeze(2) - tgt).pow(2).sum(0) < dist[e:e + chunk].unsqueeze(1)).sum(1)
               for e in range(0, featSrc.shape[1], chunk)]
        out.append(torch.cat(cnt))
    return torch.stack(out)


def main():
    import torch
    from relativepose_amd import descriptor, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "descriptor_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, h = args.pairs, args.height
    HW, C, off, Ct = 4 * h * h, 32, 22, 54
    lines = [f"# python tools/descriptor_time.py --reps {args.reps}, 1x MI355X (medians of whole calls, events on the stream; B = {B}, {h} x {4 * h})"]

    d = synth.make_pairs(B, 900, "suncg", h=h)
    depth = torch.from_numpy(d["depth"].reshape(2 * B, h, 4 * h)).to(dev)
    pc, valid = util.pano2pc_dev(depth, "suncg")
    R = torch.from_numpy(d["R"].reshape(2 * B, 4, 4)).to(dev)
    rs = np.random.RandomState(0)
    query = torch.from_numpy(rs.randint(0, HW, (B, 5000)).astype(np.int32)).to(dev)
    ms = timed(lambda: descriptor.dense_nn_dev(pc, valid, R, query), args.reps)
    hits = descriptor.dense_nn_dev(pc, valid, R, query)[2].sum(1).cpu().numpy()
    ev = B * 5000 * HW
    lines.append(f"relpose_dense_nn, nq = 5000: {ms:.3f} ms per call ({ev / ms / 1e6:.1f} G float64 distance evaluations per second); "
                 f"hits per pair {int(hits.min())}..{int(hits.max())}")

    g = torch.Generator(device=dev).manual_seed(1)
    f = torch.randn(2 * B, Ct, h, 4 * h, device=dev, generator=g)
    mask = util.apply_mask_dev(torch.ones(2 * B, 1, h, 4 * h, device=dev), "second")[1]
    for E in (100, 2000):
        idx = [torch.from_numpy(np.stack([rs.randint(0, 4 * h, (B, E)), rs.randint(0, h, (B, E))], -1).astype(np.int32)).to(dev) for _ in range(2)]
        ms = timed(lambda: descriptor.descriptor_rank_dev(f, off, C, idx[0], idx[1], None, None, mask), args.reps)
        flop = 3.0 * C * HW * E * B
        tms = timed(lambda: torch_rank(f, off, C, idx[0], idx[1]), max(1, min(args.reps, 3)))
        got = descriptor.descriptor_rank_dev(f, off, C, idx[0], idx[1], None, None, mask)[0].long()
        ref = torch_rank(f, off, C, idx[0], idx[1])
        diff = (got - ref).abs()
        lines.append(f"relpose_descriptor_rank, C = {C}, E = {E}: {ms:.3f} ms per call, {flop / ms / 1e9:.2f} TFLOP/s = "
                     f"{100 * flop / (ms * 1e-3) / PEAK_FP32_VECTOR:.1f} % of the fp32 vector peak (compute-bound: {B * 2 * Ct * HW * 4 / 1e9:.2f} GB "
                     f"of maps at most); the PyTorch expression in chunks of 32 slots: {tms:.2f} ms, {tms / ms:.1f} x the kernel; "
                     f"slots whose count differs from PyTorch's summation order: {int((diff > 0).sum())} of {B * E} (largest difference {int(diff.max())})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
