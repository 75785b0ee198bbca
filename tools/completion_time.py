"""Milliseconds of the completion-loss kernels (csrc/completion.hip) at the sizes a user runs: B = 32 pairs (64 images) of 160 x 640, S = 15,
Ct = 54.  relpose_completion_loss with labels and ce_cross, and relpose_contrast_loss at K = 2000 correspondences and 100 negatives per
pair: the median over --reps of 10 back-to-back whole calls after a warm-up, timed with events on the current stream, ALTERNATING with the same expressions
evaluated by PyTorch on the same GPU (mainPanoCompletion2view.py:549-567 with the [N,N,H,W] broadcast reduced algebraically, and :444,
:453), so both see the same clocks.  For the loss kernel the bytes it must move -- channels 0 .. 7 + S of f, complete, label, mask -- over
its time, as a share of the 8 TB/s HBM peak.  Writes profiles/completion_time.txt (--out to write elsewhere).

  python tools/completion_time.py [--reps 5] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def alternate(fa, fb, reps, inner=10):
    """Medians (ms per call) of fa and fb, alternating: every repetition times `inner` back-to-back calls of fa, then one call of fb (the
    slower side), after one warm-up call of each."""
    import torch
    fa(), fb()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts, k in ((fa, ta, inner), (fb, tb, 1)):
            ev[0].record()
            for _ in range(k):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / k)
    return float(np.median(ta)), float(np.median(tb))


def torch_losses(f, complete, label, S):
    """The reference's expressions (:553-567) -> (errG_rgb, errG_n, errG_d, errG_s)."""
    import torch
    w = (complete[:, 6:7] != 0).float()
    rgb = ((f[:, 0:3] - complete[:, 0:3]) * w).abs().mean()
    n = ((f[:, 3:6] - complete[:, 3:6]) * w).abs().mean()
    d = ((f[:, 6:7] - complete[:, 6:7]) * w).abs().mean()
    ce = torch.nn.functional.cross_entropy(f[:, 7:7 + S], label.long(), reduction="none")
    s = (ce.sum(0) * w[:, 0].sum(0)).sum() / (ce.shape[0] * ce.numel()) * 0.1          # the mean of the [N,N,H,W] product without building it
    return rgb, n, d, s


def torch_contrast(f, off, C, idx_src, idx_tgt, neg, margin=0.5):
    """:444 and :453 per pair -> (pos_sum [B], neg_sum [B])."""
    import torch
    B = f.shape[0] // 2
    pos, ngs = [], []
    for b in range(B):
        S = f[2 * b, off:off + C][:, idx_src[b, :, 1].long(), idx_src[b, :, 0].long()]              # [C, K]
        T = f[2 * b + 1, off:off + C][:, idx_tgt[b, :, 1].long(), idx_tgt[b, :, 0].long()]
        Ng = f[2 * b + 1, off:off + C][:, neg[b, :, :, 1].long(), neg[b, :, :, 0].long()]           # [C, K, M]
        pos.append((S - T).pow(2).sum(0).sum())
        ngs.append(torch.relu(margin - (S.unsqueeze(2) - Ng).pow(2).sum(0)).sum())
    return torch.stack(pos), torch.stack(ngs)


def main():
    import torch
    from relativepose_amd import completion, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "completion_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, h = args.pairs, args.height
    N, H, W, S, Ct, off, C = 2 * B, h, 4 * h, 15, 54, 22, 32
    lines = [f"# python tools/completion_time.py --reps {args.reps}, 1x MI355X (medians of whole calls, events on the stream, kernel and PyTorch "
             f"alternating; {N} images of {H} x {W}, S = {S}, Ct = {Ct})"]
    g = torch.Generator(device=dev).manual_seed(1)
    f = torch.randn(N, Ct, H, W, device=dev, generator=g)
    f[:, off:] = 0.15 * torch.tanh(f[:, off:])
    complete = torch.randn(N, 7, H, W, device=dev, generator=g)
    complete[:, 6][torch.rand(N, H, W, device=dev, generator=g) < 0.05] = 0
    label = torch.randint(0, S, (N, H, W), device=dev, generator=g, dtype=torch.uint8)
    mask = util.apply_mask_dev(torch.ones(N, 1, H, W, device=dev), "second")[1]

    ms, tms = alternate(lambda: completion.completion_loss_dev(f, complete, label, mask, None, S=S),
                        lambda: torch_losses(f, complete, label, S), args.reps)
    sums, _, cross, _ = completion.completion_loss_dev(f, complete, label, mask, None, S=S)
    sc = completion.completion_scalars(sums.cpu().numpy(), cross.cpu().numpy(), H, W)
    ref = [float(v) for v in torch_losses(f, complete, label, S)]
    rel = max(abs(sc[k] - r) / abs(r) for k, r in zip(("errG_rgb", "errG_n", "errG_d", "errG_s"), ref))
    nbytes = N * H * W * ((7 + S) * 4 + 7 * 4 + 1 + 4)
    lines.append(f"relpose_completion_loss (labels, ce_cross): {ms:.3f} ms per call; {nbytes / 1e9:.3f} GB to read at least "
                 f"({(7 + S)} of {Ct} channels of f, complete, label, mask) = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = "
                 f"{100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak (the CE / w maps for ce_cross add {N * H * W * 12 * 2 / 1e9:.3f} GB "
                 f"written and read back); the PyTorch expressions: {tms:.2f} ms, {tms / ms:.1f} x the kernel; largest relative difference "
                 f"of the four scalars from PyTorch's fp32 means {rel:.1e}")
    ms0, _ = alternate(lambda: completion.completion_loss_dev(f, complete, None, mask, None, S=S), lambda: None, args.reps)
    nb0 = N * H * W * (7 * 4 + 7 * 4 + 4)
    lines.append(f"relpose_completion_loss (no labels: the L1 rows only): {ms0:.3f} ms per call; {nb0 / 1e9:.3f} GB = "
                 f"{nb0 / (ms0 * 1e-3) / 1e12:.2f} TB/s = {100 * nb0 / (ms0 * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")

    rs = np.random.RandomState(0)
    K, M = 2000, 100
    idx = lambda *s: torch.from_numpy(np.stack([rs.randint(0, W, s), rs.randint(0, H, s)], -1).astype(np.int32)).to(dev)
    isrc, itgt, neg = idx(B, K), idx(B, K), idx(B, K, M)
    ms, tms = alternate(lambda: completion.contrast_loss_dev(f, off, C, isrc, itgt, None, neg),
                        lambda: torch_contrast(f, off, C, isrc, itgt, neg), max(1, min(args.reps, 3)))
    pos, ngs, act, _ = completion.contrast_loss_dev(f, off, C, isrc, itgt, None, neg)
    tp, tn = torch_contrast(f, off, C, isrc, itgt, neg)
    rel = max(float(((pos - tp.double()).abs() / tp.double()).max()), float(((ngs - tn.double()).abs() / tn.double()).max()))
    lines.append(f"relpose_contrast_loss, C = {C}, K = {K}, {M} negatives: {ms:.3f} ms per call ({B * K * M / ms / 1e6:.2f} G negatives per second, "
                 f"{B * K * M * C * 4 / (ms * 1e-3) / 1e12:.2f} TB/s of gathered descriptor bytes); active negatives "
                 f"{100 * float(act.sum()) / (B * K * M):.1f} %; the PyTorch expression: {tms:.2f} ms, {tms / ms:.1f} x the kernel; largest relative "
                 f"difference of the per-pair sums from PyTorch's fp32 sums {rel:.1e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
