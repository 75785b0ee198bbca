"""Milliseconds of the depth-normals kernel (csrc/normals.hip, relpose_depth_normals) at the sizes a user runs: 64 views (32 pairs) of
160 x 640 and of 320 x 1280, radius 3, the default gate and neighbour count, on synthetic rooms with 1 % holes.  The median over --reps of
10 back-to-back whole calls after a warm-up, timed with events on the current stream, ALTERNATING with the same expression written with
PyTorch ops on the same GPU (unprojection, the 48 window offsets as rolled and shifted tensors, the gated sums, torch.linalg.eigh), so both
see the same clocks.  For the kernel the bytes it must move -- 4 B of depth in, 12 B of normal and 1 B of valid out per pixel -- over its
time, as a share of the 8 TB/s HBM peak.  Writes profiles/normals_time.txt (--out to write elsewhere).  These are whole-call times (one
launch plus the allocation of `valid`); for the kernel's own time run --kernel-only (11 calls per size, nothing else, nothing written)
under `rocprofv3 --kernel-trace` and read depth_normals_kernel's rows with tools/kernel_stats.py.

  python tools/normals_time.py [--reps 5] [--out PATH]
  rocprofv3 --kernel-trace -d DIR -- python tools/normals_time.py --kernel-only"""
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


def torch_normals(depth, dataset, r=3, gate_scale=3.0, min_neighbors=6, chunk=4 << 20):
    """The contract of DESIGN.md 4.12 with PyTorch ops (fp32; PyTorch's own summation order and eigen-solver) -> (normal [n,3,h,4h], valid).
    At most `chunk` pixels go through at a time: one batched torch.linalg.eigh over the 26 M matrices of 64 views of 320 x 1280 returned
    eigenvectors 33 degrees (median) off this kernel's and its own smaller batches' on the ROCm build measured."""
    import torch
    from relativepose_amd import synth
    n, h, w = depth.shape
    per = max(1, chunk // (h * w))
    if n > per:
        parts = [torch_normals(depth[i:i + per], dataset, r, gate_scale, min_neighbors, chunk) for i in range(0, n, per)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    dev = depth.device
    x = (torch.arange(w, device=dev) % h).float()
    xn = (x / h - 0.5) * 2.0
    yn = (0.5 - torch.arange(h, device=dev).float() / h) * 2.0
    face = torch.stack((xn[None, None, :] * depth, yn[None, :, None] * depth, -depth), -1)
    P = torch.empty_like(face)
    for slot in range(4):
        R = torch.from_numpy(synth.face_rotation(dataset, slot)).float().to(dev)
        P[:, :, slot * h:(slot + 1) * h] = face[:, :, slot * h:(slot + 1) * h] @ R.T
    has = depth != 0
    g = gate_scale * r * (2.0 / h) * depth
    g2 = g * g
    cnt = torch.zeros(n, h, w, device=dev)
    s = torch.zeros(n, h, w, 3, device=dev)
    S = torch.zeros(n, h, w, 3, 3, device=dev)
    rows = torch.arange(h, device=dev)
    for dy in range(-r, r + 1):
        inside = ((rows + dy >= 0) & (rows + dy < h))[None, :, None]
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            d = torch.roll(P, (-dy, -dx), (1, 2)) - P
            ok = (torch.roll(has, (-dy, -dx), (1, 2)) & inside & has & ((d * d).sum(-1) <= g2)).float()
            d = d * ok[..., None]
            cnt += ok
            s += d
            S += d[..., :, None] * d[..., None, :]
    C = S - s[..., :, None] * s[..., None, :] / (cnt + 1.0)[..., None, None]
    lam, vec = torch.linalg.eigh(C)
    nrm = vec[..., :, 0]
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    nrm = torch.where(((nrm * P).sum(-1) > 0)[..., None], -nrm, nrm)
    valid = has & (cnt >= min_neighbors) & (lam[..., 1] > 1e-6 * lam[..., 2])
    return (nrm * valid[..., None]).permute(0, 3, 1, 2).contiguous(), valid


def main():
    import torch
    from relativepose_amd import synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_time.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only the kernel, 11 calls per size, for a kernel-trace run")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ds, r = "suncg", 3
    lines = [f"# python tools/normals_time.py --reps {args.reps}, 1x MI355X (medians of whole calls, events on the stream, kernel and PyTorch "
             f"alternating; {args.views} views, radius {r}, gate_scale 3.0, min_neighbors 6, synthetic rooms with 1 % holes)"]
    for h in (160, 320):
        rooms = [synth.render_room(np.random.RandomState(900 + k), ds, 0.01, h)[2] for k in range(4)]          # 8 distinct views, repeated
        dep = np.concatenate(rooms * ((args.views + 7) // 8))[:args.views]
        depth = torch.from_numpy(np.ascontiguousarray(dep)).to(dev)
        n, w = depth.shape[0], 4 * h
        out = torch.empty(n, 3, h, w, device=dev)
        if args.kernel_only:
            for _ in range(11):
                util.depth_normals_dev(depth, ds, radius=r, out=out)
            torch.cuda.synchronize()
            continue
        ms, tms = alternate(lambda: util.depth_normals_dev(depth, ds, radius=r, out=out), lambda: torch_normals(depth, ds, r), args.reps)
        nrm, valid = util.depth_normals_dev(depth, ds, radius=r)
        tn, tv = torch_normals(depth, ds, r)
        both = (valid != 0) & tv
        ang = torch.rad2deg(torch.acos((nrm.double() * tn.double()).sum(1)[both].clamp(-1, 1)))
        nbytes = n * h * w * 17
        lines.append(f"relpose_depth_normals, {n} views of {h} x {w}: {ms:.3f} ms per call ({n * h * w / ms / 1e6:.2f} G pixels per second); "
                     f"{nbytes / 1e9:.3f} GB to move at least (4 B in, 13 B out per pixel) = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = "
                     f"{100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak; valid pixels {100 * float((valid != 0).float().mean()):.1f} %; "
                     f"the same expression with PyTorch ops: {tms:.1f} ms, {tms / ms:.0f} x the kernel; validity differs from PyTorch's at "
                     f"{int(((valid != 0) != tv).sum())} pixels, angle to PyTorch's normals: median {float(ang.median()):.1e}, max {float(ang.max()):.1e} degrees")
        del out, nrm, valid, tn, tv
        torch.cuda.empty_cache()
    if args.kernel_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
