"""Milliseconds of the SIFT descriptor and rank kernels (csrc/siftdesc.hip) at the sizes a user runs, B = 32 pairs of 160 x 640 panoramas:
relpose_sift_describe in the shape evalSiftDescriptor calls it (per pair 2 x 100 correspondence points + the target's step-5 grid of
4096 points, size 5: 55 x 55 samples per keypoint) and on the step-1 grid of every view (102400 keypoints of size 1: 11 x 11 samples),
and relpose_sift_rank at (E, P) = (100, 4096) (the reference's sample against the step-5 grid) and (2000, 102400) (every correspondence
against the step-1 grid): the median of --reps whole calls after a warm-up, timed with events on the current stream.  For the descriptor
kernel the raster samples per second (the (2 radius + 1)^2 window of every used keypoint), for the rank kernel the share of the int8 matrix
peak (2 operations per byte product against 5.0 POP/s dense, twice the bf16 rate).  Writes profiles/siftdesc_time.txt (--out to write elsewhere).

  python tools/siftdesc_time.py [--reps 5] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fgr_time import timed  # noqa: E402

PEAK_I8 = 5.0e15


def main():
    import torch
    from relativepose_amd import descriptor, rputil, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siftdesc_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, h = args.pairs, args.height
    w = 4 * h
    lines = [f"# python tools/siftdesc_time.py --reps {args.reps}, 1x MI355X (medians of whole calls, events on the stream; B = {B}, {h} x {w})"]

    d = synth.make_pairs(min(B, 4), 900, "suncg", h=h)
    rgb = np.concatenate([d["rgb"]] * ((B + 3) // 4))[:B]
    u8, _ = rputil.sift_images(rgb, "second")
    rs = np.random.RandomState(0)
    E = 100
    grid = rputil.sift_grid_keypoints(w, h, 5)
    P = len(grid)
    kp = np.zeros((2 * B, E + P, 4), np.float32)
    kp[:, :, 2], kp[:, :, 3] = 5, -1
    kp[:, :E, 0], kp[:, :E, 1] = rs.randint(0, w, (2 * B, E)), rs.randint(0, h, (2 * B, E))
    kp[1::2, E:] = grid
    cnt = np.tile(np.array([E, E + P], np.int32), B)
    kp_d, cnt_d = torch.from_numpy(kp).to(dev), torch.from_numpy(cnt).to(dev)
    ms = timed(lambda: rputil.sift_describe_dev(u8, None, kp_d, cnt_d), args.reps)
    n_kp = int(cnt.sum())
    lines.append(f"relpose_sift_describe, 2 x {E} points + the step-5 grid ({P} points) per pair, size 5: {ms:.3f} ms per call, {n_kp} keypoints, "
                 f"{n_kp * 55 * 55 / ms / 1e6:.2f} G samples per second ({n_kp / ms / 1e3:.2f} M descriptors per second)")
    desc = rputil.sift_describe_dev(u8, None, kp_d, cnt_d)["desc"]

    ms = timed(lambda: rputil.sift_describe_grid_dev(u8, None, 1), args.reps)
    n_kp = 2 * B * h * w
    lines.append(f"relpose_sift_describe, the step-1 grid of every view, size 1: {ms:.3f} ms per call, {n_kp} keypoints, "
                 f"{n_kp * 11 * 11 / ms / 1e6:.2f} G samples per second ({n_kp / ms / 1e3:.2f} M descriptors per second)")

    src, tgt, dense = desc[0::2, :E].contiguous(), desc[1::2, :E].contiguous(), desc[1::2, E:].contiguous()
    ms = timed(lambda: descriptor.sift_rank_dev(src, tgt, dense), args.reps)
    ops = 2.0 * 128 * E * P * B
    count = descriptor.sift_rank_dev(src, tgt, dense)[0]
    lines.append(f"relpose_sift_rank, E = {E}, P = {P} (real descriptors): {ms:.3f} ms per call, {ops / ms / 1e9:.2f} TOP/s = "
                 f"{100 * ops / (ms * 1e-3) / PEAK_I8:.2f} % of the int8 matrix peak; mean ratio {float(count.double().mean()) / P:.4f}")
    del desc
    E2, P2 = 2000, h * w
    g = torch.Generator(device=dev).manual_seed(1)
    src, tgt, dense = (torch.randint(0, 256, (B, n, 128), device=dev, dtype=torch.uint8, generator=g) for n in (E2, E2, P2))
    ms = timed(lambda: descriptor.sift_rank_dev(src, tgt, dense), args.reps)
    ops = 2.0 * 128 * E2 * P2 * B
    lines.append(f"relpose_sift_rank, E = {E2}, P = {P2} (random bytes): {ms:.3f} ms per call, {ops / ms / 1e9:.2f} TOP/s = "
                 f"{100 * ops / (ms * 1e-3) / PEAK_I8:.2f} % of the int8 matrix peak ({B * P2 * 128 / 1e9:.2f} GB of grid descriptors, "
                 f"read {(E2 + 63) // 64} times)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
