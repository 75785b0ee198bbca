"""Milliseconds of the visibility check (csrc/visibility.hip, relpose_visibility) on three workloads, each ALTERNATING on the same GPU with
the same contract written with PyTorch operators (float64 tensors, one pass over all queries), and next to relpose_overlap on the same
(query, reference, pose) triples for context.

  pairs     32 SceneBatch SUNCG pairs (mined from multi-view scenes, so that the ground-truth pose means something) x 3 candidate poses at
            160 x 640: 192 directed queries of 25 600 points (util.pose_visibility_dev's queries)
  matrix    the 32 x 32 matrix of one 32-view scene: 992 directed queries of 25 600 points (util.visibility_matrix_dev)
  full      4 full-panorama clouds of 102 400 points (relpose_pano2pc's points) x 8 candidate poses: 32 queries (util.visibility_dev)

Wall-clock around synchronised calls (the call itself waits for its stream), one warm-up, --reps timed windows of 50 calls each for the
HIP call (3 for the others), the median per call over the windows and the spread (min .. max).  For the HIP call also the points per
second and the bytes it must move -- 25 B per point read (three f64 and the valid byte), 8 B gathered per point, and every panorama once
(4 B per pixel) -- over the call's time, as a share of the 8 TB/s HBM peak.  Kernel times come from a rocprofv3 --kernel-trace run of this
tool, in a run of its own.
Writes profiles/visibility_time.txt (--out to write elsewhere).

  python tools/visibility_time.py [--reps 5] [--out PATH]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def timed(fn, reps, inner=1):
    """(median, min, max) in ms per call, after one warm-up call"""
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def torch_visibility(pc, valid, depth, qc, rv, pose, dataset, tol_abs=0.05, tol_rel=0.02, radius=1):
    """The contract with PyTorch operators: -> counts [Q,6] int64.  Float64 tensor arithmetic (no fused multiply-add is asked for, none is
    excluded: the counts are compared with the kernel's and any difference is reported)."""
    import torch
    import torch.nn.functional as F
    V, h, w = depth.shape
    ok = torch.isfinite(depth) & (depth > 0)
    faces = depth.reshape(V, h, 4, h).permute(0, 2, 1, 3).reshape(V * 4, 1, h, h)
    okf = ok.reshape(V, h, 4, h).permute(0, 2, 1, 3).reshape(V * 4, 1, h, h)
    k = 2 * radius + 1
    big = torch.full_like(faces, float("inf"))
    dmax = F.max_pool2d(F.pad(torch.where(okf, faces, torch.zeros_like(faces)), (radius,) * 4, value=0.0), k, 1)
    dmin = -F.max_pool2d(F.pad(-torch.where(okf, faces, big), (radius,) * 4, value=-float("inf")), k, 1)
    back = lambda t: torch.where(okf, t, torch.zeros_like(t)).reshape(V, 4, h, h).permute(0, 2, 1, 3).reshape(V, h * w)
    dmin, dmax = back(dmin), back(dmax)
    qc = torch.as_tensor(np.asarray(qc), device=pc.device, dtype=torch.long)
    rv = torch.as_tensor(np.asarray(rv), device=pc.device, dtype=torch.long)
    p = pc[qc]                                                                  # [Q,P,3]
    va = torch.ones(p.shape[:2], dtype=torch.bool, device=pc.device) if valid is None else valid[qc] != 0
    q = torch.einsum("qij,qpj->qpi", pose[:, :3, :3], p) + pose[:, None, :3, 3]
    fin = torch.isfinite(q).all(-1)
    pix = torch.full(q.shape[:2], -1, dtype=torch.long, device=pc.device)
    d = torch.zeros(q.shape[:2], dtype=torch.float64, device=pc.device)
    x0, y0, z0 = q[..., 0], q[..., 1], q[..., 2]
    rot = ((x0, z0), (z0, -x0), (-x0, -z0), (-z0, x0))
    for slot in range(4):
        x, z = rot[(slot if "suncg" in dataset else slot + 3) & 3]
        az = z.abs() + 1e-32
        xn, yn = x / az, y0 / az
        hit = fin & (pix < 0) & (z < 0) & (xn.abs() < 1) & (yn.abs() < 1)
        cx = torch.round((xn + 1) * 0.5 * h).clamp(0, h - 1).long()
        cy = torch.round((1 - yn) * 0.5 * h).clamp(0, h - 1).long()
        pix = torch.where(hit, cy * w + slot * h + cx, pix)
        d = torch.where(hit, -z, d)
    on = va & (pix >= 0) & (d < 32768.0)
    idx = rv[:, None] * (h * w) + pix.clamp(min=0)
    lo32, hi32 = dmin.reshape(-1)[idx].double(), dmax.reshape(-1)[idx].double()
    seen = on & (lo32 > 0)
    lo = lo32 - (tol_abs + tol_rel * lo32)
    hi = hi32 + (tol_abs + tol_rel * hi32)
    cls = torch.zeros_like(pix)
    cls[va] = 1
    cls[on & ~seen] = 2
    cls[seen] = 3
    cls[seen & (d < lo)] = 4
    cls[seen & ~(d < lo) & (d > hi)] = 5
    return F.one_hot(cls, 6).sum(1)


def main():
    import torch
    from relativepose_amd import evaluation as E, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# python tools/visibility_time.py --reps {args.reps}, 1x MI355X (wall-clock per call over windows of synchronised calls after one warm-up -- 50 calls "
             "per window for hip, 3 for the others --, median (min .. max) over the windows; hip = one util.visibility_dev call (two launches), torch = the same contract with PyTorch "
             "operators, overlap = one util.overlap_dev call on the same triples)"]

    def report(name, pc, valid, depth, qc, rv, pose, ds):
        pose_d = torch.from_numpy(np.ascontiguousarray(pose)).to(dev)
        hip = lambda: util.visibility_dev(pc, valid, depth, qc, rv, pose_d, ds)
        tor = lambda: torch_visibility(pc, valid, depth, qc, rv, pose_d, ds)
        ovl = lambda: util.overlap_dev(pc, valid, qc, rv, pose_d)
        same = int((hip()[0].long() != tor()).any(1).sum())
        Q, P = len(qc), pc.shape[1]
        (m, lo, hi), (tm, tlo, thi) = timed(hip, args.reps, inner=50), timed(tor, args.reps, inner=3)
        nbytes = Q * P * (25 + 8) + depth.numel() * 4
        line = (f"{name}: hip {m:.3f} ms ({lo:.3f} .. {hi:.3f}), torch {tm:.2f} ms ({tlo:.2f} .. {thi:.2f}): {tm / m:.1f} x"
                f"{'' if tlo > hi else ' -- NOT faster beyond the spread'}; {Q} queries of {P} points = {Q * P / (m * 1e-3) / 1e9:.2f} G points/s; "
                f"{nbytes / 1e6:.1f} MB to move at least = {nbytes / (m * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (m * 1e-3) / HBM_PEAK:.2f} % of the "
                f"8 TB/s HBM peak; queries whose torch counts differ from the kernel's: {same} of {Q}")
        if pc.shape[0] == depth.shape[0]:
            om, olo, ohi = timed(ovl, args.reps, inner=3)
            line += f"; relpose_overlap on the same triples {om:.2f} ms ({olo:.2f} .. {ohi:.2f})"
        lines.append(line)
        c = hip()[0].sum(0).tolist()
        lines.append(f"    classes (invalid, outside, unobserved, consistent, violation, occluded) summed over the queries: {c}")

    # 1. pairs x candidates
    d = E.SceneBatch(32, 4000, "suncg", "second", 1, views=6, balanced=True).take(range(32))
    depth = torch.from_numpy(np.ascontiguousarray(d["depth"].reshape(64, 160, 640))).to(dev)
    pc, valid = util.depth2pc_dev(depth, "suncg")
    rs = np.random.RandomState(1)
    T = np.empty((32, 3, 4, 4))
    for b in range(32):
        gt = np.matmul(d["R"][b, 1], np.linalg.inv(d["R"][b, 0]))
        T[b] = [gt, np.matmul(synth.random_rigid(rs, 0.6, 0.5), gt), np.matmul(synth.random_rigid(rs, 0.1, 0.1), gt)]
    qc = np.repeat(np.arange(64).reshape(32, 1, 2), 3, 1).reshape(-1)
    rv = qc ^ 1
    pose = np.stack([T, np.linalg.inv(T)], 2).reshape(-1, 4, 4)
    report("pairs (32 SUNCG pairs x 3 candidates)", pc, valid, depth, qc, rv, pose, "suncg")
    got = util.pose_visibility_dev(pc, valid, depth, T, "suncg")[2]["agreement"].cpu().numpy()
    lines.append(f"    pooled agreement, mean over the pairs: true pose {got[:, 0].mean():.4f}, perturbed by (0.6 rad, 0.5) {got[:, 1].mean():.4f}, "
                 f"by (0.1 rad, 0.1) {got[:, 2].mean():.4f}; select_pose picks the true pose in "
                 f"{int((np.nanargmax(np.nan_to_num(got, nan=-1.0), 1) == 0).sum())} of 32 pairs (against the FULL rendered panoramas)")
    # 2. one scene's matrix
    sc = synth.render_scene(77, 32, "suncg")
    depth = torch.from_numpy(sc["depth"]).to(dev)
    pc, valid = util.depth2pc_dev(depth, "suncg")
    ij = [(i, j) for i in range(32) for j in range(32) if i != j]
    inv = [np.linalg.inv(sc["R"][i]) for i in range(32)]
    report("matrix (one 32-view scene)", pc, valid, depth, np.array([i for i, _ in ij]), np.array([j for _, j in ij]),
           np.stack([np.matmul(sc["R"][j], inv[i]) for i, j in ij]), "suncg")
    # 3. full panoramas
    depth = depth[:4].contiguous()
    pc3, va = util.pano2pc_dev(depth, "suncg")                                   # [4,3,P], [4,P]
    pc = pc3.transpose(1, 2).contiguous()
    qc = np.repeat(np.arange(4), 8)
    rv = (qc + 1 + np.arange(32) % 3) % 4
    pose = np.stack([np.matmul(synth.random_rigid(np.random.RandomState(9 + k), 0.1 * (k % 8), 0.1 * (k % 8)),
                               np.matmul(sc["R"][rv[k]], inv[qc[k]])) for k in range(32)])
    report("full (4 full-panorama clouds x 8 candidates)", pc, va, depth, qc, rv, pose, "suncg")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
