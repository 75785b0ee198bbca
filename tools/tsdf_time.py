"""Milliseconds of TSDF fusion and surface extraction (csrc/tsdf.hip, relpose_tsdf_fuse / relpose_tsdf_surface) on two workloads, each
ALTERNATING on the same GPU with the same contract written with PyTorch operators (float64 tensors, one scene at a time so that the
intermediates fit):

  pairs     32 pair volumes of 128^3 voxels with 2 views each at 160 x 640 (what evaluate_pairs(fuse=...) fuses per batch, at a finer voxel)
  scene     one scene of 256 x 256 x 128 voxels with 32 views at 160 x 640

Every workload runs in a child process of its own under a time limit of its own (--limit seconds); the parent never opens the GPU, and a
step that fails or runs out of time ends the tool.  Wall-clock around synchronised calls (the calls wait for their stream), one warm-up,
--reps timed windows, the median per call over the windows and the spread (min .. max).  For the HIP calls also the bytes each kernel must
move and their share of the 8 TB/s HBM peak:
  fuse      every voxel's state written once (8 B, 20 B with colours) and every panorama read once (4 B per pixel, 16 B with colours); the
            per-view gathers hit pixels a neighbouring lane or an earlier view of the chunk already brought in
  surface   the state read twice (count pass, write pass: 8 B per voxel each; the neighbours a voxel reads are its workgroup's or the next
            row's) and 52 B per crossing written (point, normal, valid; 64 B with colours)
Writes profiles/tsdf_time.txt (--out to write elsewhere).

  python tools/tsdf_time.py [--reps 5] [--limit 300] [--out PATH]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
STEPS = ("pairs", "scene")


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


def torch_fuse(depth, rgb, pose, view_begin, origin, dims, voxel, dataset, trunc):
    """The fuse contract with PyTorch operators -> (tsdf_sum, weight, color_sum) int64 / int64 / int64.  Float64 tensor arithmetic (no fused
    multiply-add is asked for, none is excluded: the result is compared with the kernel's and any difference is reported)."""
    import torch
    dev = depth.device
    nx, ny, nz = dims
    S, h = len(view_begin) - 1, depth.shape[1]
    w = 4 * h
    ts = torch.zeros(S, nz * ny * nx, dtype=torch.int64, device=dev)
    wt = torch.zeros_like(ts)
    cs = None if rgb is None else torch.zeros(S, 3, nz * ny * nx, dtype=torch.int64, device=dev)
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing="ij")
    idx = [v.reshape(-1).double() + 0.5 for v in (i, j, k)]
    for s in range(S):
        c = [float(origin[s][a]) + idx[a] * voxel for a in range(3)]
        for v in range(view_begin[s], view_begin[s + 1]):
            T = pose[v]
            q = [((T[a, 0] * c[0] + T[a, 1] * c[1]) + T[a, 2] * c[2]) + T[a, 3] for a in range(3)]
            fin = torch.isfinite(q[0]) & torch.isfinite(q[1]) & torch.isfinite(q[2])
            pix = torch.full_like(q[0], -1, dtype=torch.long)
            d = torch.zeros_like(q[0])
            rot = ((q[0], q[2]), (q[2], -q[0]), (-q[0], -q[2]), (-q[2], q[0]))
            for slot in range(4):
                x, z = rot[(slot if "suncg" in dataset else slot + 3) & 3]
                az = z.abs() + 1e-32
                xn, yn = x / az, q[1] / az
                hit = fin & (pix < 0) & (z < 0) & (xn.abs() < 1) & (yn.abs() < 1)
                cx = torch.round((xn + 1) * 0.5 * h).clamp(0, h - 1).long()
                cy = torch.round((1 - yn) * 0.5 * h).clamp(0, h - 1).long()
                pix = torch.where(hit, cy * w + slot * h + cx, pix)
                d = torch.where(hit, -z, d)
            on = (pix >= 0) & (d < 32768.0)
            pi = pix.clamp(min=0)
            D = depth[v].reshape(-1)[pi]
            ok = on & torch.isfinite(D) & (D > 0)
            sdf = D.double() - d
            ok &= ~(sdf < -trunc)
            t = torch.clamp(sdf / trunc, max=1.0)
            ts[s] += torch.where(ok, torch.round(t * 32768.0), torch.zeros_like(t)).long()
            wt[s] += ok.long()
            if rgb is not None:
                col = torch.nan_to_num(rgb[v].reshape(3, -1)[:, pi], nan=0.0).clamp(0.0, 1.0)
                cs[s] += torch.where(ok[None], torch.round(col * 255.0), torch.zeros_like(col)).long()
    shape = (S, nz, ny, nx)
    return ts.reshape(shape), wt.reshape(shape), None if cs is None else cs.reshape(S, 3, nz, ny, nx)


def _shift(a, c, d, fill):
    import torch
    ax = a.dim() - 1 - c
    out = torch.full_like(a, fill)
    n = a.shape[ax]
    if n > 1:
        if d > 0:
            out.narrow(ax, 0, n - 1).copy_(a.narrow(ax, 1, n - 1))
        else:
            out.narrow(ax, 1, n - 1).copy_(a.narrow(ax, 0, n - 1))
    return out


def torch_surface(ts, wt, cs, origin, voxel, min_weight=1):
    """The surface contract with PyTorch operators, one scene at a time -> [(points [n,3], normals [n,3], colors [n,3] or None)] per scene,
    in the contract's order."""
    import torch
    out = []
    S, nz, ny, nx = ts.shape
    dev = ts.device
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing="ij")
    idx = [v.double() + 0.5 for v in (i, j, k)]
    lin = ((k * ny + j) * nx + i).reshape(-1)
    for s in range(S):
        known = wt[s] >= min_weight
        wd = torch.where(known, wt[s], torch.ones_like(wt[s])).double()
        t = torch.where(known, ts[s].double() / (32768.0 * wd), torch.zeros_like(wd))
        g = []
        for c in range(3):
            tp, tm, kp, km = _shift(t, c, 1, 0.0), _shift(t, c, -1, 0.0), _shift(known, c, 1, False), _shift(known, c, -1, False)
            g.append(torch.where(kp & km, (tp - tm) * 0.5, torch.where(kp, tp - t, torch.where(km, t - tm, torch.zeros_like(t)))))
        ctr = [float(origin[s][a]) + idx[a] * voxel for a in range(3)]
        keys, pts, nrm, cols = [], [], [], []
        for c in range(3):
            tb, kb = _shift(t, c, 1, 0.0), _shift(known, c, 1, False)
            m = (known & kb & (((t >= 0) & (tb < 0)) | ((t < 0) & (tb >= 0)))).reshape(-1)
            sel = lambda a: a.reshape(-1)[m]
            ta, tbs = sel(t), sel(tb)
            sc = ta / (ta - tbs)
            n = torch.stack([sel(g[a]) + sc * (sel(_shift(g[a], c, 1, 0.0)) - sel(g[a])) for a in range(3)], 1)
            nn = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).unsqueeze(1)
            nrm.append(torch.where(nn > 0, n / torch.where(nn > 0, nn, torch.ones_like(nn)), n))
            p = [sel(ctr[a]) for a in range(3)]
            p[c] = float(origin[s][c]) + (sel(idx[c]) + sc) * voxel
            pts.append(torch.stack(p, 1))
            keys.append(lin[m] * 3 + c)
            if cs is not None:
                col = [cs[s, ch].double() / (255.0 * wd) for ch in range(3)]
                cols.append(torch.stack([sel(col[ch]) + sc * (sel(_shift(col[ch], c, 1, 0.0)) - sel(col[ch])) for ch in range(3)], 1).float())
        order = torch.argsort(torch.cat(keys))
        out.append((torch.cat(pts)[order], torch.cat(nrm)[order], None if cs is None else torch.cat(cols)[order]))
    return out


def workload(step):
    """-> (name, depth, rgb, R, view_begin, origin, dims, voxel) on the host"""
    from relativepose_amd import synth
    if step == "pairs":
        depth, rgb, R, origin = [], [], [], []
        for b in range(32):
            sc = synth.render_scene(4000 + b, 2, "suncg")
            depth.append(sc["depth"]), rgb.append(sc["rgb"]), R.append(sc["R"])
            origin.append(-64 * 0.0625 * np.ones(3))
        return ("pairs (32 volumes of 128^3, 2 views each)", np.concatenate(depth), np.concatenate(rgb), np.concatenate(R),
                np.arange(0, 65, 2, dtype=np.int32), np.stack(origin), (128, 128, 128), 0.0625)
    sc = synth.render_scene(77, 32, "suncg")
    dims = (256, 256, 128)
    voxel = float(np.max(2 * (sc["half"] + 0.1) / np.array(dims)))
    return ("scene (one volume of 256 x 256 x 128, 32 views)", sc["depth"], sc["rgb"], sc["R"], np.array([0, 32], np.int32),
            (-0.5 * voxel * np.array(dims))[None], dims, voxel)


def run_step(step, reps):
    import torch
    from relativepose_amd import util
    dev = torch.device("cuda", 0)
    name, depth, rgb, R, vb, origin, dims, voxel = workload(step)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    depth, rgb, pose = up(depth, np.float32), up(rgb, np.float32), up(R, np.float64)
    S, V, h = len(vb) - 1, depth.shape[0], depth.shape[1]
    nvox = dims[0] * dims[1] * dims[2]
    trunc = 4 * voxel
    lines = []
    for colours in (True, False):
        col = rgb if colours else None
        state = util.tsdf_fuse_dev(depth, col, pose, vb, origin, dims, voxel, "suncg")
        hip = lambda: util.tsdf_fuse_dev(depth, col, pose, vb, origin, dims, voxel, "suncg", state=None)
        tor = lambda: torch_fuse(depth, col, pose, vb.tolist(), origin, dims, voxel, "suncg", trunc)
        t_ts, t_wt, t_cs = tor()
        diff = int(((t_ts != state["tsdf_sum"].long()) | (t_wt != state["weight"].long())).sum())
        if colours:
            diff_c = int((t_cs != state["color_sum"].long()).any(1).sum())
        del t_ts, t_wt, t_cs
        (m, lo, hi), (tm, tlo, thi) = timed(hip, reps, inner=3), timed(tor, max(2, reps // 2))
        nbytes = S * nvox * (20 if colours else 8) + V * h * 4 * h * (16 if colours else 4)
        updates = sum(int(vb[s + 1] - vb[s]) for s in range(S)) * nvox
        lines.append(f"{name}, fuse {'with' if colours else 'without'} colours: hip {m:.3f} ms ({lo:.3f} .. {hi:.3f}), torch {tm:.1f} ms ({tlo:.1f} .. {thi:.1f}): "
                     f"{tm / m:.1f} x{'' if tlo > hi else ' -- NOT faster beyond the spread'}; {updates / 1e6:.1f} M voxel-view updates = "
                     f"{updates / (m * 1e-3) / 1e9:.2f} G updates/s; {nbytes / 1e6:.1f} MB to move at least = {nbytes / (m * 1e-3) / 1e12:.3f} TB/s = "
                     f"{100 * nbytes / (m * 1e-3) / HBM_PEAK:.2f} % of the 8 TB/s HBM peak; voxels whose torch sums differ from the kernel's: {diff} of {S * nvox}"
                     + (f" (colours: {diff_c})" if colours else ""))
        # surface
        n_pts = util.tsdf_surface_dev(state, 1, 1)[4]
        n_all, cap = int(n_pts.sum().item()), max(1, int(n_pts.max().item()))
        hip_s = lambda: util.tsdf_surface_dev(state, 1, cap)
        cs_l = None if state["color_sum"] is None else state["color_sum"].long()
        tor_s = lambda: torch_surface(state["tsdf_sum"].long(), state["weight"].long(), cs_l, origin, voxel)
        got, ref = hip_s(), tor_s()
        bad, dn = 0, 0.0
        for s in range(S):
            n = int(n_pts[s].item())
            same = ref[s][0].shape[0] == n and torch.equal(got[0][s, :n], ref[s][0])
            bad += 0 if same else 1
            if same and n:
                dn = max(dn, float((got[1][s, :n] - ref[s][1]).abs().max().item()))
        del got, ref
        (m, lo, hi), (tm, tlo, thi) = timed(hip_s, reps, inner=3), timed(tor_s, max(2, reps // 2))
        nbytes = 2 * S * nvox * 8 + n_all * (64 if colours else 52)
        lines.append(f"{name}, surface {'with' if colours else 'without'} colours: hip {m:.3f} ms ({lo:.3f} .. {hi:.3f}), torch {tm:.1f} ms ({tlo:.1f} .. {thi:.1f}): "
                     f"{tm / m:.1f} x{'' if tlo > hi else ' -- NOT faster beyond the spread'}; {n_all} crossings (cap {cap} per scene); "
                     f"{nbytes / 1e6:.1f} MB to move at least = {nbytes / (m * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (m * 1e-3) / HBM_PEAK:.2f} % of the "
                     f"8 TB/s HBM peak; scenes whose torch points differ bitwise from the kernel's: {bad} of {S}; largest difference of a normal component {dn:.1e}")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_time.txt"))
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args.reps)
        return
    lines = [f"# python tools/tsdf_time.py --reps {args.reps}, 1x MI355X (wall-clock per call over windows of synchronised calls after one warm-up -- 3 calls per "
             "window for hip, 1 for torch --, median (min .. max) over the windows; hip = one util.tsdf_fuse_dev / util.tsdf_surface_dev call (one / three "
             "launches), torch = the same contract with PyTorch operators, scene by scene)"]
    for step in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)], capture_output=True, text=True,
                           timeout=args.limit, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"step {step} ended with status {r.returncode}: nothing more is started")
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
