"""Milliseconds of frame-to-model alignment (csrc/tsdfalign.hip, relpose_tsdf_align) on two workloads, each ALTERNATING on the same GPU with
the same contract written with PyTorch operators (float64 tensors, int64 sums, a batched eigh for the 6 x 6):

  pairs     64 views at 160 x 640 against 32 pair volumes of 128^3 voxels (view 2b and 2b + 1 against volume b)
  scene     32 views at 160 x 640 against one scene of 256 x 256 x 128 voxels

12 iterations (13 evaluations) each, every pose started random_rigid(0.05, 0.05) away from the truth.  Every workload runs in a child process
of its own under a time limit of its own (--limit seconds); the parent never opens the GPU, and a step that fails or runs out of time ends
the tool.  Wall-clock around synchronised calls (the call waits for its stream), one warm-up, --reps timed windows, the median per call over
the windows and the spread (min .. max).  For the HIP call also
  per evaluation   (t(12 iterations) - t(0 iterations)) / 12: one accumulate launch and one step launch
  step alone       the same call with a stride that leaves one pixel per view: the accumulate kernel has nothing to do, what remains is the
                   13 step launches (one wave per view: the serial Jacobi) and the launch overhead
  bytes            what an evaluation must read: 4 B per sampled pixel and the touched cells once (8 B per distinct corner voxel, counted at
                   the start poses), and their share of the 8 TB/s HBM peak -- a bound from below: the volumes of these workloads fit the
                   last-level cache, so the kernel need not be reading HBM at all
Writes profiles/align_time.txt (--out to write elsewhere).

  python tools/align_time.py [--reps 5] [--limit 300] [--out PATH]"""
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
ITERS = 12


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


def torch_points(depth, dataset):
    """-> (p [V,N,3] f64 camera points of every pixel, ok [V,N] bool)"""
    import torch
    V, h, w = depth.shape
    dev = depth.device
    row, col = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    slot, px = col // h, col % h
    xn = (2.0 * px.double()) / float(h) - 1.0
    yn = 1.0 - (2.0 * row.double()) / float(h)
    D = depth.double()
    fx, fy, fz = xn * D, yn * D, -D
    k = (slot if "suncg" in dataset else (slot + 3) & 3)[None].expand(V, h, w)
    x = torch.where(k == 0, fx, torch.where(k == 1, -fz, torch.where(k == 2, -fx, fz)))
    z = torch.where(k == 0, fz, torch.where(k == 1, fx, torch.where(k == 2, -fz, -fx)))
    ok = torch.isfinite(depth) & (depth > 0)
    return torch.stack([x, fy, z], -1).reshape(V, h * w, 3), ok.reshape(V, h * w)


def torch_align(ts, wt, origin, dims, voxel, p, ok, pose, sov, iters, eig_min, cells=None):
    """The alignment contract with PyTorch operators -> (pose [V,4,4], sums [V,32] int64 of the last evaluation).  The per-point rule follows
    the contract statement by statement in float64 tensor arithmetic; the 6 x 6 is solved by torch.linalg.eigh instead of the fixed Jacobi
    sweeps, so the poses agree to rounding, not bit for bit (the difference is reported)."""
    import torch
    nx, ny, nz = dims
    dev = p.device
    V = p.shape[0]
    o = origin[sov]                                                  # [V,3]
    c = o + (torch.tensor(dims, dtype=torch.float64, device=dev) * 0.5) * voxel
    base = (sov.long() * (nx * ny * nz))[:, None]
    tsf, wtf = ts.reshape(-1), wt.reshape(-1)
    T = pose.clone()
    scale = torch.tensor([256.0] * 3 + [65536.0] * 3, dtype=torch.float64, device=dev)
    iu = torch.triu_indices(6, 6, device=dev)
    for e in range(iters + 1):
        Rm, t = T[:, :3, :3], T[:, :3, 3]
        W, w3 = Rm.transpose(1, 2), -torch.einsum("vba,vb->va", Rm, t)
        q = torch.einsum("vab,vnb->vna", W, p) + w3[:, None]
        u = (q - o[:, None]) / voxel - 0.5
        fl = torch.floor(u)
        lim = torch.tensor([nx - 2, ny - 2, nz - 2], dtype=torch.float64, device=dev)
        inside = ok & torch.isfinite(q).all(-1) & ((fl >= 0) & (fl <= lim)).all(-1)
        i0 = torch.where(inside[..., None], fl, torch.zeros_like(fl)).long()
        f = u - fl
        tc, known = [], inside.clone()
        for cn in range(8):
            lin = base + ((i0[..., 2] + (cn >> 2 & 1)) * ny + (i0[..., 1] + (cn >> 1 & 1))) * nx + (i0[..., 0] + (cn & 1))
            if cells is not None:
                cells.append(lin[inside])
            w = wtf[lin]
            k = w >= 1
            known &= k
            tc.append(torch.where(k, tsf[lin].double() / (32768.0 * torch.where(k, w, torch.ones_like(w)).double()), torch.zeros_like(q[..., 0])))
        tc = torch.stack(tc, -1)
        sat = known & (tc.abs() >= 1.0).any(-1)
        use = known & ~sat
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        d00, d10, d01, d11 = tc[..., 1] - tc[..., 0], tc[..., 3] - tc[..., 2], tc[..., 5] - tc[..., 4], tc[..., 7] - tc[..., 6]
        a00, a10, a01, a11 = tc[..., 0] + fx * d00, tc[..., 2] + fx * d10, tc[..., 4] + fx * d01, tc[..., 6] + fx * d11
        c0, c1 = a10 - a00, a11 - a01
        b0, b1 = a00 + fy * c0, a01 + fy * c1
        gz = b1 - b0
        r = b0 + fz * gz
        gy = c0 + fz * (c1 - c0)
        e0, e1 = d00 + fy * (d10 - d00), d01 + fy * (d11 - d01)
        gx = e0 + fz * (e1 - e0)
        l = (q - c[:, None]) / voxel
        J = torch.stack([l[..., 1] * gz - l[..., 2] * gy, l[..., 2] * gx - l[..., 0] * gz, l[..., 0] * gy - l[..., 1] * gx, gx, gy, gz], -1)
        m = use[..., None]
        Jq = torch.where(m, torch.round(J * scale), torch.zeros_like(J)).long()
        rq = torch.where(use, torch.round(r * 65536.0), torch.zeros_like(r)).long()
        A = torch.einsum("vni,vnj->vij", Jq.double(), Jq.double())          # exact while the sums stay below 2^53, which these workloads do
        bq = torch.einsum("vni,vn->vi", Jq.double(), rq.double())
        n_used = use.sum(1)
        sums = torch.cat([A[:, iu[0], iu[1]].long(), bq.long(), (rq * rq).sum(1, keepdim=True),
                          (ok & ~inside).sum(1, keepdim=True), (inside & ~known).sum(1, keepdim=True), sat.sum(1, keepdim=True), n_used[:, None]], 1)
        if e == iters:
            return T, sums
        A = A / (scale[:, None] * scale[None])
        b = bq / (scale * 65536.0)
        lam, Vec = torch.linalg.eigh(A)
        keep = (lam > eig_min * n_used[:, None].double()) & (n_used[:, None] >= 6)
        coef = torch.where(keep, -torch.einsum("vik,vi->vk", Vec, b) / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
        delta = torch.einsum("vik,vk->vi", Vec, coef)
        a = delta[:, :3] * 0.5
        aa = (a * a).sum(1)
        K = torch.zeros(V, 3, 3, dtype=torch.float64, device=dev)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
        eye = torch.eye(3, dtype=torch.float64, device=dev)[None]
        Rd = ((1.0 - aa)[:, None, None] * eye + 2.0 * a[:, :, None] * a[:, None, :] + 2.0 * K) / (1.0 + aa)[:, None, None]
        d = c - torch.einsum("vij,vj->vi", Rd, c) + voxel * delta[:, 3:]
        Rn = Rm @ Rd.transpose(1, 2)
        Tn = T.clone()
        Tn[:, :3, :3], Tn[:, :3, 3] = Rn, t - torch.einsum("vij,vj->vi", Rn, d)
        T = torch.where((n_used >= 6)[:, None, None], Tn, T)


def workload(step):
    """-> (name, depth, R true, R start, scene_of_view, view_begin of the fusion, origin, dims, voxel) on the host"""
    from relativepose_amd import synth
    rs = np.random.RandomState(5)
    jolt = lambda R: np.stack([np.matmul(synth.random_rigid(rs, 0.05, 0.05), T) for T in R])
    if step == "pairs":
        depth, R, origin = [], [], []
        for b in range(32):
            sc = synth.render_scene(4000 + b, 2, "suncg")
            depth.append(sc["depth"]), R.append(sc["R"])
            origin.append(-64 * 0.0625 * np.ones(3))
        R = np.concatenate(R)
        return ("pairs (64 views against 32 volumes of 128^3)", np.concatenate(depth), R, jolt(R), np.repeat(np.arange(32, dtype=np.int32), 2),
                np.arange(0, 65, 2, dtype=np.int32), np.stack(origin), (128, 128, 128), 0.0625)
    sc = synth.render_scene(77, 32, "suncg")
    dims = (256, 256, 128)
    voxel = float(np.max(2 * (sc["half"] + 0.1) / np.array(dims)))
    return ("scene (32 views against one volume of 256 x 256 x 128)", sc["depth"], sc["R"], jolt(sc["R"]), np.zeros(32, np.int32),
            np.array([0, 32], np.int32), (-0.5 * voxel * np.array(dims))[None], dims, voxel)


def run_step(step, reps):
    import torch
    from relativepose_amd import _lib, util
    dev = torch.device("cuda", 0)
    name, depth, R, R0, sov, vb, origin, dims, voxel = workload(step)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    depth, pose0 = up(depth, np.float32), up(R0, np.float64)
    V, h = depth.shape[0], depth.shape[1]
    state = util.tsdf_fuse_dev(depth, None, R, vb, origin, dims, voxel, "suncg")
    eig_min = _lib.TSDF_ALIGN_EIG_MIN
    hip = lambda: util.tsdf_align_dev(state, depth, pose0, sov, ITERS)
    hip0 = lambda: util.tsdf_align_dev(state, depth, pose0, sov, 0)
    hip_step = lambda: util.tsdf_align_dev(state, depth, pose0, sov, ITERS, stride=4 * h * h)
    p, ok = torch_points(depth, "suncg")
    org, sovd = up(origin, np.float64), up(sov, np.int64)
    cells = []
    torch_align(state["tsdf_sum"], state["weight"], org, dims, voxel, p, ok, pose0, sovd, 0, eig_min, cells)
    touched = int(torch.unique(torch.cat(cells)).numel())
    del cells
    tor = lambda: torch_align(state["tsdf_sum"], state["weight"], org, dims, voxel, p, ok, pose0, sovd, ITERS, eig_min)
    got, (t_pose, t_sums) = hip(), tor()
    pose_diff = float((got["pose"] - t_pose).abs().max().item())
    first = hip0()
    sums_same = bool(torch.equal(first["sums"], torch_align(state["tsdf_sum"], state["weight"], org, dims, voxel, p, ok, pose0, sovd, 0, eig_min)[1]))
    rms = got["rms"].cpu().numpy()
    err = lambda P: float(np.median([np.linalg.norm(np.linalg.inv(P[v])[:3, 3] - np.linalg.inv(R[v])[:3, 3]) for v in range(V)])) / voxel
    (m, lo, hi), (m0, lo0, hi0), (ms, los, his) = timed(hip, reps, inner=3), timed(hip0, reps, inner=3), timed(hip_step, reps, inner=3)
    tm, tlo, thi = timed(tor, max(2, reps // 2))
    per = (m - m0) / ITERS
    nbytes = V * h * 4 * h * 4 + touched * 8
    print(f"{name}, {ITERS} iterations: hip {m:.3f} ms ({lo:.3f} .. {hi:.3f}), torch {tm:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tm / m:.1f} x"
          f"{'' if tlo > hi else ' -- NOT faster beyond the spread'}; 0 iterations (one evaluation): {m0:.3f} ms ({lo0:.3f} .. {hi0:.3f}); per further "
          f"evaluation {per * 1e3:.1f} us; one pixel per view (13 step launches, no accumulation to speak of): {ms:.3f} ms ({los:.3f} .. {his:.3f}) = "
          f"{ms / (ITERS + 1) * 1e3:.1f} us per evaluation, so the accumulate kernel takes about {(per - ms / (ITERS + 1)) * 1e3:.1f} us of each; "
          f"{V * h * 4 * h / 1e6:.2f} M points, {touched / 1e6:.2f} M distinct corner voxels: {nbytes / 1e6:.1f} MB to read at least per evaluation = "
          f"{nbytes / (per * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (per * 1e-3) / HBM_PEAK:.2f} % of the 8 TB/s HBM peak; "
          f"median camera-centre error {err(R0):.3f} -> {err(got['pose'].cpu().numpy()):.3f} voxels, median rms residual {np.median(rms[:, 0]):.4f} -> "
          f"{np.median(rms[:, 1]):.4f} trunc, views with held directions {int((got['held'] > 0).sum().item())} of {V}; "
          f"first evaluation's integer sums equal torch's: {sums_same}; largest difference of a refined pose entry against torch (eigh, not Jacobi): "
          f"{pose_diff:.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.txt"))
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args.reps)
        return
    lines = [f"# python tools/align_time.py --reps {args.reps}, 1x MI355X (wall-clock per call over windows of synchronised calls after one warm-up -- 3 calls "
             "per window for hip, 1 for torch --, median (min .. max) over the windows; hip = one util.tsdf_align_dev call (26 launches), torch = the same "
             "contract with PyTorch operators, all views at once)"]
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
