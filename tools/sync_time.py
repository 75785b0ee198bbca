"""Milliseconds of pose-graph synchronisation (csrc/posesync.hip, relpose_pose_sync) on two workloads, each ALTERNATING on the same GPU with
the same contract written with PyTorch operators, and against the numpy model (tests/sync_model.py) on the host:

  rooms     64 scenes of 8 views and 84 edges each (28 pairs x 3 competing poses; a quarter of the edges are outliers)
  hall      one scene of 64 views and 4096 edges (a chain, random extra edges and duplicates; a tenth of the edges are outliers)

The call is latency-bound by construction: per iteration a Cholesky factorisation of M dependent columns (two barriers each) and two
substitutions of 2 M dependent steps each; nothing here is compared with a roofline.  What the time is made of is measured instead: `hall`
is run again with its 63 chain edges alone -- the same 64 x 64 factorisation, substitutions and Prim steps, next to no per-edge work --
and the dependent steps are counted from the code: iterations x (2 M column phases + 4 M substitution steps) + M Prim steps.

Every workload runs in a child process of its own under a time limit of its own (--limit seconds); the parent never opens the GPU, and a
step that fails or runs out of time ends the tool.  Wall-clock around synchronised calls, one warm-up, --reps timed windows, the median per
call over the windows and the spread (min .. max).  torch = the iterations of the contract with PyTorch operators, batched over the scenes
(index_add_ assembly, torch.linalg.cholesky, torch.cholesky_solve); its spanning-tree initialisation is taken from the model and not timed.
Writes profiles/sync_time.txt (--out to write elsewhere).

  python tools/sync_time.py [--reps 5] [--limit 300] [--out PATH]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ("rooms", "hall")


def timed(fn, reps, inner=1, sync=True):
    """(median, min, max) in ms per call, after one warm-up call"""
    import torch
    fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def graph(rs, M, pairs, outlier_share):
    from relativepose_amd import synth
    G = np.stack([synth.random_rigid(rs, np.pi, 2.0) for _ in range(M)])
    T = np.stack([np.matmul(G[j], np.linalg.inv(G[i])) for i, j in pairs])
    bad = rs.rand(len(pairs)) < outlier_share
    for e in np.nonzero(bad)[0]:
        T[e] = synth.random_rigid(rs, np.pi, 2.0)
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32), T, G, bad


def workload(step):
    """-> (name, scenes [(M, src, dst, T, G, bad)])"""
    rs = np.random.RandomState(4000)
    if step == "rooms":
        pairs = [(i, j) for i in range(8) for j in range(i + 1, 8) for _ in range(3)]
        return "rooms (64 scenes x 8 views x 84 edges)", [(8,) + graph(rs, 8, pairs, 0.25) for _ in range(64)]
    pairs = [(v, v + 1) for v in range(63)]
    while len(pairs) < 3500:
        i, j = rs.randint(0, 64, 2)
        if i != j:
            pairs.append((int(i), int(j)))
    pairs += [pairs[k] for k in rs.randint(63, 3500, 4096 - 3500)]
    src, dst, T, G, bad = graph(rs, 64, pairs, 0.1)
    for e in range(63):                                            # the chain stays exact: `hall` without the other edges is solvable
        T[e], bad[e] = np.matmul(G[e + 1], np.linalg.inv(G[e])), False
    return "hall (1 scene x 64 views x 4096 edges)", [(64, src, dst, T, G, bad)]


def batch_of(scenes):
    return (np.concatenate([s[3] for s in scenes]), np.concatenate([s[1] for s in scenes]), np.concatenate([s[2] for s in scenes]),
            np.ones(sum(len(s[1]) for s in scenes)), np.cumsum([0] + [s[0] for s in scenes]).astype(np.int32),
            np.cumsum([0] + [len(s[1]) for s in scenes]).astype(np.int32))


def torch_sync(R0, u0, gauge, src, dst, T, w0, mus, sr2=0.01, st2=0.01):
    """The iterations of the contract for S scenes of the same M and E with PyTorch operators: R0 [S,M,3,3], u0 [S,M,3] the spanning tree's
    poses, gauge [S,M] bool, src / dst [S,E] long, T [S,E,4,4], w0 [S,E] -> (pose [S,M,4,4], confidence [S,E])."""
    import torch
    S, M = gauge.shape
    E = src.shape[1]
    R, u = R0.clone(), u0.clone()
    Rij, tij = T[:, :, :3, :3], T[:, :, :3, 3]
    bi = torch.arange(S, device=R.device)[:, None].expand(S, E)
    free = (~gauge)[bi, src] & (~gauge)[bi, dst]
    eye = torch.eye(M, dtype=torch.float64, device=R.device)
    g3 = gauge[:, :, None]

    def log(Em):
        v = torch.stack([Em[..., 2, 1] - Em[..., 1, 2], Em[..., 0, 2] - Em[..., 2, 0], Em[..., 1, 0] - Em[..., 0, 1]], -1)
        n = v.norm(dim=-1)
        c = (Em[..., 0, 0] + Em[..., 1, 1] + Em[..., 2, 2] - 1.0) * 0.5
        th = torch.atan2(n * 0.5, c)
        f = torch.where(n < 1e-6, torch.full_like(n, 0.5), th / n.clamp(min=1e-300))
        return v * f[..., None]

    def exp(d):
        t2 = (d * d).sum(-1)
        th = t2.sqrt()
        small = t2 < 1e-8
        ths = torch.where(small, torch.ones_like(th), th)
        A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(ths) / ths)
        B = torch.where(small, 0.5 - t2 / 24.0, 2.0 * torch.sin(ths * 0.5) ** 2 / torch.where(small, torch.ones_like(t2), t2))
        K = torch.zeros(d.shape[:-1] + (3, 3), dtype=d.dtype, device=d.device)
        K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
        return torch.eye(3, dtype=d.dtype, device=d.device) + A[..., None, None] * K + B[..., None, None] * (K @ K)

    def rhs(vec, w):
        b = torch.zeros(S, M, 3, dtype=torch.float64, device=R.device)
        wv = w[..., None] * vec
        b.index_put_((bi, dst), wv, accumulate=True)
        b.index_put_((bi, src), -wv, accumulate=True)
        return torch.where(g3, torch.zeros_like(b), b)

    conf = torch.ones_like(w0)
    for mu in mus:
        Ri, Rj = R[bi, src], R[bi, dst]
        om = log(Rj.transpose(-1, -2) @ (Rij @ Ri))
        rho = (Rj.transpose(-1, -2) @ tij[..., None])[..., 0] - (u[bi, dst] - u[bi, src])
        q = 1.0 + ((om * om).sum(-1) / sr2 + (rho * rho).sum(-1) / st2) / (mu * mu)
        conf = 1.0 / (q * q)
        w = w0 * conf
        L = torch.zeros(S, M, M, dtype=torch.float64, device=R.device)
        wf = torch.where(free, w, torch.zeros_like(w))
        L.index_put_((bi, src, dst), -wf, accumulate=True)
        L.index_put_((bi, dst, src), -wf, accumulate=True)
        diag = torch.zeros(S, M, dtype=torch.float64, device=R.device)
        diag.index_put_((bi, src), w, accumulate=True)
        diag.index_put_((bi, dst), w, accumulate=True)
        L = L + torch.diag_embed(torch.where(gauge, torch.ones_like(diag), diag))
        C = torch.linalg.cholesky(L)
        d = torch.cholesky_solve(rhs(om, w), C)
        R = R @ exp(torch.where(g3, torch.zeros_like(d), d))
        cvec = (R[bi, dst].transpose(-1, -2) @ tij[..., None])[..., 0]
        u = torch.where(g3, torch.zeros_like(u), torch.cholesky_solve(rhs(cvec, w), C))
    pose = torch.zeros(S, M, 4, 4, dtype=torch.float64, device=R.device)
    pose[..., :3, :3], pose[..., :3, 3], pose[..., 3, 3] = R, (R @ u[..., None])[..., 0], 1.0
    return pose, conf


def run_step(step, reps):
    import torch
    import sync_model as SM
    from relativepose_amd import util
    dev = torch.device("cuda", 0)
    name, scenes = workload(step)
    T, src, dst, w0, vb, eb = batch_of(scenes)
    S, M, E = len(scenes), scenes[0][0], len(scenes[0][1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Td, sd, dd, wd = up(T), up(src), up(dst), up(w0)
    hip = lambda: util.pose_sync_dev(Td, sd, dd, wd, vb, eb)
    got = hip()
    # the spanning tree's poses for torch: the model with no iteration
    init = [SM.sync_scene(M, s[1], s[2], s[3], np.ones(E), mu0=1.0, n_final=0) for s in scenes]
    R0, u0 = up(np.stack([p["pose"][:, :3, :3] for p in init])), None
    u0 = up(np.stack([np.einsum("vba,vb->va", p["pose"][:, :3, :3], p["pose"][:, :3, 3]) for p in init]))
    gauge = up(np.stack([p["component"] == np.arange(M) for p in init]))
    mus = SM.schedule()
    tor = lambda: torch_sync(R0, u0, gauge, sd.long().reshape(S, E), dd.long().reshape(S, E), Td.reshape(S, E, 4, 4), wd.reshape(S, E), mus)
    tp, tc = tor()
    d_pose = float((tp.reshape(-1, 4, 4) - got["pose"]).abs().max().item())
    model = lambda: SM.sync(T, src, dst, w0, vb, eb)
    want = model()
    d_model = float(np.abs(want["pose"] - got["pose"].cpu().numpy()).max())
    G = np.concatenate([np.stack([np.matmul(g, np.linalg.inv(s[4][0])) for g in s[4]]) for s in scenes])
    err = float(np.abs(got["pose"].cpu().numpy() - G).max())
    bad = np.concatenate([s[5] for s in scenes])
    conf = got["confidence"].cpu().numpy()
    (m, lo, hi), (tm, tlo, thi), (nm, nlo, nhi) = timed(hip, reps, inner=5), timed(tor, reps), timed(model, max(2, reps // 2), sync=False)
    n_iter = len(mus)
    chain = n_iter * 6 * M + M
    lines = [f"{name}: hip {m:.3f} ms ({lo:.3f} .. {hi:.3f}), torch {tm:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tm / m:.1f} x"
             f"{'' if tlo > hi else ' -- NOT faster beyond the spread'}, numpy model on the host {nm:.0f} ms ({nlo:.0f} .. {nhi:.0f}): {nm / m:.0f} x; "
             f"{n_iter} iterations, {chain} dependent steps per scene = {m * 1e6 / chain:.0f} ns per step; largest pose difference to torch {d_pose:.1e}, to the "
             f"model {d_model:.1e}, to ground truth {err:.1e}; outlier edges below 0.5: {int((conf[bad] < 0.5).sum())} of {int(bad.sum())}, "
             f"inliers above: {int((conf[~bad] > 0.5).sum())} of {int((~bad).sum())}"]
    if step == "hall":
        k = 63
        small = lambda: util.pose_sync_dev(Td[:k], sd[:k], dd[:k], wd[:k], vb, np.array([0, k], np.int32))
        sm, slo, shi = timed(small, reps, inner=5)
        lines.append(f"hall with its 63 chain edges alone (the same factorisation, substitutions and Prim steps): hip {sm:.3f} ms ({slo:.3f} .. {shi:.3f}) = "
                     f"{100 * sm / m:.0f} % of the full call: the dependent chain; the rest is per-edge work (residuals, weights, adjacency walks)")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_time.txt"))
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one workload in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args.reps)
        return
    lines = [f"# python tools/sync_time.py --reps {args.reps}, 1x MI355X (wall-clock per call over windows of synchronised calls after one warm-up -- 5 calls per "
             "window for hip, 1 for torch and the model --, median (min .. max) over the windows; hip = one util.pose_sync_dev call (one launch), torch = "
             "the iterations of the same contract with PyTorch operators, batched over the scenes)"]
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
