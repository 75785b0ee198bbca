"""Milliseconds of rendering panoramas from TSDF volumes (csrc/tsdfrender.hip, relpose_tsdf_render) on the two workloads of the TSDF tools,
each ALTERNATING on the same GPU with the same contract written with PyTorch operators (float64 tensors, every ray marched through all
n_steps samples at once per step):

  pairs     64 views at 160 x 640 against 32 pair volumes of 128^3 voxels (view 2b and 2b + 1 against volume b)
  scene     32 views at 160 x 640 against one scene of 256 x 256 x 128 voxels

Every view is rendered from its true pose with the defaults (step = voxel / 2, d_max = the box diagonal), depth, normal, colour and cls.
Every workload runs in a child process of its own under a time limit of its own (--limit seconds); the parent never opens the GPU, and a
step that fails or runs out of time ends the tool.  Wall-clock around synchronised calls (the call waits for its stream), one warm-up,
--reps timed windows, the median per call over the windows and the spread (min .. max).  For the HIP call
  skip on / off     the same call with skip = 1 and skip = 0 (bitwise the same images: checked)
  flag launch       (t(skip = 1) - t(skip = 0)) of a call that marches nothing: one view at h = 2 with d_max = d_min (one sample per ray),
                    so what remains of the difference is the memset and the flag kernel over all volumes
  n_evaluated       the mean number of evaluated samples per ray under either mode, and rays per second
  bytes             what the call must read at least: 8 B per distinct corner voxel of an evaluated sample (counted with the PyTorch form,
                    skip = 0) and what it writes (29 B per pixel with every output), as a share of the 8 TB/s HBM peak -- a bound from
                    below: the volumes of these workloads fit the last-level cache, so the kernel need not be reading HBM at all
Writes profiles/render_time.txt (--out to write elsewhere).

  python tools/render_time.py [--reps 5] [--limit 400] [--out PATH]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12
STEPS = ("pairs", "scene")


def torch_rays(h, dataset, dev):
    import torch
    pix = torch.arange(4 * h * h, device=dev)
    row, col = pix // (4 * h), pix % (4 * h)
    slot, px = col // h, col % h
    xn = (2.0 * px.double()) / float(h) - 1.0
    yn = 1.0 - (2.0 * row.double()) / float(h)
    zn = -torch.ones_like(xn)
    k = slot if "suncg" in dataset else (slot + 3) & 3
    x = torch.where(k == 0, xn, torch.where(k == 1, -zn, torch.where(k == 2, -xn, zn)))
    z = torch.where(k == 0, zn, torch.where(k == 1, xn, torch.where(k == 2, -zn, -xn)))
    return torch.stack([x, yn, z], -1)


def torch_render(ts, wt, cs, origin, dims, voxel, pose, sov, dataset, h, d_min, step, n_steps, touched=None):
    """The rendering contract with PyTorch operators, skip = 0 and no clip: all rays of all views advance one sample per iteration.
    -> (depth [V,h,4h] f32, cls u8, normal [V,3,h,4h] f32, color [V,3,h,4h] f32, n_evaluated i32)"""
    import torch
    nx, ny, nz = dims
    dev = pose.device
    V = pose.shape[0]
    N = 4 * h * h
    dirs = torch_rays(h, dataset, dev)                               # [N,3]
    Rm, t = pose[:, :3, :3], pose[:, :3, 3]
    W, w3 = Rm.transpose(1, 2), -torch.einsum("vba,vb->va", Rm, t)
    wd = torch.einsum("vab,nb->vna", W, dirs)                        # world direction per unit depth (the model rounds q per sample instead)
    o = origin[sov]
    nvox = nx * ny * nz
    base = (sov.long() * nvox)[:, None]
    tsf, wtf = ts.reshape(-1), wt.reshape(-1)
    lim = torch.tensor([nx - 2, ny - 2, nz - 2], dtype=torch.float64, device=dev)

    def cell(d):
        q = wd * d + w3[:, None] if not torch.is_tensor(d) else wd * d[..., None] + w3[:, None]
        u = (q - o[:, None]) / voxel - 0.5
        fl = torch.floor(u)
        inr = torch.isfinite(q).all(-1) & ((fl >= 0) & (fl <= lim)).all(-1)
        i0 = torch.where(inr[..., None], fl, torch.zeros_like(fl)).long()
        return inr, i0, u - fl

    def lerp(c, f, grad=False):
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        d00, d10, d01, d11 = c[1] - c[0], c[3] - c[2], c[5] - c[4], c[7] - c[6]
        a00, a10, a01, a11 = c[0] + fx * d00, c[2] + fx * d10, c[4] + fx * d01, c[6] + fx * d11
        c0, c1 = a10 - a00, a11 - a01
        b0, b1 = a00 + fy * c0, a01 + fy * c1
        gz = b1 - b0
        r = b0 + fz * gz
        if not grad:
            return r
        gy = c0 + fz * (c1 - c0)
        e0, e1 = d00 + fy * (d10 - d00), d01 + fy * (d11 - d01)
        return r, torch.stack([e0 + fz * (e1 - e0), gy, gz], -1)

    def corners(i0):
        return [base + ((i0[..., 2] + (c >> 2 & 1)) * ny + (i0[..., 1] + (c >> 1 & 1))) * nx + (i0[..., 0] + (c & 1)) for c in range(8)]

    def value(i0, f, grad=False):
        lin = corners(i0)
        w = [wtf[l] for l in lin]
        known = torch.stack([x >= 1 for x in w]).all(0)
        tc = [tsf[l].double() / (32768.0 * torch.clamp(x, min=1).double()) for l, x in zip(lin, w)]
        return (known, lerp(tc, f, grad), lin, w)

    cls = torch.zeros(V, N, dtype=torch.uint8, device=dev)
    nev = torch.zeros(V, N, dtype=torch.int32, device=dev)
    hitk = torch.full((V, N), -1, dtype=torch.int64, device=dev)
    alive = torch.ones(V, N, dtype=torch.bool, device=dev)
    pv = torch.zeros_like(alive)
    pt = torch.zeros(V, N, dtype=torch.float64, device=dev)
    for k in range(n_steps):
        inr, i0, f = cell(d_min + float(k) * step)
        ev = alive & inr
        nev += ev
        known, tt, lin, _ = value(i0, f)
        if touched is not None:
            for l in lin:
                touched[l[ev]] = True
        v = ev & known
        pair = v & pv
        hit, back = pair & (pt >= 0) & (tt < 0), pair & (pt < 0) & (tt >= 0)
        cls[hit], cls[back] = 1, 2
        hitk[hit] = k
        alive &= ~(hit | back)
        pv, pt = v, torch.where(v, tt, torch.zeros_like(tt))
    m = cls == 1
    kb = hitk.clamp(min=1).double()
    da, db = d_min + (kb - 1.0) * step, d_min + kb * step
    outs = []
    for d in (da, db):
        _, i0, f = cell(d)
        _, (tv, g), lin, w = value(i0, f, True)
        col = torch.stack([lerp([cs.reshape(-1)[(sov.long() * 3 * nvox)[:, None] + ch * nvox + (l - base)].double() / (255.0 * torch.clamp(x, min=1).double())
                                 for l, x in zip(lin, w)], f) for ch in range(3)], -1)
        outs.append((tv, g, col))
    (ta, ga, ca), (tb, gb, cb) = outs
    s = torch.where(m, ta / torch.where(m, ta - tb, torch.ones_like(ta)), torch.zeros_like(ta))
    depth = torch.where(m, da + s * step, torch.zeros_like(da)).float()
    nv = ga + s[..., None] * (gb - ga)
    nn = torch.sqrt((nv * nv).sum(-1, keepdim=True))
    nv = torch.where(nn > 0, nv / torch.where(nn > 0, nn, torch.ones_like(nn)), nv)
    normal = torch.where(m[..., None], torch.einsum("vij,vnj->vni", Rm, nv), torch.zeros_like(nv)).float()
    color = torch.where(m[..., None], ca + s[..., None] * (cb - ca), torch.zeros_like(ca)).float()
    shape = lambda a: a.reshape(V, h, 4 * h, 3).permute(0, 3, 1, 2).contiguous()
    return depth.reshape(V, h, 4 * h), cls.reshape(V, h, 4 * h), shape(normal), shape(color), nev.reshape(V, h, 4 * h)


def workload(step):
    """align_time.py's two workloads with their colours -> (name, depth, rgb, R, scene_of_view, view_begin, origin, dims, voxel)"""
    from relativepose_amd import synth
    if step == "pairs":
        depth, rgb, R = [], [], []
        for b in range(32):
            sc = synth.render_scene(4000 + b, 2, "suncg")
            depth.append(sc["depth"]), rgb.append(sc["rgb"]), R.append(sc["R"])
        return ("pairs (64 views against 32 volumes of 128^3)", np.concatenate(depth), np.concatenate(rgb), np.concatenate(R),
                np.repeat(np.arange(32, dtype=np.int32), 2), np.arange(0, 65, 2, dtype=np.int32), np.tile(-64 * 0.0625 * np.ones(3), (32, 1)),
                (128, 128, 128), 0.0625)
    sc = synth.render_scene(77, 32, "suncg")
    dims = (256, 256, 128)
    voxel = float(np.max(2 * (sc["half"] + 0.1) / np.array(dims)))
    return ("scene (32 views against one volume of 256 x 256 x 128)", sc["depth"], sc["rgb"], sc["R"], np.zeros(32, np.int32),
            np.array([0, 32], np.int32), (-0.5 * voxel * np.array(dims))[None], dims, voxel)


def run_step(step, reps, hip_only=False):
    import torch
    from align_time import timed
    from relativepose_amd import evaluation, util
    dev = torch.device("cuda", 0)
    name, depth, rgb, R, sov, vb, origin, dims, voxel = workload(step)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    depth, rgb, pose = up(depth, np.float32), up(rgb, np.float32), up(R, np.float64)
    V, h = depth.shape[0], depth.shape[1]
    state = util.tsdf_fuse_dev(depth, rgb, R, vb, origin, dims, voxel, "suncg")
    stp, n_steps = util.tsdf_render_steps(dims, voxel)
    hip = {s: (lambda s=s: util.tsdf_render_dev(state, pose, "suncg", h, sov, skip=bool(s), stages=True)) for s in (1, 0)}
    tiny = {s: (lambda s=s: util.tsdf_render_dev(state, pose[:1], "suncg", 2, sov[:1], d_max=0.0, skip=bool(s))) for s in (1, 0)}
    if hip_only:                                                     # for a counter run: the two HIP modes alone, no PyTorch form
        for s in (1, 0):
            m, lo, hi = timed(hip[s], reps, inner=3)
            print(f"{name}: hip skip={s} {m:.3f} ms ({lo:.3f} .. {hi:.3f})", flush=True)
        return
    org, sovd = up(origin, np.float64), up(sov, np.int64)
    touched = torch.zeros(state["tsdf_sum"].numel(), dtype=torch.bool, device=dev)
    ref = torch_render(state["tsdf_sum"], state["weight"], state["color_sum"], org, dims, voxel, pose, sovd, "suncg", h, 0.0, stp, n_steps, touched)
    n_touched = int(touched.sum().item())
    del touched
    tor = lambda: torch_render(state["tsdf_sum"], state["weight"], state["color_sum"], org, dims, voxel, pose, sovd, "suncg", h, 0.0, stp, n_steps)
    a, b = hip[1](), hip[0]()
    same = all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    cls_same = float((a[3] == ref[1]).double().mean().item())
    both = (a[3] == 1) & (ref[1] == 1)
    depth_diff = float((a[0][both] - ref[0][both]).abs().max().item()) if bool(both.any()) else float("nan")
    (med, p90), cov = evaluation.render_scores(a[0], a[3], depth, voxel)
    rays = V * 4 * h * h
    ev = {s: float(x[4].double().mean().item()) for s, x in ((1, a), (0, b))}
    t = {s: timed(hip[s], reps, inner=3) for s in (1, 0)}
    tt = {s: timed(tiny[s], reps, inner=5) for s in (1, 0)}
    tm, tlo, thi = timed(tor, max(2, reps // 2))
    nbytes = n_touched * 8 + rays * 29
    best = min(t[1][0], t[0][0])
    print(f"{name}, {n_steps} steps of {stp:.5f}: hip skip=1 {t[1][0]:.3f} ms ({t[1][1]:.3f} .. {t[1][2]:.3f}), skip=0 {t[0][0]:.3f} ms ({t[0][1]:.3f} .. "
          f"{t[0][2]:.3f}): skip is {'faster' if t[1][2] < t[0][1] else ('slower' if t[1][1] > t[0][2] else 'NOT different beyond the spread')}; "
          f"images bitwise equal between the modes: {same}; torch (skip=0, no clip) {tm:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tm / best:.1f} x"
          f"{'' if tlo > max(t[1][2], t[0][2]) else ' -- NOT faster beyond the spread'}; flag launch (memset + kernel over all volumes; one view at h = 2, "
          f"one sample per ray): skip=1 {tt[1][0] * 1e3:.1f} us ({tt[1][1] * 1e3:.1f} .. {tt[1][2] * 1e3:.1f}), skip=0 {tt[0][0] * 1e3:.1f} us "
          f"({tt[0][1] * 1e3:.1f} .. {tt[0][2] * 1e3:.1f}): {max(tt[1][0] - tt[0][0], 0.0) * 1e3:.1f} us; evaluated samples per ray: skip=1 {ev[1]:.1f}, "
          f"skip=0 {ev[0]:.1f} of {n_steps}; {rays / 1e6:.2f} M rays: {rays / (t[1][0] * 1e-3) / 1e9:.2f} G rays/s with skip, "
          f"{rays / (t[0][0] * 1e-3) / 1e9:.2f} without; {n_touched / 1e6:.2f} M distinct corner voxels + 29 B per pixel = {nbytes / 1e6:.1f} MB at least = "
          f"{nbytes / (best * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (best * 1e-3) / HBM_PEAK:.2f} % of the 8 TB/s HBM peak; against the scans: median "
          f"{med:.4f} p90 {p90:.4f} voxels, coverage {cov:.4f}; against torch (q = o + d w, not rounded per sample as the contract does): cls equal on "
          f"{100 * cls_same:.3f} % of the pixels, largest depth difference on common hits {depth_diff:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds each workload's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.txt"))
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one workload in this process")
    ap.add_argument("--hip-only", action="store_true", help="with --step: time the HIP calls only (what a rocprofv3 --pmc run wraps)")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args.reps, args.hip_only)
        return
    lines = [f"# python tools/render_time.py --reps {args.reps}, 1x MI355X (wall-clock per call over windows of synchronised calls after one warm-up -- 3 calls "
             "per window for hip, 5 for the flag launch, 1 for torch --, median (min .. max) over the windows; hip = one util.tsdf_render_dev call with "
             "depth, normal, colour, cls and n_evaluated, torch = the same contract with PyTorch operators, all views at once)"]
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
