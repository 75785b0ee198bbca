"""Milliseconds of mesh extraction (csrc/mesh.hip, relpose_tsdf_mesh) next to surface extraction (relpose_tsdf_surface) on the same fused
state, ALTERNATING in the same run on the same GPU, on tools/tsdf_time.py's two workloads:

  pairs     32 pair volumes of 128^3 voxels with 2 views each at 160 x 640
  scene     one scene of 256 x 256 x 128 voxels with 32 views at 160 x 640

The mesh call does the surface call's work plus the triangles, so mesh / surface is the cost of connectivity.  Also the same contract
written with PyTorch operators (tools/tsdf_time.py's torch_surface for the vertices, torch_triangles below for the index buffer, scene by
scene), whose triangles are compared with the kernel's.  Both workloads run in ONE child process under one time limit (--limit seconds); the
parent never opens the GPU.  Wall-clock around synchronised calls (the calls wait for their stream), one warm-up, --reps timed windows of
three calls, the median per call over the windows and the spread (min .. max).  Bytes the mesh call must move at least, and their share of
the 8 TB/s HBM peak:
  count      tsdf_sum and weight read once (8 B per voxel; the corners a cell shares with its neighbours come from the caches)
  vertices   the state read once more (8 B per voxel), 52 B per vertex written (point, normal, valid; 64 B with colours), and per voxel the
             index of its first vertex and a flag byte written (5 B)
  triangles  those 5 B per voxel read, 12 B per triangle written
Writes profiles/mesh_time.txt (--out to write elsewhere).

  python tools/mesh_time.py [--reps 5] [--limit 600] [--no-torch] [--out PATH]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_mc_table as GEN  # noqa: E402
import tsdf_time as TT  # noqa: E402

HBM_PEAK = TT.HBM_PEAK


def torch_triangles(ts, wt, min_weight=1):
    """The triangle contract with PyTorch operators, one scene at a time -> [tri int64 [n,3]] per scene, in the contract's order"""
    import torch
    dev = ts.device
    T = GEN.table()
    count = torch.tensor([len(t) for t in T], device=dev)
    edges = torch.full((256, GEN.MAX_TRIANGLES, 3), -1, dtype=torch.long, device=dev)
    for c, t in enumerate(T):
        if t:
            edges[c, :len(t)] = torch.tensor(t, device=dev)
    off = torch.tensor([GEN.edge_ends(e)[0] for e in range(12)], device=dev)
    axis = torch.arange(12, device=dev) // 4
    lower = torch.tensor([[bin(m & ((1 << a) - 1)).count("1") for a in range(3)] for m in range(8)], device=dev)
    S, nz, ny, nx = ts.shape
    out = []
    for s in range(S):
        known = wt[s] >= min_weight
        neg = known & (ts[s] < 0)
        mask = torch.zeros_like(ts[s], dtype=torch.long)
        for c in range(3):
            kb, nb = TT._shift(known, c, 1, False), TT._shift(neg, c, 1, False)
            mask |= (known & kb & (neg != nb)).long() << c
        mask = mask.reshape(-1)
        cnt = lower[mask, 2] + (mask >> 2)
        first = torch.cumsum(cnt, 0) - cnt
        if min(nx, ny, nz) < 2:
            out.append(torch.zeros(0, 3, dtype=torch.long, device=dev))
            continue
        full = torch.ones(nz - 1, ny - 1, nx - 1, dtype=torch.bool, device=dev)
        case = torch.zeros(nz - 1, ny - 1, nx - 1, dtype=torch.long, device=dev)
        for c in range(8):
            ox, oy, oz = c & 1, c >> 1 & 1, c >> 2 & 1
            full &= known[oz:oz + nz - 1, oy:oy + ny - 1, ox:ox + nx - 1]
            case |= neg[oz:oz + nz - 1, oy:oy + ny - 1, ox:ox + nx - 1].long() << c
        k, j, i = torch.nonzero(full & (count[case] > 0), as_tuple=True)       # lexicographic: ascending cell index, x fastest
        ed = edges[case[k, j, i]]
        keep = ed[..., 0] >= 0
        e = ed.clamp(min=0)
        lin = ((k[:, None, None] + off[e, 2]) * ny + (j[:, None, None] + off[e, 1])) * nx + (i[:, None, None] + off[e, 0])
        out.append((first[lin] + lower[mask[lin], axis[e]])[keep].reshape(-1, 3))
    return out


def run(reps, with_torch):
    import torch
    from relativepose_amd import _lib, util
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    lines = [f"library: {os.path.basename(_lib.LIB_PATH)}"] if os.environ.get("RELPOSE_LIB_PATH") else []
    for step in TT.STEPS:
        name, depth, rgb, R, vb, origin, dims, voxel = TT.workload(step)
        S = len(vb) - 1
        nvox = dims[0] * dims[1] * dims[2]
        state = util.tsdf_fuse_dev(up(depth, np.float32), up(rgb, np.float32), up(R, np.float64), vb, origin, dims, voxel, "suncg")
        for colours in (True, False):
            st = state if colours else dict(state, color_sum=None)
            cnt = util.tsdf_surface_dev(st, 1, 1)[4]
            cap = max(1, int(cnt.max().item()))
            probe = util.tsdf_mesh_dev(st, 1, cap, 1)
            n_v, n_t, cap_tri = int(probe["n_points"].sum().item()), int(probe["n_triangles"].sum().item()), max(1, int(probe["n_triangles"].max().item()))
            del probe
            surf = lambda: util.tsdf_surface_dev(st, 1, cap)
            mesh = lambda: util.tsdf_mesh_dev(st, 1, cap, cap_tri)
            got_s, got_m = surf(), mesh()
            same_v = all(torch.equal(a, got_m[k]) for a, k in zip(got_s, ("points", "normals", "colors", "valid", "n_points")) if a is not None)
            # alternate: surface, mesh, surface, mesh, ...
            ts_, tm_ = [], []
            for _ in range(reps):
                ts_.append(TT.timed(surf, 1, inner=3)[0])
                tm_.append(TT.timed(mesh, 1, inner=3)[0])
            sm, slo, shi = float(np.median(ts_)), float(np.min(ts_)), float(np.max(ts_))
            mm, mlo, mhi = float(np.median(tm_)), float(np.min(tm_)), float(np.max(tm_))
            nbytes = S * nvox * (8 + 8 + 5 + 5) + n_v * (64 if colours else 52) + n_t * 12
            line = (f"{name}, {'with' if colours else 'without'} colours: mesh {mm:.3f} ms ({mlo:.3f} .. {mhi:.3f}), surface {sm:.3f} ms ({slo:.3f} .. {shi:.3f}): "
                    f"mesh / surface = {mm / sm:.2f}, connectivity costs {mm - sm:.3f} ms"
                    f"{'' if mlo > shi else ' -- NOT slower beyond the spread'}; {n_v} vertices, {n_t} triangles (caps {cap}, {cap_tri} per scene); "
                    f"{nbytes / 1e6:.1f} MB to move at least = {nbytes / (mm * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (mm * 1e-3) / HBM_PEAK:.2f} % of the "
                    f"8 TB/s HBM peak; vertex outputs bitwise the surface call's: {same_v}")
            if with_torch and colours:
                cs_l = state["color_sum"].long()
                tsl, wtl = state["tsdf_sum"].long(), state["weight"].long()
                tor = lambda: (TT.torch_surface(tsl, wtl, cs_l, origin, voxel), torch_triangles(tsl, wtl))
                ref = tor()[1]
                bad = sum(0 if (ref[s].shape[0] == int(got_m["n_triangles"][s]) and torch.equal(ref[s], got_m["triangles"][s, :ref[s].shape[0]].long()))
                          else 1 for s in range(S))
                del ref
                tt, tlo, thi = TT.timed(tor, max(2, reps // 2))
                line += (f"; torch (surface + triangles, scene by scene) {tt:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tt / mm:.1f} x"
                         f"{'' if tlo > mhi else ' -- NOT faster beyond the spread'}; scenes whose torch triangles differ from the kernel's: {bad} of {S}")
            lines.append(line)
            del got_s, got_m
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds the child process may take")
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch-operator version")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_time.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        run(args.reps, not args.no_torch)
        return
    lines = [f"# python tools/mesh_time.py --reps {args.reps}, 1x MI355X, one process (wall-clock per call over windows of 3 synchronised calls after one warm-up, "
             "surface and mesh windows alternating on the same state, median (min .. max) over the windows; mesh = one util.tsdf_mesh_dev call (four launches), "
             "surface = one util.tsdf_surface_dev call (three launches), torch = the same contract with PyTorch operators, 1 call per window)"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)] + (["--no-torch"] if args.no_torch else []),
                       capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measuring process ended with status {r.returncode}")
    lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
