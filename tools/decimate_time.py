"""Milliseconds of mesh decimation by vertex clustering (csrc/meshdecim.hip: relpose_mesh_decimate) on the meshes relpose_tsdf_mesh extracts
from tools/tsdf_time.py's two workloads, at factors 2 and 4 of the volume's voxel (util.mesh_decimate_volume_dev):

  pairs     32 pair volumes of 128^3 voxels with 2 views each at 160 x 640
  scene     one scene of 256 x 256 x 128 voxels with 32 views at 160 x 640

Per workload and factor: the call with and without dedupe, the triangles and vertices before and after, and the same contract written with
PyTorch operators (torch.unique over the cell indices, index_add_ into int64 rows, torch.unique over the rotated rows; scene by scene), whose
counts, positions and triangles are compared with the kernel's bit for bit (the normals within 1e-15: the operators' division is not
pinned).  Then the eight default rooms of `--mine-pairs --fuse 0.05 --mesh` (seeds 4000 .. 4007, 6 views): the triangle share that stays
and how far the vertices move (evaluation.decimate_mesh).  Everything runs in ONE
child process under one time limit (--limit seconds); the parent never opens the GPU.  Wall-clock around synchronised calls, one warm-up,
--reps timed windows of three calls, the kinds of window alternating, the median per call over the windows and the spread (min .. max).
Writes profiles/decimate_time.txt (--out to write elsewhere).

  python tools/decimate_time.py [--reps 5] [--limit 900] [--no-torch] [--out PATH]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tsdf_time as TT  # noqa: E402

FACTORS = (2, 4)
ROOMS, ROOM_VIEWS, ROOM_SEED, ROOM_VOXEL = 8, 6, 4000, 0.05


def torch_decimate(mesh, origin, cell, dims, dedupe=True):
    """The decimation contract with PyTorch operators, one scene at a time -> [(points f64 [n,3], count i64 [n], triangles i64 [m,3],
    normals f64 [n,3])] per scene"""
    import torch
    out = []
    dev = mesh["points"].device
    g = torch.tensor(dims, dtype=torch.float64, device=dev)
    n_pts, n_tri = mesh["n_points"].tolist(), mesh["n_triangles"].tolist()
    for s in range(mesh["points"].shape[0]):
        nv, nt = min(max(n_pts[s], 0), mesh["points"].shape[1]), min(max(n_tri[s], 0), mesh["triangles"].shape[1])
        o = torch.as_tensor(origin[s], dtype=torch.float64, device=dev)
        u = (mesh["points"][s, :nv] - o) / cell
        f = torch.floor(u)
        inside = (torch.isfinite(u) & (f >= 0) & (f < g)).all(1)
        idx = torch.nonzero(inside)[:, 0]
        fi = f[idx].long()
        lin = (fi[:, 2] * dims[1] + fi[:, 1]) * dims[0] + fi[:, 0]
        cells, inv = torch.unique(lin, return_inverse=True)
        first = torch.full((len(cells),), nv, dtype=torch.int64, device=dev).scatter_reduce(0, inv, idx, "amin")
        rank = torch.empty_like(first)
        rank[torch.argsort(first)] = torch.arange(len(first), device=dev)
        cl = rank[inv]
        vmap = torch.full((nv,), -1, dtype=torch.int64, device=dev)
        vmap[idx] = cl
        q = torch.round(u[idx] * 65536.0).long()                                # (torch.round: ties to even)
        acc = torch.zeros(len(cells), 3, dtype=torch.int64, device=dev).index_add_(0, cl, q)
        cnt = torch.zeros(len(cells), dtype=torch.int64, device=dev).index_add_(0, cl, torch.ones_like(cl))
        pts = o + (acc.double() / (65536.0 * cnt.double()[:, None])) * cell
        nn = mesh["normals"][s, :nv][idx]
        ok = torch.isfinite(nn) & (nn.abs() <= 65536.0)
        sn = torch.zeros(len(cells), 3, dtype=torch.int64, device=dev).index_add_(0, cl, torch.round(torch.where(ok, nn, torch.zeros_like(nn)) * 32768.0).long())
        sd = sn.double()
        ln = torch.sqrt((sd[:, 0] * sd[:, 0] + sd[:, 1] * sd[:, 1]) + sd[:, 2] * sd[:, 2])[:, None]
        nrm = torch.where(ln == 0, torch.zeros_like(sd), sd / torch.where(ln == 0, torch.ones_like(ln), ln))
        if mesh.get("colors") is not None:
            c = mesh["colors"][s, :nv][idx].double()
            c = torch.where(torch.isnan(c), torch.zeros_like(c), c.clamp(0.0, 1.0))
            sc = torch.zeros(len(cells), 3, dtype=torch.int64, device=dev).index_add_(0, cl, torch.round(c * 65535.0).long())
            col = (sc.double() / (65535.0 * cnt.double()[:, None])).float()    # noqa: F841  (computed, as the kernel does)
        t = mesh["triangles"][s, :nt].long()
        t = t[((t >= 0) & (t < nv)).all(1)]
        m = vmap[t]
        m = m[(m >= 0).all(1)]
        m = m[(m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])]
        if dedupe and len(m):
            k = torch.argmin(m, 1)
            rot = torch.stack([m.gather(1, ((k + j) % 3)[:, None])[:, 0] for j in range(3)], 1)
            key = (rot[:, 0] * len(cells) + rot[:, 1]) * len(cells) + rot[:, 2]
            _, kinv = torch.unique(key, return_inverse=True)
            rows = torch.arange(len(m), device=dev)
            low = torch.full((int(kinv.max()) + 1,), len(m), dtype=torch.int64, device=dev).scatter_reduce(0, kinv, rows, "amin")
            m = m[low[kinv] == rows]
        out.append((pts, cnt, m, nrm))
    return out


def run(reps, with_torch):
    import torch
    from relativepose_amd import evaluation as E, synth, util
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    f = lambda v: f"{np.median(v):.3f} ms ({np.min(v):.3f} .. {np.max(v):.3f})"
    lines = []
    for step in TT.STEPS:
        name, depth, rgb, R, vb, origin, dims, voxel = TT.workload(step)
        state = util.tsdf_fuse_dev(up(depth, np.float32), up(rgb, np.float32), up(R, np.float64), vb, origin, dims, voxel, "suncg")
        mesh = util.tsdf_mesh_dev(state, 1)
        S, nv, nt = int(mesh["points"].shape[0]), int(mesh["n_points"].sum()), int(mesh["n_triangles"].sum())
        calls = {(k, d): (lambda k=k, d=d: util.mesh_decimate_volume_dev(mesh, state, k, dedupe=d)) for k in FACTORS for d in (True, False)}
        times = {key: [] for key in calls}
        for fn in calls.values():
            fn()
        for _ in range(reps):                                                  # alternate the four in every window
            for key, fn in calls.items():
                times[key].append(TT.timed(fn, 1, inner=3)[0])
        for k in FACTORS:
            dec = calls[(k, True)]()
            loose = calls[(k, False)]()
            n1, t1, t0 = int(dec["n_points"].sum()), int(dec["n_triangles"].sum()), int(loose["n_triangles"].sum())
            line = (f"{name}, factor {k} (cell {k * voxel:g} m, grid {' x '.join(str(d) for d in dec['decimate_dims'])}): {nv} vertices, {nt} triangles -> {n1} vertices, "
                    f"{t1} triangles ({t1 / max(nt, 1):.4f} of the triangles; {int(dec['degenerate_triangles'].sum())} degenerate, "
                    f"{int(dec['duplicate_triangles'].sum())} duplicate, {int(dec['outside_triangles'].sum())} outside; {t0} triangles without dedupe); "
                    f"with dedupe {f(times[(k, True)])}, without {f(times[(k, False)])}")
            if with_torch:
                tor = lambda: torch_decimate(mesh, state["origin"], k * voxel, dec["decimate_dims"], True)
                ref = tor()
                bad = 0
                for s in range(S):
                    p, c, m, nrm = ref[s]
                    n, ntri = int(dec["n_points"][s]), int(dec["n_triangles"][s])
                    same = len(p) == n and len(m) == ntri and torch.equal(p, dec["points"][s, :n]) and torch.equal(c.int(), dec["count"][s, :n]) and \
                        torch.equal(m.int(), dec["triangles"][s, :ntri]) and torch.allclose(nrm, dec["normals"][s, :n], rtol=0.0, atol=1e-15)
                    bad += 0 if same else 1
                tt, tlo, thi = TT.timed(tor, max(2, reps // 2))
                kt = float(np.median(times[(k, True)]))
                line += (f"; torch (unique + index_add_, scene by scene) {tt:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tt / kt:.1f} x the call with dedupe"
                         f"{'' if tlo > np.max(times[(k, True)]) else ' -- NOT faster beyond the spread'}; scenes whose torch result differs from the kernel's: {bad} of {S}")
            lines.append(line)
        del state, mesh
    parts = {k: [] for k in FACTORS}
    before = []
    for s in range(ROOMS):
        sc = synth.render_scene(ROOM_SEED + s, ROOM_VIEWS, "suncg")
        mesh = E.fuse_views(up(sc["depth"], np.float32), up(sc["rgb"], np.float32), sc["R"], "suncg", ROOM_VOXEL, mesh=True)
        before.append(int(mesh["n_triangles"][0]))
        for k in FACTORS:
            parts[k].append(E.decimate_mesh(mesh, k)[1])
    for k in FACTORS:
        sm = E.mesh_decimate_summary(parts[k])
        lines.append(f"rooms ({ROOMS} suncg rooms of {ROOM_VIEWS} views at voxel {ROOM_VOXEL} m, seeds {ROOM_SEED} .. {ROOM_SEED + ROOMS - 1}), factor {k}: triangles median "
                     f"{float(np.median(before)):.0f} -> {sm['mesh_decimated_triangles_median']:.0f} (share median {sm['mesh_decimated_share_median']:.4f}); a vertex moves "
                     f"{sm['mesh_decimated_dist_median'] * 1e3:.2f} mm (median of the rooms' medians) = {sm['mesh_decimated_dist_median'] / (k * ROOM_VOXEL):.3f} cells; "
                     f"new vertices within half a cell of the original cloud: {sm['mesh_decimated_within_median']:.4f}")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds the child process may take")
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch-operator version")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decimate_time.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        run(args.reps, not args.no_torch)
        return
    lines = [f"# python tools/decimate_time.py --reps {args.reps}, 1x MI355X, one process (wall-clock per call over windows of 3 synchronised calls after one "
             "warm-up, the four kinds of window alternating on the same mesh, median (min .. max) over the windows; a call = one "
             "util.mesh_decimate_volume_dev call: the output and workspace allocations, the origin launches, and eleven kernel launches)"]
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
