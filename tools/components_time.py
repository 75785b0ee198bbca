"""Milliseconds of mesh connected components and of their removal (csrc/meshcc.hip: relpose_mesh_components, relpose_mesh_filter) on the
meshes relpose_tsdf_mesh extracts from tools/tsdf_time.py's two workloads:

  pairs     32 pair volumes of 128^3 voxels with 2 views each at 160 x 640
  scene     one scene of 256 x 256 x 128 voxels with 32 views at 160 x 640

Per workload: the labelling call with statistics (areas included), the same call as a counting call (cap_comp = 0: labels only), the filter
call that keeps every scene's largest component, and the propagation rounds the labelling took.  The statistics' cost is the difference of
the first two; next to it the NAIVE form of the triangle statistics (tools/components_naive.hip: one atomicAdd per triangle and sum, built
here with hipcc into tools/components_naive.so), whose sums are compared with the library's.  Also the same contract written with PyTorch
operators (min-label propagation with scatter_reduce and pointer jumping, scene by scene, its labels compared with the kernel's) and
scipy.sparse.csgraph.connected_components on the host (the graph build included, the copy to the host not).  Both workloads run in ONE child
process under one time limit (--limit seconds); the parent never opens the GPU.  Wall-clock around synchronised calls, one warm-up, --reps
timed windows of three calls, the median per call over the windows and the spread (min .. max).
Writes profiles/components_time.txt (--out to write elsewhere).

  python tools/components_time.py [--reps 5] [--limit 600] [--no-torch] [--out PATH]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tsdf_time as TT  # noqa: E402

NAIVE_SRC, NAIVE_LIB = os.path.join(HERE, "components_naive.hip"), os.path.join(HERE, "components_naive.so")


def build_naive():
    if not os.path.exists(NAIVE_LIB) or os.path.getmtime(NAIVE_SRC) > os.path.getmtime(NAIVE_LIB):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               "-ffp-contract=off", "-o", NAIVE_LIB, NAIVE_SRC])
    return NAIVE_LIB


def torch_components(tri, n_tri, n_pts):
    """The labelling contract with PyTorch operators, one scene at a time -> [vertex_label int64 [nv]] per scene (-1: unused)"""
    import torch
    out = []
    for s in range(tri.shape[0]):
        nv, nt = int(n_pts[s]), int(n_tri[s])
        t = tri[s, :nt].long()
        t = t[((t >= 0) & (t < nv)).all(1)]
        L = torch.arange(nv, device=tri.device)
        while True:
            m = L[t].min(1).values
            new = L.scatter_reduce(0, t.reshape(-1), m.repeat_interleave(3), "amin")
            new = new[new]
            if torch.equal(new, L):
                break
            L = new
        used = torch.zeros(nv, dtype=torch.bool, device=tri.device)
        used[t.reshape(-1)] = True
        root = used & (L == torch.arange(nv, device=tri.device))
        rank = torch.cumsum(root.long(), 0) - 1
        out.append(torch.where(used, rank[L], torch.full_like(L, -1)))
    return out


def scipy_components(tri, n_tri, n_pts):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = []
    for s in range(tri.shape[0]):
        nv, t = int(n_pts[s]), tri[s, :int(n_tri[s])].astype(np.int64)
        i, j = np.concatenate([t[:, 0], t[:, 0]]), np.concatenate([t[:, 1], t[:, 2]])
        k, lab = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(nv, nv)), directed=False)
        used = np.zeros(nv, bool)
        used[t.reshape(-1)] = True
        n.append(len(np.unique(lab[used])))
    return n


def run(reps, with_torch):
    import torch
    from relativepose_amd import _lib, util
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    naive = C.CDLL(build_naive())
    naive.components_naive_stats.restype = C.c_int
    naive.components_naive_stats.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 3
    lines = []
    for step in TT.STEPS:
        name, depth, rgb, R, vb, origin, dims, voxel = TT.workload(step)
        state = util.tsdf_fuse_dev(up(depth, np.float32), up(rgb, np.float32), up(R, np.float64), vb, origin, dims, voxel, "suncg")
        mesh = util.tsdf_mesh_dev(state, 1)
        mesh["voxel"] = voxel
        del state
        S, cap, cap_tri = int(mesh["points"].shape[0]), int(mesh["points"].shape[1]), int(mesh["triangles"].shape[1])
        comps = util.mesh_components_dev(mesh)
        cap_comp, scale = int(comps["comp_root"].shape[1]), comps["area_scale"]
        n_comp = comps["n_components"].cpu().numpy()
        ct = comps["comp_triangles"].cpu().numpy()
        share = ct.max(1) / np.maximum(ct.sum(1), 1)
        rounds = []

        def label(cc):
            c = util.mesh_components_dev(mesh, scale, cc)
            rounds.append(c["rounds"])
            return c

        keep = util.mesh_keep_mask(comps, largest=1)
        filt = lambda: util.mesh_filter_dev(mesh, comps, keep)
        clean = filt()
        # the naive statistics kernel on the library's labels
        nt_, na_ = torch.zeros_like(comps["comp_triangles"]), torch.zeros_like(comps["comp_area"])
        tri, pts, tl = mesh["triangles"].contiguous(), mesh["points"].contiguous(), comps["tri_label"]

        def naive_stats():
            nt_.zero_(), na_.zero_()
            assert naive.components_naive_stats(tri.data_ptr(), tl.data_ptr(), pts.data_ptr(), S, cap, cap_tri, cap_comp, scale, nt_.data_ptr(),
                                                na_.data_ptr(), _lib.stream_ptr()) == 0

        naive_stats()
        same_naive = torch.equal(nt_, comps["comp_triangles"]) and torch.equal(na_, comps["comp_area"])
        zero = lambda: (nt_.zero_(), na_.zero_())
        tw, tc, tf, tn, tz = [], [], [], [], []
        for _ in range(reps):                                                  # alternate the five in every window
            tw.append(TT.timed(lambda: label(cap_comp), 1, inner=3)[0])
            tc.append(TT.timed(lambda: label(0), 1, inner=3)[0])
            tf.append(TT.timed(filt, 1, inner=3)[0])
            tn.append(TT.timed(naive_stats, 1, inner=3)[0])
            tz.append(TT.timed(zero, 1, inner=3)[0])
        f = lambda v: f"{np.median(v):.3f} ms ({np.min(v):.3f} .. {np.max(v):.3f})"
        stats_cost = float(np.median(tw) - np.median(tc))
        naive_cost = float(np.median(tn) - np.median(tz))
        line = (f"{name}: {int(mesh['n_points'].sum())} vertices, {int(mesh['n_triangles'].sum())} triangles (caps {cap}, {cap_tri} per scene), components per scene "
                f"{int(n_comp.min())} .. {int(n_comp.max())} (median {float(np.median(n_comp)):.0f}), largest share median {float(np.median(share)):.4f}; "
                f"rounds {min(rounds)} .. {max(rounds)} over {len(rounds)} calls; labels + statistics {f(tw)}, labels only (counting call) {f(tc)}: "
                f"the aggregated statistics cost {stats_cost:.3f} ms; the naive per-triangle atomics (triangle count and area, two clears included) {f(tn)}, "
                f"the clears alone {f(tz)}: naive statistics {naive_cost:.3f} ms = {naive_cost / max(stats_cost, 1e-9):.1f} x the aggregated "
                f"(which also hold comp_vertices and comp_root), sums equal: {same_naive}; filter (largest component kept) {f(tf)}, "
                f"{int(mesh['n_triangles'].sum()) - int(clean['n_triangles'].sum())} triangles removed")
        host = {k: mesh[k].cpu().numpy() for k in ("triangles", "n_triangles", "n_points")}
        t0 = time.perf_counter()
        n_sci = scipy_components(host["triangles"], host["n_triangles"], host["n_points"])
        t_sci = (time.perf_counter() - t0) * 1e3
        line += (f"; scipy connected_components on the host, scene by scene, {t_sci:.1f} ms (one run): {t_sci / np.median(tc):.1f} x the counting call, "
                 f"counts equal: {n_sci == n_comp.tolist()}")
        if with_torch:
            tor = lambda: torch_components(mesh["triangles"], host["n_triangles"], host["n_points"])
            ref = tor()
            bad = sum(0 if torch.equal(ref[s], comps["vertex_label"][s, :len(ref[s])].long()) else 1 for s in range(S))
            tt, tlo, thi = TT.timed(tor, max(2, reps // 2))
            line += (f"; torch (min-label propagation, scene by scene) {tt:.1f} ms ({tlo:.1f} .. {thi:.1f}): {tt / np.median(tc):.1f} x the counting call"
                     f"{'' if tlo > np.max(tc) else ' -- NOT faster beyond the spread'}; scenes whose torch labels differ from the kernel's: {bad} of {S}")
        lines.append(line)
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds the child process may take")
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch-operator version")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_time.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        run(args.reps, not args.no_torch)
        return
    lines = [f"# python tools/components_time.py --reps {args.reps}, 1x MI355X, one process (wall-clock per call over windows of 3 synchronised calls after one "
             "warm-up, the five kinds of window alternating on the same mesh, median (min .. max) over the windows; labels = one util.mesh_components_dev call "
             "with a given cap_comp: init, mark, two launches per round with one wait per 4 rounds, five ranking and statistics launches; filter = one "
             "util.mesh_filter_dev call, four launches)"]
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
