"""CPU: the generated marching-cubes table (tools/gen_mc_table.py -> csrc/mc_table.h) is the committed one and has the pinned properties;
the mesh contract's numpy model (tests/mesh_model.py) agrees with its own plain-loop statement and gives closed, consistently wound,
manifold meshes; save_ply writes faces and leaves a cloud's bytes alone; and the host layers around relpose_tsdf_mesh -- operator
registration, workspace query, argument validation, CLI flag -- work without a GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import mesh_model as MM
import mesh_scenes as MS
import tsdf_model as TM
import tsdf_scenes as TS

GEN = MM.GEN


def test_committed_header_is_the_generators_output():
    assert open(GEN.HEADER).read() == GEN.header_text()
    words = [GEN.packed(t) for t in MM.TABLE]
    assert all(f"0x{w:016x}ull" in open(GEN.HEADER).read() for w in words)
    for c, w in enumerate(words):                                              # the packing reads back
        n = w >> 60
        assert [tuple(w >> 4 * (3 * t + j) & 15 for j in range(3)) for t in range(n)] == MM.TABLE[c]


def test_table_counts_and_no_in_face_diagonal():
    T = MM.TABLE
    assert sum(len(t) for t in T) == 820 and max(len(t) for t in T) == 5
    assert T[0] == [] and T[255] == []
    loops = [GEN.case_loops(c) for c in range(256)]
    assert max(len(lp) for ls in loops for lp in ls) == 7 and max(len(ls) for ls in loops) == 4
    for c in range(256):
        crossing = {e for e, (a, b) in enumerate(GEN.EDGE_CORNERS) if (c >> a & 1) != (c >> b & 1)}
        assert {e for t in T[c] for e in t} == crossing                        # every crossing edge is used, and nothing else
        assert sum(len(lp) - 2 for lp in loops[c]) == len(T[c])
        assert all(len(set(t)) == 3 for t in T[c])
        # a triangle side that is no loop segment is a fan diagonal: it must not join two edges of one cube face
        seg = {(lp[x], lp[(x + 1) % len(lp)]) for lp in loops[c] for x in range(len(lp))}
        for t in T[c]:
            for x in range(3):
                a, b = t[x], t[(x + 1) % 3]
                if (a, b) not in seg and (b, a) not in seg:
                    assert not (GEN.EDGE_FACES[a] & GEN.EDGE_FACES[b]), (c, t)
        # inside a cell the directed sides pair up except along the loops, which run once each
        d = [(t[x], t[(x + 1) % 3]) for t in T[c] for x in range(3)]
        assert len(set(d)) == len(d) and {e for e in d if (e[1], e[0]) not in d} == seg


def test_winding_faces_where_t_grows():
    """planes t = n . x - d, all 26 n in {-1, 0, 1}^3 with 23 offsets each: (p1 - p0) x (p2 - p0) . n >= 0 for every triangle"""
    from fractions import Fraction as Fr                                       # exact: "non-negative" needs no tolerance
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    checked, cases = 0, set()
    for n in itertools.product((-1, 0, 1), repeat=3):
        if n == (0, 0, 0):
            continue
        for d in np.linspace(-1.4, 2.9, 23):
            t = [sum(n[a] * GEN.corner_offset(c)[a] for a in range(3)) - Fr(float(d)) for c in range(8)]
            case = sum(1 << c for c in range(8) if t[c] < 0)
            pos = {}
            for e in range(12):
                p, q = GEN.edge_ends(e)
                ta, tb = t[GEN.corner_index(p)], t[GEN.corner_index(q)]
                if (ta < 0) != (tb < 0):
                    pos[e] = [p[a] + ta / (ta - tb) * (q[a] - p[a]) for a in range(3)]
            for tri in MM.TABLE[case]:
                p0, p1, p2 = (pos[e] for e in tri)
                nn = cross([p1[a] - p0[a] for a in range(3)], [p2[a] - p0[a] for a in range(3)])
                assert sum(nn[a] * n[a] for a in range(3)) >= 0, (n, d, tri)
                checked += 1
                cases.add(case)
    assert checked >= 500 and len(cases) >= 40                                 # 509 triangles over the cases that planes produce


@pytest.mark.parametrize("name", ["all_cases", "noise", "flat", "empty_in_batch", "edge_state"])
def test_loops_equal_the_array_form(name):
    c = MS.case(name)
    total = 0
    for s in range(c["tsdf_sum"].shape[0]):
        a, b = MM.triangles(c["tsdf_sum"][s], c["weight"][s], c["min_weight"]), MM.triangles_loops(c["tsdf_sum"][s], c["weight"][s], c["min_weight"])
        assert TS.bits_equal(a[0], b[0]) and TS.bits_equal(a[1], b[1]), s
        assert (np.diff(a[1]) >= 0).all()                                      # ascending cell index
        n = TM.surface(c["tsdf_sum"][s], c["weight"][s], None, c["origin"][s], c["voxel"], c["min_weight"])["n"]
        assert len(a[0]) == 0 or (a[0].min() >= 0 and a[0].max() < n)
        assert (a[0][:, 0] != a[0][:, 1]).all() and (a[0][:, 1] != a[0][:, 2]).all() and (a[0][:, 0] != a[0][:, 2]).all()
        total += len(a[0])
        if name == "all_cases":
            assert len(a[0]) == len(MM.TABLE[s])                               # scene s realises case s
    nv, nt = MS.counts(name)
    assert nt.sum() == total and (name != "flat" or (total == 0 and nv.min() > 0))
    if name == "all_cases":
        assert total == 820
    if name == "empty_in_batch":
        assert nv[1] == 0 and nt[1] == 0 and nt[0] > 0 and nt[2] > 0


def _cell_complete(known, lo):
    nz, ny, nx = known.shape
    i, j, k = lo
    if i < 0 or j < 0 or k < 0 or i > nx - 2 or j > ny - 2 or k > nz - 2:
        return False
    return bool(known[k:k + 2, j:j + 2, i:i + 2].all())


def test_noise_is_manifold_and_open_only_where_a_cell_is_missing():
    c = MS.case("noise")
    ts, wt = c["tsdf_sum"][0], c["weight"][0]
    assert ts.shape == (9, 11, 13) and 0.02 < (wt == 0).mean() < 0.09 and ((ts == 0) & (wt > 0)).sum() >= 3
    tri, _ = MM.triangles(ts, wt, 1)
    edge = TM.surface(ts, wt, None, c["origin"][0], c["voxel"], 1)["edge"]
    dup, unpaired = MM.edge_report(tri)
    assert dup == 0 and len(tri) > 1000
    assert 0 < len(unpaired) < 3 * len(tri)
    known = wt >= 1
    nz, ny, nx = ts.shape
    for a, b in unpaired:                                                      # both vertices on one grid face next to a missing cell
        pts = []
        for v in (a, b):
            lin, ax = edge[v]
            p = np.array([lin % nx, lin // nx % ny, lin // (nx * ny)])
            q = p.copy()
            q[ax] += 1
            pts += [p, q]
        lo, hi = np.min(pts, 0), np.max(pts, 0)
        ext = hi - lo
        assert sorted(ext.tolist()) == [0, 1, 1], (a, b)
        n = int(np.argmin(ext))
        below = lo.copy()
        below[n] -= 1
        assert not (_cell_complete(known, lo) and _cell_complete(known, below)), (a, b)


def test_sphere_is_closed_with_euler_characteristic_2_and_outward_winding():
    c = MS.case("sphere")
    ts, wt = c["tsdf_sum"][0], c["weight"][0]
    tri, _ = MM.triangles(ts, wt, 1)
    s = TM.surface(ts, wt, None, c["origin"][0], c["voxel"], 1)
    dup, unpaired = MM.edge_report(tri)
    assert dup == 0 and len(unpaired) == 0 and len(tri) > 2000
    V, E, F = len(np.unique(tri)), 3 * len(tri) // 2, len(tri)
    assert V == s["n"] and V - E + F == 2
    p, nrm = s["points"], s["normals"]
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    for j in range(3):
        assert ((n * nrm[tri[:, j]]).sum(1) > 0).all()
    from relativepose_amd import evaluation as E_
    st = E_.mesh_stats({"points": p[None], "triangles": tri[None], "n_triangles": np.array([F])})[0]
    assert st["triangles"] == F and st["border_edges"] == 0 and st["nonmanifold_edges"] == 0
    assert abs(st["area"] / (4 * np.pi * (8.4 * c["voxel"]) ** 2) - 1) < 0.02
    # mesh_stats counts what is wrong with a broken mesh: a dropped triangle opens three edges, a doubled one makes three non-manifold
    cut = E_.mesh_stats({"points": p[None], "triangles": tri[None, 1:], "n_triangles": np.array([F - 1])})[0]
    dbl = E_.mesh_stats({"points": p[None], "triangles": np.concatenate([tri, tri[:1]])[None], "n_triangles": np.array([F + 1])})[0]
    assert cut["border_edges"] == 3 and cut["nonmanifold_edges"] == 0 and dbl["nonmanifold_edges"] == 3
    assert E_.mesh_summary([st, cut])["mesh_nonmanifold_edges"] == 0 and E_.mesh_summary([st, cut])["mesh_triangles_median"] == F - 0.5


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS)
def test_rooms_mesh_is_manifold(ds, h):
    c = MS.case(f"room_{ds}_{h}")
    tri, _ = MM.triangles(c["tsdf_sum"][0], c["weight"][0], 1)
    dup, unpaired = MM.edge_report(tri)
    assert dup == 0 and len(tri) > 4000 and len(unpaired) < len(tri)


def test_mesh_outputs_truncate_like_the_contract():
    c = MS.case("edge_state")
    nv, nt = MS.counts("edge_state")
    cap, cap_tri, full = MS.expected("edge_state")
    assert cap == nv[0] + 3 and cap_tri == nt[0] + 3 and (full["triangles"][0, nt[0]:] == MS.TRI_FILL).all() and full["n_triangles"][0] == nt[0]
    _, _, cut = MS.expected("edge_state", 10, 7)
    assert cut["n_triangles"][0] == nt[0] and TS.bits_equal(cut["triangles"][0], full["triangles"][0, :7]) and cut["triangles"].max() >= 10


def test_save_ply_with_faces_and_without(tmp_path):
    from relativepose_amd import util
    rs = np.random.RandomState(4)
    N, F = 11, 7
    p, n, c = rs.randn(N, 3), rs.randn(N, 3), rs.uniform(-0.2, 1.2, (N, 3)).astype(np.float32)
    f = rs.randint(0, N, (F, 3)).astype(np.int32)

    def vertex_bytes(with_n, with_c):
        out = b""
        q = np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8)
        for r in range(N):
            out += p[r].astype("<f4").tobytes() + (n[r].astype("<f4").tobytes() if with_n else b"") + (q[r].tobytes() if with_c else b"")
        return out

    def head(with_n, with_c, faces):
        h = ["ply", "format binary_little_endian 1.0", f"element vertex {N}", "property float x", "property float y", "property float z"]
        h += ["property float nx", "property float ny", "property float nz"] if with_n else []
        h += ["property uchar red", "property uchar green", "property uchar blue"] if with_c else []
        h += [f"element face {faces}", "property list uchar int vertex_indices"] if faces is not None else []
        return ("\n".join(h + ["end_header"]) + "\n").encode("ascii")

    face_bytes = b"".join(b"\x03" + f[r].astype("<i4").tobytes() for r in range(F))
    for with_n, with_c in ((True, True), (False, False), (False, True)):
        kw = dict(normals=n if with_n else None, colors=c if with_c else None)
        assert util.save_ply(str(tmp_path / "cloud.ply"), p, **kw) == N
        assert (tmp_path / "cloud.ply").read_bytes() == head(with_n, with_c, None) + vertex_bytes(with_n, with_c)      # as before
        assert util.save_ply(str(tmp_path / "mesh.ply"), p, faces=f, **kw) == N
        raw = (tmp_path / "mesh.ply").read_bytes()
        assert raw == head(with_n, with_c, F) + vertex_bytes(with_n, with_c) + face_bytes
        # and parses back
        payload = raw.split(b"end_header\n", 1)[1]
        rec = np.frombuffer(payload[len(vertex_bytes(with_n, with_c)):], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert (rec["n"] == 3).all() and np.array_equal(rec["v"], f)
    import torch
    assert util.save_ply(str(tmp_path / "t.ply"), torch.from_numpy(p), faces=torch.from_numpy(f)) == N
    assert (tmp_path / "t.ply").read_bytes() == head(False, False, F) + vertex_bytes(False, False) + face_bytes
    assert util.save_ply(str(tmp_path / "none.ply"), p, faces=np.zeros((0, 3), np.int32)) == N
    assert (tmp_path / "none.ply").read_bytes() == head(False, False, 0) + vertex_bytes(False, False)
    for bad in (np.array([[0, 1, N]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError):
            util.save_ply(str(tmp_path / "bad.ply"), p, faces=bad)


def test_operator_is_registered_with_a_meta_kernel():
    import torch
    from relativepose_amd import ops
    assert "tsdf_mesh" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    ts, wt, cs, org = m(3, 27, 34, 20, dt=torch.int32), m(3, 27, 34, 20, dt=torch.int32), m(3, 3, 27, 34, 20, dt=torch.int32), m(3, 3, dt=torch.float64)
    p, n, c, v, k, t, kt = torch.ops.relpose.tsdf_mesh(ts, wt, cs, org, 0.25, 1, 500, 900)
    assert p.shape == n.shape == c.shape == (3, 500, 3) and p.dtype == n.dtype == torch.float64 and c.dtype == torch.float32
    assert v.shape == (3, 500) and v.dtype == torch.uint8 and k.shape == kt.shape == (3,) and k.dtype == kt.dtype == torch.int32
    assert t.shape == (3, 900, 3) and t.dtype == torch.int32
    assert torch.ops.relpose.tsdf_mesh(ts, wt, None, org, 0.25)[2].numel() == 0
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.tsdf_mesh(torch.ones(1, 2, 2, 2, dtype=torch.int32), torch.ones(1, 2, 2, 2, dtype=torch.int32), None,
                                    torch.zeros(1, 3, dtype=torch.float64), 0.5)


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_tsdf_mesh(None) == EINVAL
    buf = (C.c_double * 64)()                      # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    host = TS.host_arrays()
    calls = MS.mesh_einval_calls()
    assert len(calls) >= 35 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        assert lib.relpose_tsdf_mesh(C.byref(MS.mesh_args(_lib, p, host, kw))) == EINVAL, name
    assert buf[:] == [0.0] * 64
    W = lib.relpose_tsdf_mesh_workspace_bytes
    nblk = lambda n: (n + 255) // 256
    assert W(2, 3, 2, 2) >= 2 * 3 * 8 + 2 * 2 * nblk(12) * 4 + 2 * 12 * 5 and W(2, 3, 2, 2) % 256 == 0
    assert W(1, 256, 256, 128) - W(1, 256, 256, 64) == 2 * nblk(256 * 256 * 64) * 4 + 256 * 256 * 64 * 5     # per voxel an int and a byte
    for a in ((0, 3, 2, 2), (2, 0, 2, 2), (2, 3, -2, 2), (2, 3, 2, 0), (2, 2048, 1024, 512), (1, 1024, 1024, 700), (-1, 3, 2, 2),
              (1, 1024, 1024, 512)):                                           # the last: 5 cells >= 2^31 with 3 voxels below it
        assert W(*a) == 0, a
    assert W(1, 1024, 1024, 400) > 0 and W(3, 7, 1, 5) > 0
    assert lib.relpose_tsdf_surface_workspace_bytes(1, 1024, 1024, 512) > 0


def test_cli_flag_and_its_default():
    from relativepose_amd import evaluation as E
    assert E._cli_parser_completion().parse_args([]).mesh is False
    assert E._cli_parser_completion().parse_args(["--mine-pairs", "--fuse", "0.05", "--mesh"]).mesh is True
    for argv in (["--mesh"], ["--mine-pairs", "--mesh"], ["--method", "fgs", "--fuse", "0.1", "--mesh"], ["--reconstruct", "--mesh"]):
        with pytest.raises(SystemExit):
            E.main(argv)
