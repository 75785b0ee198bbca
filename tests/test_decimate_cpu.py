"""CPU: the numpy model of relpose_mesh_decimate (tests/decimate_model.py): its two statements against each other, the
properties the contract promises (members near their cluster, closed surfaces stay closed chains, a fine grid gives the mesh back, one cell
gives one vertex, the counters add up), every RELPOSE_EINVAL path of the entry point without a device, and the Python layers."""
import ctypes as C
import os

import numpy as np
import pytest

import decimate_model as DM
import decimate_scenes as DS
from components_model import counts
from tsdf_scenes import bits_equal, differ


@pytest.mark.parametrize("name", DS.ALL)
def test_array_model_equals_loop_model_bitwise(name):
    sc = DS.scene(name)
    for dedupe in (1, 0):
        want = DS.expected(name, dedupe)
        loops = DS.model(sc, dedupe, loops=True)
        assert differ(loops, want, DM.KEYS) == [], (name, dedupe)
    zero = DS.model(sc, 1, fill=0)                                             # the fill only shows where nothing is written
    for s in range(len(zero["n_points"])):
        n, nt = int(zero["n_points"][s]), int(zero["n_triangles"][s])
        assert all(bits_equal(zero[k][s, :n], want_k[s, :n]) for k, want_k in ((k, DS.expected(name)[k]) for k in ("points", "normals", "count")))
        assert bits_equal(zero["triangles"][s, :nt], DS.expected(name)["triangles"][s, :nt])
        assert not zero["points"][s, n:].any() and not zero["triangles"][s, nt:].any()


@pytest.mark.parametrize("name", DS.ALL)
def test_members_lie_within_a_cell_diagonal_and_the_counters_add_up(name):
    sc = DS.scene(name)
    m = sc["mesh"]
    cap, cap_tri = m["points"].shape[1], m["triangles"].shape[1]
    bound = np.sqrt(3.0) * sc["cell"] * (1.0 + 2.0 ** -30)                     # the mean of points of one cell stays in the cell
    for dedupe in (1, 0):
        got = DS.expected(name, dedupe)
        for s in range(len(got["n_points"])):
            nv, nt = counts(m["n_points"][s], m["n_triangles"][s], cap, cap_tri)
            vm, n = got["vertex_map"][s], int(got["n_points"][s])
            assert (vm[nv:] == -1).all() and vm.max(initial=-1) == n - 1
            inside = np.nonzero(vm >= 0)[0]
            d = np.linalg.norm(m["points"][s, inside] - got["points"][s, vm[inside]], axis=1)
            assert (d <= bound).all(), (name, s, d.max())
            assert np.array_equal(np.bincount(vm[inside], minlength=n), got["count"][s, :n])
            reps = np.array([inside[vm[inside] == c].min() for c in range(n)], np.int64)
            assert (np.diff(reps) > 0).all()                                   # numbered by smallest member
            nn = np.linalg.norm(got["normals"][s, :n], axis=1)
            assert (np.abs(nn - 1.0) < 1e-12)[nn != 0].all()
            survivors = int(got["n_triangles"][s])
            assert sum(int(got[k][s]) for k in DM.COUNTERS) + survivors == nt, (name, s)
            tm = got["tri_map"][s]
            assert (tm[nt:] == DM.BEYOND).all() and np.array_equal(tm[:nt][tm[:nt] >= 0], np.arange(survivors))
            assert [int((tm[:nt] == c).sum()) for c in (DM.BAD, DM.OUTSIDE, DM.DEGENERATE, DM.DUPLICATE)] == [int(got[k][s]) for k in DM.COUNTERS]
            t = got["triangles"][s, :survivors]
            assert ((t >= 0) & (t < n)).all() and (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
            if dedupe:
                k = np.argmin(t, 1)
                rot = np.stack([t[np.arange(len(t)), (k + j) % 3] for j in range(3)], 1)
                assert len(np.unique(rot, axis=0)) == len(t)
            else:
                assert got["duplicate_triangles"][s] == 0


@pytest.mark.parametrize("name", [f"{n}@{f}" for n in ("sphere", "two_balls") for f in DS.FACTORS])
def test_closed_surfaces_stay_closed_chains_without_dedupe(name):
    """a closed surface stays a closed 2-chain under a vertex map once degenerate rows are dropped: (a, b) occurs as often as (b, a)"""
    got = DS.expected(name, 0)
    assert got["outside_triangles"][0] == 0 and got["bad_triangles"][0] == 0 and got["degenerate_triangles"][0] > 0
    t = got["triangles"][0, :int(got["n_triangles"][0])].astype(np.int64)
    assert len(t) > 20
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(got["n_points"][0])
    fwd, back = np.bincount(e[:, 0] * n + e[:, 1], minlength=n * n), np.bincount(e[:, 1] * n + e[:, 0], minlength=n * n)
    assert np.array_equal(fwd, back)
    assert DS.expected(name, 1)["n_triangles"][0] <= got["n_triangles"][0]


def test_a_cell_below_the_vertex_spacing_gives_the_mesh_back():
    sc = DS.scene("sheet_once")
    m = sc["mesh"]
    nv, nt = int(m["n_points"][0]), int(m["n_triangles"][0])
    p = m["points"][0, :nv]
    gap = np.abs(p[:, None] - p[None]).max(2) + np.eye(nv) * 9.0               # two vertices share a cell only if every axis is within it
    cell = 0.05
    assert gap.min() > cell
    origin = p.min(0)[None] - 0.01
    dims = tuple(int(v) for v in np.floor((p.max(0) - origin[0]) / cell) + 1)
    got = DM.decimate(m, origin, cell, dims, 1, DM.before(m))
    assert got["n_points"][0] == nv and got["n_triangles"][0] == nt and all(got[k][0] == 0 for k in DM.COUNTERS)
    assert np.array_equal(got["vertex_map"][0, :nv], np.arange(nv)) and np.array_equal(got["tri_map"][0, :nt], np.arange(nt))
    assert bits_equal(got["triangles"][0, :nt], m["triangles"][0, :nt]) and (got["count"][0, :nv] == 1).all()
    assert np.abs(got["points"][0, :nv] - p).max() <= 2.0 ** -17 * cell        # the stated quantisation
    # The normal's stated quantisation, 2^-16, is that of the summed integers: llrint(n 32768) / 32768 is within 2^-16 of n per component.  The
    # output is that vector normalised, and normalising moves a component by up to sqrt(3) 2^-16 more (1.88e-5 > 2^-16 = 1.53e-5 was measured
    # here on random unit normals), so the bound is applied where the contract states it and the output is then demanded bit for bit.
    q = np.rint(m["normals"][0, :nv] * 32768.0)
    assert np.abs(q / 32768.0 - m["normals"][0, :nv]).max() <= 2.0 ** -16
    assert bits_equal(got["normals"][0, :nv], q / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])[:, None])
    assert np.abs(got["normals"][0, :nv] - m["normals"][0, :nv]).max() <= 2.0 ** -16 * (1.0 + np.sqrt(3.0))
    assert np.abs(got["colors"][0, :nv].astype(np.float64) - m["colors"][0, :nv].astype(np.float64)).max() <= 2.0 ** -17


def test_a_grid_of_one_cell_gives_one_vertex_and_no_triangle():
    for dedupe in (0, 1):
        got = DS.expected("one_cell", dedupe)
        nt = int(DS.scene("one_cell")["mesh"]["n_triangles"][0])
        assert got["n_points"][0] == 1 and got["count"][0, 0] == DS.ONE_CELL and got["n_triangles"][0] == 0
        assert got["degenerate_triangles"][0] == nt and got["bad_triangles"][0] == 0 and got["outside_triangles"][0] == 0
        assert (got["tri_map"][0, :nt] == DM.DEGENERATE).all() and got["valid"][0].tolist() == [1] + [0] * (len(got["valid"][0]) - 1)
    both = DS.expected("shared_edge")
    assert both["n_points"][0] == 1 and both["n_triangles"][0] == 0 and both["degenerate_triangles"][0] == 2


def test_pinned_counts_of_the_hand_built_scenes():
    fan, loose = DS.expected("fan", 1), DS.expected("fan", 0)
    assert fan["n_points"][0] == 4 and loose["n_triangles"][0] > fan["n_triangles"][0] >= 2 and fan["duplicate_triangles"][0] > 0
    assert loose["n_triangles"][0] == fan["n_triangles"][0] + fan["duplicate_triangles"][0]
    tie = DS.expected("bow_tie")
    assert tie["n_points"][0] == 2 and tie["n_triangles"][0] == 0 and tie["degenerate_triangles"][0] == 2
    sheet = DS.expected("sheet")
    assert sheet["outside_triangles"][0] > 0 and sheet["duplicate_triangles"][0] >= sheet["n_triangles"][0] // 2 > 10
    faces = DS.expected("faces")
    sc = DS.scene("faces")
    nv = int(sc["mesh"]["n_points"][0])
    lat = (sc["mesh"]["points"][0, :nv] - sc["origin"][0]) / sc["cell"]
    on_lattice = (lat == np.rint(lat)).all(1)
    want = ((lat >= 0) & (lat < np.array(sc["dims"]))).all(1)
    assert on_lattice.sum() >= 6 * 8 * 5 and np.array_equal((faces["vertex_map"][0, :nv] >= 0)[on_lattice], want[on_lattice])
    off = (faces["vertex_map"][0, :nv] >= 0)[~on_lattice].reshape(3, 4)       # per axis: past the far face, before it, before the origin, past it
    assert not off[:, 0].any() and not off[:, 2].any() and off[:, 3].all()     # (one ulp before the far face: p - origin may round onto it)
    assert DS.expected("bad_rows")["bad_triangles"][0] == 3
    bad = DS.expected("nonfinite")
    k = bad["vertex_map"][0, 0]
    assert bad["count"][0, k] >= 5 and bits_equal(bad["normals"][0, bad["vertex_map"][0, 5]], np.zeros(3))
    batch = DS.expected("batch")
    assert batch["n_points"][1] == 0 and batch["n_triangles"][1] == 0 and (batch["vertex_map"][1] == -1).all()
    trunc = DS.scene("truncated@2")["mesh"]
    assert trunc["n_triangles"][0] > trunc["triangles"].shape[1]
    assert DS.expected("no_colors")["colors"] is None


def test_default_grid_covers_the_finite_vertices():
    assert max(DM.default_grid(DS.scene("nonfinite")["mesh"], 0.25)[1]) > 1024  # a vertex at 1e308 is finite: no grid within the limits covers it
    for name in ("sheet", "faces", "batch"):
        sc = DS.scene(name)
        origin, dims = DM.default_grid(sc["mesh"], sc["cell"])
        got = DM.decimate(sc["mesh"], origin, sc["cell"], dims, 1, DM.before(sc["mesh"]))
        m = sc["mesh"]
        for s in range(len(origin)):
            nv = min(max(int(m["n_points"][s]), 0), m["points"].shape[1])
            fin = np.isfinite(m["points"][s, :nv]).all(1)
            assert np.array_equal(got["vertex_map"][s, :nv] >= 0, fin) and got["outside_triangles"][s] <= (~fin).sum() * 900


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_mesh_decimate(None) == EINVAL
    buf = (C.c_double * 2048)()                    # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    ptrs = {k: p + 512 * i for i, k in enumerate(DS.POINTERS)}                 # every pointer an address of its own
    host = DS.host_arrays()
    calls = DS.einval_calls()
    assert len(calls) >= 50 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        assert lib.relpose_mesh_decimate(C.byref(DS.decimate_args(_lib, ptrs, host, kw))) == EINVAL, name
    assert buf[:] == [0.0] * 2048
    W = lib.relpose_mesh_decimate_workspace_bytes
    assert W(2, 8, 6, 3, 5, 2) > 0 and W(2, 8, 6, 3, 5, 2) % 256 == 0
    assert W(1, 1 << 20, 1 << 21, 64, 64, 64) >= (1 << 20) * 80 + (1 << 18) * 4 + (1 << 22) * 20
    for a in ((0, 8, 6, 3, 5, 2), (-1, 8, 6, 3, 5, 2), (2, 0, 6, 3, 5, 2), (2, 8, 0, 3, 5, 2), (2, 1 << 28, 6, 3, 5, 2), (2, 8, 1 << 28, 3, 5, 2),
              (2, 8, 6, 0, 5, 2), (2, 8, 6, 3, -1, 2), (2, 8, 6, 3, 5, 0), (2, 8, 6, 1025, 5, 2), (2, 8, 6, 3, 1025, 2), (2, 8, 6, 3, 5, 1025),
              (2, 8, 6, 1024, 1024, 64), (1, 8, 6, 1024, 1024, 128)):
        assert W(*a) == 0, a
    assert W(1, 8, 6, 1024, 1024, 127) > 0 and W(1, (1 << 29) - 1, 1, 1, 1, 1) > 0


def test_operator_is_registered_with_a_meta_kernel():
    import torch
    from relativepose_amd import ops
    assert "mesh_decimate" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
    args = (m(3, 500, 3, dt=f64), m(3, 500, 3, dt=f64), m(3, 500, 3, dt=f32), m(3, dt=i32), m(3, 900, 3, dt=i32), m(3, dt=i32), m(3, 3, dt=f64))
    out = torch.ops.relpose.mesh_decimate(*args, 0.1, 8, 8, 8)
    assert [tuple(o.shape) for o in out] == [(3, 500, 3)] * 3 + [(3, 500), (3,), (3, 500), (3, 900, 3), (3,), (3, 500), (3, 900)] + [(3,)] * 4
    assert [o.dtype for o in out] == [f64, f64, f32, u8] + [i32] * 10
    assert torch.ops.relpose.mesh_decimate(*args[:2], None, *args[3:], 0.1, 8, 8, 8, False)[2].numel() == 0
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.mesh_decimate(torch.zeros(1, 3, 3, dtype=f64), torch.zeros(1, 3, 3, dtype=f64), None, torch.zeros(1, dtype=i32),
                                        torch.zeros(1, 1, 3, dtype=i32), torch.zeros(1, dtype=i32), torch.zeros(1, 3, dtype=f64), 1.0, 1, 1, 1)


def test_decimate_summary_and_the_cli_flag():
    from relativepose_amd import evaluation as E
    s = E.mesh_decimate_summary([(100, 25, 0.25, 1.0), (200, 100, 0.75, 0.5), (0, 0, float("nan"), float("nan"))])
    assert s == {"mesh_decimated_triangles_median": 25.0, "mesh_decimated_share_median": 0.375, "mesh_decimated_dist_median": 0.5,
                 "mesh_decimated_within_median": 0.75}
    P = E._cli_parser_completion()
    assert P.parse_args([]).mesh_decimate is None
    assert P.parse_args(["--mine-pairs", "--fuse", "0.05", "--mesh", "--mesh-decimate", "2"]).mesh_decimate == 2
    for argv in (["--mesh-decimate", "2"], ["--mine-pairs", "--fuse", "0.1", "--mesh-decimate", "2"],
                 ["--mine-pairs", "--fuse", "0.1", "--mesh", "--mesh-decimate", "0"]):
        with pytest.raises(SystemExit):
            E.main(argv)
