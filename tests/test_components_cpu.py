"""CPU: the numpy model of relpose_mesh_components / relpose_mesh_filter (tests/components_model.py) against scipy's
connected components, the component counts of the project's own mesh fixtures, the properties of the filter, and every RELPOSE_EINVAL path of
the two entry points without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import components_model as CM
import components_scenes as CS
import mesh_scenes as MS
from tsdf_scenes import bits_equal

ALL = [("hand", n) for n in CS.HAND] + [("volume", n) for n in CS.VOLUMES] + [("volume", "room_suncg_16")]


def mesh_of(kind, name):
    return CS.hand(name) if kind == "hand" else CS.volume_mesh(name)


@pytest.mark.parametrize("kind,name", ALL)
def test_partition_is_scipys_and_numbered_by_smallest_vertex(kind, name):
    m = mesh_of(kind, name)
    cap_comp, got = CS.expected(kind, name)
    S, cap = m["points"].shape[:2]
    for s in range(S):
        nv, nt = CM.counts(m["n_points"][s], m["n_triangles"][s], cap, m["triangles"].shape[1])
        n, lab = CM.scipy_partition(m["triangles"][s, :nt], nv)
        vl = got["vertex_label"][s, :nv]
        assert got["n_components"][s] == n and (got["vertex_label"][s, nv:] == -1).all() and (got["tri_label"][s, nt:] == -1).all()
        assert np.array_equal(vl < 0, lab < 0)
        used = vl >= 0
        pairs = np.unique(np.stack([vl[used], lab[used]], 1), axis=0)           # a bijection between the two numberings
        assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
        roots = got["comp_root"][s, :n]
        assert (np.diff(roots) > 0).all()                                      # ascending smallest index
        for c in range(n):
            members = np.nonzero(vl == c)[0]
            assert members.min() == roots[c] and len(members) == got["comp_vertices"][s, c]
        assert (got["comp_root"][s, n:] == -1).all() and (got["comp_triangles"][s, n:] == 0).all() and (got["comp_area"][s, n:] == 0).all()
        tl = got["tri_label"][s, :nt]
        assert (tl < 0).sum() == got["bad_triangles"][s] and got["comp_triangles"][s].sum() == (tl >= 0).sum()
        good = tl >= 0
        assert all((vl[m["triangles"][s, :nt][good][:, k]] == tl[good]).all() for k in range(3))


TABLE = {  # case: per scene (vertices, unused, triangles, components, largest, smallest)
    "noise": [(1542, 109, 1963, 30, 1826, 1)], "edge_state": [(68, 17, 39, 7, 26, 1)],
    "empty_in_batch": [(132, 108, 16, 4, 11, 1), (0, 0, 0, 0, None, None), (122, 101, 9, 6, 3, 1)],
    "sphere": [(1328, 0, 2652, 1, 2652, 2652)], "room_suncg_16": [(2652, 0, 5120, 1, 5120, 5120)]}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_component_counts_of_the_mesh_fixtures(name):
    m = CS.volume_mesh(name)
    _, got = CS.expected("volume", name)
    for s, (nv, unused, nt, n, largest, smallest) in enumerate(TABLE[name]):
        assert m["n_points"][s] == nv and m["n_triangles"][s] == nt and got["n_components"][s] == n and got["bad_triangles"][s] == 0
        assert (got["vertex_label"][s, :nv] < 0).sum() == unused
        if n:
            assert got["comp_triangles"][s, :n].max() == largest and got["comp_triangles"][s, :n].min() == smallest


def test_two_balls_are_two_closed_surfaces():
    from relativepose_amd import evaluation as E
    m = CS.volume_mesh("two_balls")
    _, got = CS.expected("volume", "two_balls")
    assert got["n_components"][0] == 2 and (got["vertex_label"][0, :m["n_points"][0]] >= 0).all()
    for c in range(2):
        keep = np.zeros((1, got["comp_root"].shape[1]), bool)
        keep[0, c] = True
        out = CM.filter_outputs(m, got, keep, 1, filter_before(m))
        V, F = int(out["n_points"][0]), int(out["n_triangles"][0])
        st = E.mesh_stats(out)[0]
        edges = np.unique(np.sort(MS.MM.directed_edges(out["triangles"][0, :F]), 1), axis=0)
        assert st["border_edges"] == 0 and st["nonmanifold_edges"] == 0 and V - len(edges) + F == 2
        assert V == got["comp_vertices"][0, c] and F == got["comp_triangles"][0, c]
    assert got["comp_triangles"][0, 0] != got["comp_triangles"][0, 1]


def test_area_terms_round_clamp_and_drop_non_finite():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3e9, 0, 0], [0, 3e9, 0], [np.nan, 0, 0], [np.inf, 0, 0], [1e200, 0, 0], [0, 1e200, 0]], np.float64)
    t = np.array([[0, 1, 2], [0, 3, 4], [0, 1, 5], [0, 6, 2], [0, 7, 8], [1, 1, 2]])
    assert CM.area_terms(p, t, 1024.0).tolist() == [512, 2 ** 31, 0, 0, 0, 0]
    assert CM.area_terms(p, t[:1], 3.0).tolist() == [2] and CM.area_terms(p, t[:1], 5.0).tolist() == [2]      # 1.5 and 2.5: ties to even
    m = CS.hand("bad_rows")
    _, got = CS.expected("hand", "bad_rows")
    assert got["bad_triangles"][0] == 3 and got["comp_area"].max() >= 2 ** 31


def filter_before(m):
    S, cap = m["points"].shape[:2]
    return {"points": np.full((S, cap, 3), -7.5), "normals": np.full((S, cap, 3), 9.25),
            "colors": None if m["colors"] is None else np.full((S, cap, 3), -3.0, np.float32), "valid": np.full((S, cap), 77, np.uint8),
            "n_points": np.full(S, -7, np.int32), "triangles": np.full(m["triangles"].shape, MS.TRI_FILL, np.int32),
            "n_triangles": np.full(S, -7, np.int32), "vertex_map": np.full((S, cap), -5, np.int32)}


@pytest.mark.parametrize("kind,name", [("hand", "random"), ("hand", "batch"), ("hand", "bad_rows"), ("volume", "noise"), ("volume", "empty_in_batch")])
def test_filter_properties(kind, name):
    m = mesh_of(kind, name)
    cap_comp, comps = CS.expected(kind, name)
    S, cap = m["points"].shape[:2]
    cap_tri = m["triangles"].shape[1]
    before = filter_before(m)
    # keep-all with drop_unused = 0: the identity on the vertices; the triangles without their bad rows
    same = CM.filter_outputs(m, comps, np.ones((S, cap_comp), bool), 0, before)
    for s in range(S):
        nv, nt = CM.counts(m["n_points"][s], m["n_triangles"][s], cap, cap_tri)
        assert same["n_points"][s] == nv and same["n_triangles"][s] == nt - comps["bad_triangles"][s]
        assert all(bits_equal(same[k][s, :nv], m[k][s, :nv]) for k in ("points", "normals", "colors") if m[k] is not None)
        assert np.array_equal(same["vertex_map"][s, :nv], np.arange(nv)) and (same["vertex_map"][s, nv:] == -1).all()
        assert np.array_equal(same["triangles"][s, :same["n_triangles"][s]], m["triangles"][s, :nt][comps["tri_label"][s, :nt] >= 0])
        assert (same["points"][s, nv:] == -7.5).all() and (same["triangles"][s, same["n_triangles"][s]:] == MS.TRI_FILL).all()
    # a selection: every surviving index is below the new count, filtering twice is filtering once
    keep = (comps["comp_triangles"] >= 2) & (np.arange(cap_comp)[None] % 3 != 1)
    once = CM.filter_outputs(m, comps, keep, 1, before)
    for s in range(S):
        n, nt = int(once["n_points"][s]), int(once["n_triangles"][s])
        t = once["triangles"][s, :nt]
        assert nt == comps["comp_triangles"][s][keep[s]].sum() and n == comps["comp_vertices"][s][keep[s]].sum()
        assert nt == 0 or (t.min() >= 0 and t.max() < n)
        assert (once["valid"][s] == (np.arange(cap) < n)).all()
    again_in = dict(once, area_scale=m["area_scale"])
    c2 = CM.components(again_in, cap_comp, m["area_scale"])
    assert np.array_equal(c2["n_components"], keep.sum(1)) and (c2["bad_triangles"] == 0).all()
    twice = CM.filter_outputs(again_in, c2, np.arange(cap_comp)[None] < c2["n_components"][:, None], 1, before)
    for s in range(S):
        n, nt = int(once["n_points"][s]), int(once["n_triangles"][s])
        assert twice["n_points"][s] == n and twice["n_triangles"][s] == nt
        assert all(bits_equal(twice[k][s, :n], once[k][s, :n]) for k in ("points", "normals", "colors") if m[k] is not None)
        assert bits_equal(twice["triangles"][s, :nt], once["triangles"][s, :nt])
        for c, q in enumerate(np.nonzero(keep[s])[0]):                        # the statistics travel with the components
            assert all(c2[k][s, c] == comps[k][s, q] for k in ("comp_vertices", "comp_triangles", "comp_area"))


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_mesh_components(None) == EINVAL and lib.relpose_mesh_filter(None) == EINVAL
    buf = (C.c_double * 256)()                     # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    rounds = C.c_int(-9)
    for calls, pointers, make, fn in ((CS.components_einval_calls(), CS.COMPONENT_POINTERS, CS.components_args, lib.relpose_mesh_components),
                                      (CS.filter_einval_calls(), CS.FILTER_POINTERS, CS.filter_args, lib.relpose_mesh_filter)):
        ptrs = {k: p + 64 * i for i, k in enumerate(pointers)}                 # every pointer an address of its own
        assert len(calls) >= 30 and len({n for n, _ in calls}) == len(calls)
        for name, kw in calls:
            a = make(_lib, ptrs, kw)
            if fn is lib.relpose_mesh_components:
                a.rounds_host = C.addressof(rounds)
            assert fn(C.byref(a)) == EINVAL, name
    assert buf[:] == [0.0] * 256 and rounds.value == -9
    for W, per_scene in ((lib.relpose_mesh_components_workspace_bytes, lambda cap, ct: cap * 5),
                         (lib.relpose_mesh_filter_workspace_bytes, lambda cap, ct: cap * 4)):
        assert W(2, 8, 6) > 0 and W(2, 8, 6) % 256 == 0
        assert W(1, 1 << 20, 1 << 21) >= per_scene(1 << 20, 1 << 21) and W(3, 1 << 20, 1 << 21) >= 3 * per_scene(1 << 20, 1 << 21)
        for a in ((0, 8, 6), (-1, 8, 6), (2, 0, 6), (2, 8, 0), (2, -8, 6), (2, 1 << 28, 6), (2, 8, 1 << 28), (1, 1 << 29, 6)):
            assert W(*a) == 0, a
        assert W(1, (1 << 29) - 1, 1) > 0


def test_operators_are_registered_with_meta_kernels():
    import torch
    from relativepose_amd import ops
    assert "mesh_components" in ops.OPS and "mesh_filter" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
    pts, npts, tri, ntri = m(3, 500, 3, dt=f64), m(3, dt=i32), m(3, 900, 3, dt=i32), m(3, dt=i32)
    out = torch.ops.relpose.mesh_components(pts, npts, tri, ntri, 1024.0, 7)
    shapes = [(3, 500), (3, 900), (3,), (3,), (3, 7), (3, 7), (3, 7), (3, 7), (1,)]
    assert [tuple(o.shape) for o in out] == shapes and [o.dtype for o in out] == [i32] * 7 + [torch.int64, i32]
    got = torch.ops.relpose.mesh_filter(pts, m(3, 500, 3, dt=f64), m(3, 500, 3, dt=f32), npts, tri, ntri, out[0], out[1], m(3, 7, dt=u8))
    assert [tuple(o.shape) for o in got] == [(3, 500, 3)] * 3 + [(3, 500), (3,), (3, 900, 3), (3,), (3, 500)]
    assert [o.dtype for o in got] == [f64, f64, f32, u8, i32, i32, i32, i32]
    assert torch.ops.relpose.mesh_filter(pts, m(3, 500, 3, dt=f64), None, npts, tri, ntri, out[0], out[1], m(3, 7, dt=u8))[2].numel() == 0
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.mesh_components(torch.zeros(1, 3, 3, dtype=f64), torch.zeros(1, dtype=i32), torch.zeros(1, 1, 3, dtype=i32),
                                          torch.zeros(1, dtype=i32), 1.0, 1)


def test_component_stats_and_the_cli_flag():
    from relativepose_amd import evaluation as E
    _, got = CS.expected("volume", "empty_in_batch")
    st = E.mesh_component_stats(got)
    assert [s["components"] for s in st] == [4, 0, 6] and [s["small_triangles"] for s in st] == [5, 0, 6]
    assert st[0]["largest_share"] == 11 / 16 and np.isnan(st[1]["largest_share"]) and st[2]["largest_share"] == 3 / 9
    P = E._cli_parser_completion()
    assert P.parse_args([]).mesh_min_component is None
    assert P.parse_args(["--mine-pairs", "--fuse", "0.05", "--mesh", "--mesh-min-component", "20"]).mesh_min_component == 20
    for argv in (["--mesh-min-component", "5"], ["--mine-pairs", "--fuse", "0.1", "--mesh-min-component", "5"],
                 ["--mine-pairs", "--fuse", "0.1", "--mesh", "--mesh-min-component", "0"]):
        with pytest.raises(SystemExit):
            E.main(argv)
