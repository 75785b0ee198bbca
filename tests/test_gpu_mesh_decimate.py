"""GPU: relpose_mesh_decimate.  Every output is compared bit for bit with tests/decimate_model.py, written into pre-filled
buffers so that rows beyond the counts are shown untouched: hand-built meshes (one cell, two cells, a fan whose rim collapses to duplicates,
1500 vertices on one accumulator row, vertices on cell faces and one ulp off the grid, NaN / inf points, normals and colours, bad rows,
shuffled rows and vertex ids, a batch with an empty and a truncated scene), the meshes of mesh_scenes' volumes and of two balls at factors 2
and 3, with and without dedupe, colours and tri_map; repeats and batch invariance; the operator and the Python layers against the C ABI;
fuse_views(decimate=K); every RELPOSE_EINVAL path with pre-filled outputs.  Every test runs under a time limit of its own: a watchdog ends
the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import components_scenes as CS
import decimate_model as DM
import decimate_scenes as DS
import mesh_scenes as MS
import tsdf_scenes as TS
from gpu_util import log
from relativepose_amd import synth

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few
MESH_IN = ("points", "normals", "colors", "n_points", "triangles", "n_triangles")
OUT_FIELD = {k: "out_" + k for k in ("points", "normals", "colors", "valid", "n_points", "count", "triangles", "n_triangles")}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    import torch
    return torch.device("cuda:0")


def up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def dev_mesh(m):
    return {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in m.items()}


def decimate_raw(sc, dedupe, tri_map=True, dm=None, rc=0):
    """relpose_mesh_decimate through the C ABI into outputs pre-filled with decimate_model.FILL -> what it left, as numpy"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    m = sc["mesh"]
    dm = dev_mesh(m) if dm is None else dm
    S, cap = m["points"].shape[:2]
    cap_tri = m["triangles"].shape[1]
    gx, gy, gz = sc["dims"]
    nbytes = L.relpose_mesh_decimate_workspace_bytes(S, cap, cap_tri, gx, gy, gz)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    out = {k: up(v) for k, v in DM.before(m).items()}
    origin = np.array(sc["origin"], dtype=np.float64)
    a = _lib.MeshDecimateArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.gx, a.gy, a.gz, a.dedupe, a.cell = S, cap, cap_tri, gx, gy, gz, dedupe, sc["cell"]
    for k in MESH_IN:
        setattr(a, k, 0 if dm[k] is None else dm[k].data_ptr())
    a.origin_host = origin.ctypes.data
    for k in DM.KEYS:
        setattr(a, OUT_FIELD.get(k, k), 0 if out[k] is None or (k == "tri_map" and not tri_map) else out[k].data_ptr())
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_mesh_decimate(C.byref(a)) == rc
    origin[:] = np.nan                                                         # the host origin is the caller's again
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


@pytest.mark.parametrize("name", DS.ALL)
def test_scenes_match_the_model_bitwise(name):
    sc = DS.scene(name)
    dm = dev_mesh(sc["mesh"])
    for dedupe in (1, 0):
        want = DS.expected(name, dedupe)
        got = decimate_raw(sc, dedupe, dm=dm)
        bad = TS.differ(got, want, DM.KEYS)
        log(f"mesh_decimate_{name}_dedupe{dedupe}", differ=bad, n_points=got["n_points"], n_triangles=got["n_triangles"],
            **{k: got[k] for k in DM.COUNTERS})
        assert bad == [], (name, dedupe, bad, got["n_points"], want["n_points"], got["n_triangles"], want["n_triangles"])
    again = decimate_raw(sc, 0, dm=dm)                                         # a second run
    assert TS.differ(again, got, DM.KEYS) == []
    no_map = decimate_raw(sc, 0, tri_map=False, dm=dm)                         # tri_map = NULL: everything else the same
    assert TS.differ(no_map, got, [k for k in DM.KEYS if k != "tri_map"]) == [] and (no_map["tri_map"] == DM.FILL["tri_map"]).all()
    S = sc["mesh"]["points"].shape[0]
    if S > 1:                                                                  # a scene alone is the scene inside its batch
        for s in range(S):
            one = decimate_raw(DS.scene_of(sc, s), 0)
            assert all(TS.bits_equal(one[k][0], got[k][s]) for k in DM.KEYS if got[k] is not None), (name, s)


def test_what_the_scenes_are_there_for():
    for dedupe in (1, 0):
        one = decimate_raw(DS.scene("one_cell"), dedupe)
        assert one["n_points"][0] == 1 and one["count"][0, 0] == DS.ONE_CELL and one["n_triangles"][0] == 0
    fan, loose = decimate_raw(DS.scene("fan"), 1), decimate_raw(DS.scene("fan"), 0)
    assert fan["duplicate_triangles"][0] > 0 and loose["duplicate_triangles"][0] == 0
    assert loose["n_triangles"][0] == fan["n_triangles"][0] + fan["duplicate_triangles"][0]
    assert decimate_raw(DS.scene("no_colors"), 1)["colors"] is None
    assert DS.scene("bow_tie")["dims"] == (3, 5, 2) and DS.scene("faces")["dims"] == (3, 5, 2)      # non-cubic grids
    batch = decimate_raw(DS.scene("truncated@2"), 1)
    assert batch["n_points"][1] == 0 and (batch["vertex_map"][1] == -1).all() and (batch["tri_map"][1] == DM.BEYOND).all()


def volume_state(name):
    c = CS.volume_case(name)
    ts = c["tsdf_sum"]
    S, nz, ny, nx = ts.shape
    return {"tsdf_sum": up(ts.astype(np.int32)), "weight": up(c["weight"].astype(np.int32)),
            "color_sum": None if c["color_sum"] is None else up(c["color_sum"].view(np.int32)),
            "origin": np.ascontiguousarray(c["origin"], dtype=np.float64), "dims": (nx, ny, nz), "voxel": c["voxel"]}, c["min_weight"]


def test_operator_and_python_layers_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import ops, util  # noqa: F401
    sc = DS.scene("batch")
    m = sc["mesh"]
    dm = dev_mesh(m)
    zero = DS.model(sc, 1, fill=0)                                             # the shim and the operator pre-fill with zeros
    raw = decimate_raw(sc, 1, dm=dm)
    for s in range(3):
        n, nt = int(raw["n_points"][s]), int(raw["n_triangles"][s])
        assert TS.bits_equal(raw["points"][s, :n], zero["points"][s, :n]) and TS.bits_equal(raw["triangles"][s, :nt], zero["triangles"][s, :nt])
    with pytest.raises(ValueError):                                            # a truncated scene needs truncated=True
        util.mesh_decimate_dev(dm, sc["cell"], sc["origin"], sc["dims"])
    shim = util.mesh_decimate_dev(dm, sc["cell"], sc["origin"], sc["dims"], True, truncated=True)
    assert set(shim) == set(DM.KEYS) | {"decimate_origin", "decimate_dims", "decimate_cell"} and shim["decimate_dims"] == sc["dims"]
    op = torch.ops.relpose.mesh_decimate(*(dm[k] for k in MESH_IN), up(sc["origin"]), sc["cell"], *sc["dims"], True, True)
    assert tuple(util.DECIMATE_KEYS) == DM.KEYS
    for got in ({k: shim[k].cpu().numpy() for k in DM.KEYS}, {k: v.cpu().numpy() for k, v in zip(DM.KEYS, op)}):
        assert TS.differ(got, zero, DM.KEYS) == []
    meta = torch.ops.relpose.mesh_decimate(*(dm[k].to("meta") for k in MESH_IN), up(sc["origin"]).to("meta"), sc["cell"], *sc["dims"], True, True)
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(meta, op))
    loose = util.mesh_decimate_dev(dm, sc["cell"], sc["origin"], sc["dims"], False, truncated=True)
    assert TS.differ({k: loose[k].cpu().numpy() for k in DM.KEYS}, DS.model(sc, 0, fill=0), DM.KEYS) == []
    # the default grid: the finite vertices' own box, computed on the device
    for name in ("sheet", "faces", "no_colors"):
        one = DS.scene(name)
        d1 = dev_mesh(one["mesh"])
        origin, dims = DM.default_grid(one["mesh"], 0.3)
        o, d = util.mesh_decimate_grid(d1, 0.3)
        assert TS.bits_equal(o, origin) and d == dims
        auto = util.mesh_decimate_dev(d1, 0.3)
        want = DM.decimate(one["mesh"], origin, 0.3, dims, 1, DM.before(one["mesh"], 0))
        assert TS.differ({k: (None if auto[k] is None else auto[k].cpu().numpy()) for k in DM.KEYS}, want, DM.KEYS) == [], name
        assert (auto["outside_triangles"] == 0).all()
    with pytest.raises(ValueError):
        util.mesh_decimate_dev(dev_mesh(DS.scene("nonfinite")["mesh"]), 0.25)     # a vertex at 1e308: no grid within the limits covers it
    with pytest.raises(ValueError):
        util.mesh_decimate_dev(d1, 0.0)
    # the volume's grid: the extracted mesh on the state's origin, coarsened
    for name, factor in (("sphere", 2), ("empty_in_batch", 3)):
        st, mw = volume_state(name)
        vm = util.tsdf_mesh_dev(st, mw)
        dec = util.mesh_decimate_volume_dev(vm, st, factor)
        vs = DS.scene(f"{name}@{factor}")
        assert dec["decimate_dims"] == vs["dims"] and dec["decimate_cell"] == vs["cell"]
        want = DS.model(vs, 1, fill=0)
        for s in range(len(want["n_points"])):                                 # (the extracted mesh has capacities of its own)
            n, nt = int(want["n_points"][s]), int(want["n_triangles"][s])
            assert int(dec["n_points"][s]) == n and int(dec["n_triangles"][s]) == nt
            assert all(TS.bits_equal(dec[k][s, :n].cpu().numpy(), want[k][s, :n]) for k in ("points", "normals", "count") if want[k] is not None)
            assert want["colors"] is None or TS.bits_equal(dec["colors"][s, :n].cpu().numpy(), want["colors"][s, :n])
            assert TS.bits_equal(dec["triangles"][s, :nt].cpu().numpy(), want["triangles"][s, :nt])
            assert all(int(dec[k][s]) == int(want[k][s]) for k in DM.COUNTERS)
    with pytest.raises(ValueError):
        util.mesh_decimate_volume_dev(vm, st, 0)


def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, cap, cap_tri = 2, 8, 6
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    tri = torch.tensor([[0, 1, 2], [2, 3, 4], [5, 6, 7], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.int32, device=dev()).repeat(S, 1, 1).contiguous()
    pts = torch.tensor([[-0.9, 0.6, 2.1], [-0.4, 0.6, 2.1], [-0.9, 1.1, 2.1], [0.1, 1.1, 2.1], [0.1, 1.6, 2.6], [-0.9, 2.6, 2.6], [-0.4, 2.6, 2.6],
                        [0.1, 2.6, 2.1]], dtype=torch.float64, device=dev())
    off = torch.tensor([[0.0, 0.0, 0.0], [1.0, -0.5, -2.0]], dtype=torch.float64, device=dev())     # scene 1 around its own origin (0, 0, 0)
    src = {"points": (pts[None] + off[:, None]).contiguous(), "normals": f((S, cap, 3), 0.5, torch.float64), "colors": f((S, cap, 3), 0.25, torch.float32),
           "n_points": f((S,), 8, torch.int32), "triangles": tri, "n_triangles": f((S,), 4, torch.int32)}
    mesh = {k: v.cpu().numpy() for k, v in src.items()}
    out = {OUT_FIELD.get(k, k): up(v) for k, v in DM.before(mesh).items()}
    before = {k: v.clone() for k, v in out.items()}
    ws = torch.empty(L.relpose_mesh_decimate_workspace_bytes(S, cap, cap_tri, 3, 5, 2) + 512, dtype=torch.uint8, device=dev())
    ptrs = {k: {**src, **out}[k].data_ptr() for k in DS.POINTERS}
    host = DS.host_arrays()
    for name, kw in DS.einval_calls():
        a = DS.decimate_args(_lib, ptrs, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256)
        a.stream = _lib.stream_ptr()
        assert L.relpose_mesh_decimate(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], before[k]) for k in before)
    a = DS.decimate_args(_lib, ptrs, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256)
    a.stream = _lib.stream_ptr()
    assert L.relpose_mesh_decimate(C.byref(a)) == 0                            # the base call itself is valid
    torch.cuda.synchronize()
    want = DM.decimate(mesh, np.array(DS.HOST["org"]).reshape(2, 3), 0.5, (3, 5, 2), 1, DM.before(mesh))
    assert TS.differ({k: out[OUT_FIELD.get(k, k)].cpu().numpy() for k in DM.KEYS}, want, DM.KEYS) == []
    assert out["out_n_points"].tolist() == [8, 8] and out["out_n_triangles"].tolist() == [3, 3] and out["degenerate_triangles"].tolist() == [1, 1]
    W = L.relpose_mesh_decimate_workspace_bytes
    for bad in ((0, 8, 6, 3, 5, 2), (2, 0, 6, 3, 5, 2), (2, 8, 0, 3, 5, 2), (2, 1 << 28, 6, 3, 5, 2), (2, 8, 6, 0, 5, 2), (2, 8, 6, 3, 1025, 2),
                (2, 8, 6, 1024, 1024, 64)):
        assert W(*bad) == 0, bad


def test_fuse_views_decimates_only_when_asked():
    """synth.render_scene(7, 4, "suncg", 16) fused at voxel 0.25 (test_gpu_mesh.py's room): without decimate fuse_views(mesh=True) is what it
    was -- util.tsdf_mesh_dev of its state, with the keys it had; with decimate=2 it is the model's decimation of that mesh on the volume's
    grid, with fewer triangles; after min_component when both are given."""
    from relativepose_amd import evaluation as E, util
    sc = synth.render_scene(7, 4, "suncg", 16)
    depth, rgb = up(sc["depth"].astype(np.float32)), up(sc["rgb"].astype(np.float32))
    mesh = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True)
    assert set(mesh) == set(MS.MESH_KEYS) | {"origin", "dims", "voxel", "state"}
    direct = util.tsdf_mesh_dev(mesh["state"], 1)
    assert all(TS.bits_equal(mesh[k].cpu().numpy(), direct[k].cpu().numpy()) for k in MS.MESH_KEYS)
    dec = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True, decimate=2)
    hm = {k: (None if mesh[k] is None else mesh[k].cpu().numpy()) for k in MS.MESH_KEYS}
    _, nz, ny, nx = mesh["state"]["tsdf_sum"].shape
    dims = tuple(-(-n // 2) for n in (nx, ny, nz))
    want = DM.decimate(hm, np.asarray(mesh["origin"], np.float64).reshape(1, 3), 0.5, dims, 1, DM.before(hm, 0))
    assert TS.differ({k: dec[k].cpu().numpy() for k in DM.KEYS}, want, DM.KEYS) == []
    nt, nd = int(mesh["n_triangles"][0]), int(dec["n_triangles"][0])
    assert 0 < nd < nt and int(dec["decimated_from"][1][0]) == nt and 0 < int(dec["n_points"][0]) < int(mesh["n_points"][0])
    st = E.mesh_stats(dec)[0]
    assert st["triangles"] == nd and st["area"] > 0
    both, part = E.decimate_mesh(mesh, 2)
    assert part[:2] == (nt, nd) and 0 < part[2] <= np.sqrt(3.0) * 0.5 and 0 < part[3] <= 1.0
    assert all(TS.bits_equal(both[k].cpu().numpy(), dec[k].cpu().numpy()) for k in DM.KEYS)
    log("mesh_decimate_room", before_after=(nt, nd), dist=part[2], within=part[3], **{k: int(dec[k][0]) for k in DM.COUNTERS}, **st)
    N = 20
    clean = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True, min_component=N)
    chain = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True, min_component=N, decimate=2)
    after = util.mesh_decimate_volume_dev(clean, clean["state"], 2)
    assert all(TS.bits_equal(chain[k].cpu().numpy(), after[k].cpu().numpy()) for k in DM.KEYS) and "components" in chain
    with pytest.raises(ValueError):
        E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, decimate=2)
