"""GPU: relpose_tsdf_mesh (marching cubes over a TSDF volume).  On every case of tests/mesh_scenes.py the vertex outputs
are relpose_tsdf_surface's bit for bit and the triangles the numpy model's; batch invariance and repeatability; the overflow of cap_tri and
of cap; the operator and the shim against the C ABI; every RELPOSE_EINVAL path with pre-filled outputs; and a rendered room fused and
meshed end to end.  Every test runs under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import mesh_model as MM
import mesh_scenes as MS
import tsdf_scenes as TS
from gpu_util import log
from relativepose_amd import synth

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    import torch
    return torch.device("cuda:0")


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


def device_state(c, scenes=None):
    """a case of mesh_scenes (or some of its scenes) as tsdf_fuse_dev's state"""
    sl = slice(None) if scenes is None else scenes
    ts = c["tsdf_sum"][sl]
    S, nz, ny, nx = ts.shape
    return {"tsdf_sum": up(ts, np.int32), "weight": up(c["weight"][sl], np.int32),
            "color_sum": None if c["color_sum"] is None else up(c["color_sum"][sl].view(np.int32), np.int32),
            "origin": np.ascontiguousarray(c["origin"][sl], dtype=np.float64), "dims": (nx, ny, nz), "voxel": c["voxel"]}


def filled_outputs(S, cap, cap_tri, colours):
    import torch
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    return {"points": f((S, cap, 3), TS.FILL["points"], torch.float64), "normals": f((S, cap, 3), TS.FILL["normals"], torch.float64),
            "colors": f((S, cap, 3), TS.FILL["colors"], torch.float32) if colours else None, "valid": f((S, cap), 77, torch.uint8),
            "n_points": f((S,), -7, torch.int32), "triangles": f((S, cap_tri, 3), MS.TRI_FILL, torch.int32), "n_triangles": f((S,), -7, torch.int32)}


def mesh_raw(st, min_weight, cap, cap_tri, spare_rows=0):
    """relpose_tsdf_mesh through the C ABI into pre-filled outputs -> the model's output dict.  spare_rows (one scene only): `triangles` gets
    that many rows behind the cap_tri the call is told of."""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, nz, ny, nx = st["tsdf_sum"].shape
    nbytes = L.relpose_tsdf_mesh_workspace_bytes(S, nx, ny, nz)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    assert spare_rows == 0 or S == 1
    out = filled_outputs(S, cap, cap_tri + spare_rows, st["color_sum"] is not None)
    a = _lib.TsdfMeshArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap, a.cap_tri = S, nx, ny, nz, min_weight, cap, cap_tri
    a.tsdf_sum, a.weight, a.color_sum = st["tsdf_sum"].data_ptr(), st["weight"].data_ptr(), (0 if st["color_sum"] is None else st["color_sum"].data_ptr())
    a.origin_host, a.voxel = st["origin"].ctypes.data, st["voxel"]
    for k in ("points", "normals", "valid", "n_points", "triangles", "n_triangles"):
        setattr(a, k, out[k].data_ptr())
    a.colors = 0 if out["colors"] is None else out["colors"].data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_mesh(C.byref(a)) == 0
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def surface_raw(st, min_weight, cap):
    """relpose_tsdf_surface on the same state into the same pre-filled outputs (test_gpu_tsdf.surface_raw's call)"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, nz, ny, nx = st["tsdf_sum"].shape
    nbytes = L.relpose_tsdf_surface_workspace_bytes(S, nx, ny, nz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    out = filled_outputs(S, cap, 1, st["color_sum"] is not None)
    a = _lib.TsdfSurfaceArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap = S, nx, ny, nz, min_weight, cap
    a.tsdf_sum, a.weight, a.color_sum = st["tsdf_sum"].data_ptr(), st["weight"].data_ptr(), (0 if st["color_sum"] is None else st["color_sum"].data_ptr())
    a.origin_host, a.voxel = st["origin"].ctypes.data, st["voxel"]
    a.points, a.normals, a.valid, a.n_points = (out[k].data_ptr() for k in ("points", "normals", "valid", "n_points"))
    a.colors = 0 if out["colors"] is None else out["colors"].data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_surface(C.byref(a)) == 0
    return {k: (None if out[k] is None else out[k].cpu().numpy()) for k in TS.SURF_KEYS}


@pytest.mark.parametrize("name", MS.CASES)
def test_vertices_are_the_surface_and_triangles_the_model_bitwise(name):
    c = MS.case(name)
    cap, cap_tri, want = MS.expected(name)
    st = device_state(c)
    got = mesh_raw(st, c["min_weight"], cap, cap_tri)
    surf = surface_raw(st, c["min_weight"], cap)
    bad_v, bad = TS.differ(got, surf, TS.SURF_KEYS), TS.differ(got, want, MS.MESH_KEYS)
    log("tsdf_mesh_" + name, differ_surface=bad_v, differ_model=bad, n_points=int(got["n_points"].sum()), n_triangles=int(got["n_triangles"].sum()),
        want_triangles=int(want["n_triangles"].sum()))
    assert bad_v == [] and bad == [], (name, bad_v, bad, got["n_triangles"].tolist()[:8], want["n_triangles"].tolist()[:8])
    nt = got["n_triangles"]
    assert all((got["triangles"][s, nt[s]:] == MS.TRI_FILL).all() for s in range(len(nt)))     # rows beyond the count keep their fill
    assert nt.sum() > 0 or name == "flat"
    assert TS.differ(mesh_raw(st, c["min_weight"], cap, cap_tri), got, MS.MESH_KEYS) == []    # a second run


def test_all_cases_batch_equals_its_scenes_one_by_one():
    c = MS.case("all_cases")
    cap, cap_tri, want = MS.expected("all_cases")
    got = mesh_raw(device_state(c), 1, cap, cap_tri)
    assert got["n_triangles"].tolist() == [len(t) for t in MM.TABLE] and got["n_triangles"].sum() == 820
    for s in range(256):
        one = mesh_raw(device_state(c, slice(s, s + 1)), 1, cap, cap_tri)
        assert all(TS.bits_equal(one[k][0], got[k][s]) for k in MS.MESH_KEYS), s
    b = MS.case("empty_in_batch")                                              # and a scene between an empty one and another
    cap, cap_tri, want = MS.expected("empty_in_batch")
    full = mesh_raw(device_state(b), b["min_weight"], cap, cap_tri)
    assert full["n_triangles"][1] == 0 and full["n_points"][1] == 0 and (full["valid"][1] == 0).all() and (full["triangles"][1] == MS.TRI_FILL).all()
    for s in (0, 2):
        one = mesh_raw(device_state(b, slice(s, s + 1)), b["min_weight"], cap, cap_tri)
        assert all(TS.bits_equal(one[k][0], full[k][s]) for k in MS.MESH_KEYS), s


@pytest.mark.parametrize("name", ["noise", "edge_state"])
def test_small_caps_report_the_count_and_write_the_prefix(name):
    c = MS.case(name)
    nv, nt = MS.counts(name)
    st = device_state(c)
    full_cap, full_tri, full = MS.expected(name)
    for cap_tri in (1, int(nt[0]) // 2):                                       # cap_tri below the count: the prefix, the rest keeps its fill
        got = mesh_raw(st, c["min_weight"], full_cap, cap_tri)
        _, _, want = MS.expected(name, full_cap, cap_tri)
        assert TS.differ(got, want, MS.MESH_KEYS) == [], cap_tri
        assert got["n_triangles"][0] == nt[0] > cap_tri and TS.bits_equal(got["triangles"][0], full["triangles"][0, :cap_tri])
        wide = mesh_raw(st, c["min_weight"], full_cap, cap_tri, spare_rows=6)
        assert TS.bits_equal(wide["triangles"][0, :cap_tri], got["triangles"][0]) and (wide["triangles"][0, cap_tri:] == MS.TRI_FILL).all()
    for cap in (1, int(nv[0]) // 3):                                           # cap below the vertex count: the triangles are still the model's
        got = mesh_raw(st, c["min_weight"], cap, full_tri)
        _, _, want = MS.expected(name, cap, full_tri)
        assert TS.differ(got, want, MS.MESH_KEYS) == [], cap
        assert got["n_points"][0] == nv[0] > cap and TS.bits_equal(got["triangles"], full["triangles"]) and got["triangles"].max() >= cap
        assert TS.differ(got, surface_raw(st, c["min_weight"], cap), TS.SURF_KEYS) == []


def test_operator_and_shim_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import ops, util  # noqa: F401
    c = MS.case("empty_in_batch")
    cap, cap_tri, _ = MS.expected("empty_in_batch")
    st = device_state(c)
    mw = c["min_weight"]
    st0 = {k: c[k] for k in TS.STATE_KEYS}
    zero = MM.mesh_outputs(st0, c["origin"], c["voxel"], mw, cap, cap_tri, {"points": 0.0, "normals": 0.0, "colors": 0.0}, 0)    # the shim pre-fills with zeros
    raw = mesh_raw(st, mw, cap, cap_tri)
    shim = util.tsdf_mesh_dev(st, mw, cap, cap_tri)
    assert set(shim) == set(MS.MESH_KEYS)
    op = torch.ops.relpose.tsdf_mesh(st["tsdf_sum"], st["weight"], st["color_sum"], torch.from_numpy(st["origin"]), c["voxel"], mw, cap, cap_tri)
    for got in ({k: v.cpu().numpy() for k, v in shim.items()}, {k: v.cpu().numpy() for k, v in zip(MS.MESH_KEYS, op)}):
        assert TS.differ(got, zero, MS.MESH_KEYS) == []
        assert all(TS.bits_equal(got[k], raw[k]) for k in ("n_points", "n_triangles", "valid"))
    auto = util.tsdf_mesh_dev(st, mw)                                          # None caps: the largest scene's counts
    assert auto["points"].shape[1] == cap - 3 == int(raw["n_points"].max()) and auto["triangles"].shape[1] == cap_tri - 3 == int(raw["n_triangles"].max())
    for k in MS.MESH_KEYS:
        w = zero[k] if k in ("n_points", "n_triangles") else zero[k][:, :(cap_tri if k == "triangles" else cap) - 3]
        assert TS.bits_equal(auto[k].cpu().numpy(), w), k
    surf = util.tsdf_surface_dev(st, mw, cap)
    assert all(torch.equal(a, shim[k]) for a, k in zip(surf, TS.SURF_KEYS))
    no_col = dict(st, color_sum=None)
    assert util.tsdf_mesh_dev(no_col, mw)["colors"] is None
    assert torch.ops.relpose.tsdf_mesh(st["tsdf_sum"], st["weight"], None, torch.from_numpy(st["origin"]), c["voxel"], mw, cap, cap_tri)[2].numel() == 0
    with pytest.raises(ValueError):                                            # a given cap that truncates the vertices
        util.tsdf_mesh_dev(st, mw, int(raw["n_points"].max()) - 1, cap_tri)
    few = util.tsdf_mesh_dev(st, mw, cap, 5)                                   # a small max_triangles only truncates
    assert TS.bits_equal(few["triangles"].cpu().numpy(), zero["triangles"][:, :5]) and TS.bits_equal(few["n_triangles"].cpu().numpy(), zero["n_triangles"])
    m = torch.ops.relpose.tsdf_mesh(st["tsdf_sum"].to("meta"), st["weight"].to("meta"), st["color_sum"].to("meta"), torch.from_numpy(st["origin"]).to("meta"),
                                    c["voxel"], mw, cap, cap_tri)
    for got, ref in zip(m, op):
        assert got.shape == ref.shape and got.dtype == ref.dtype
    flat = util.tsdf_mesh_dev(device_state(MS.case("flat")))                   # a dimension of 1: vertices, no triangle
    assert flat["n_triangles"].tolist() == [0, 0] and flat["triangles"].shape == (2, 1, 3) and flat["n_points"].min() > 0


def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, nx, ny, nz, cap, cap_tri = 2, 3, 2, 2, 8, 8
    host = TS.host_arrays()
    ts = torch.full((S, nz, ny, nx), 5, dtype=torch.int32, device=dev())
    ts[:, :, :, 1] = -5
    wt = torch.ones((S, nz, ny, nx), dtype=torch.int32, device=dev())
    cs = torch.full((S, 3, nz, ny, nx), 100, dtype=torch.int32, device=dev())
    out = filled_outputs(S, cap, cap_tri, True)
    before = {k: v.clone() for k, v in out.items()}
    ws = torch.empty(L.relpose_tsdf_mesh_workspace_bytes(S, nx, ny, nz) + 512, dtype=torch.uint8, device=dev())
    ptrs = {"tsdf_sum": ts.data_ptr(), "weight": wt.data_ptr(), "color_sum": cs.data_ptr()}
    ptrs.update({k: v.data_ptr() for k, v in out.items()})
    for name, kw in MS.mesh_einval_calls():
        a = MS.mesh_args(_lib, 0, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
        a.stream = _lib.stream_ptr()
        assert L.relpose_tsdf_mesh(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], before[k]) for k in out)
    a = MS.mesh_args(_lib, 0, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
    a.stream = _lib.stream_ptr()
    assert L.relpose_tsdf_mesh(C.byref(a)) == 0                                # the base call itself is valid
    assert out["n_points"].tolist() == [8, 8] and out["n_triangles"].tolist() == [4, 4] and (out["valid"] == 1).all()
    assert int(out["triangles"][:, :4].min()) == 0 and int(out["triangles"][:, :4].max()) == 7 and (out["triangles"][:, 4:] == MS.TRI_FILL).all()


def test_rendered_room_fused_meshed_and_written(tmp_path):
    """synth.render_scene(7, 4, "suncg", 16) fused at voxel 0.25 under the ground-truth poses (as test_gpu_sync.py fuses it) and meshed"""
    from relativepose_amd import evaluation as E, util
    sc = synth.render_scene(7, 4, "suncg", 16)
    depth, rgb = up(sc["depth"], np.float32), up(sc["rgb"], np.float32)
    mesh = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True)
    cloud = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25)
    for k in TS.SURF_KEYS:                                                     # mesh=True leaves the cloud what it is
        assert TS.bits_equal(mesh[k].cpu().numpy(), cloud[k].cpu().numpy()), k
    assert "triangles" not in cloud
    n, nt = int(mesh["n_points"][0]), int(mesh["n_triangles"][0])
    tri = mesh["triangles"][0, :nt].cpu().numpy()
    host = {k: mesh["state"][k][0].cpu().numpy() for k in ("tsdf_sum", "weight")}
    assert TS.bits_equal(tri, MM.triangles(host["tsdf_sum"], host["weight"], 1)[0])
    st = E.mesh_stats(mesh)[0]
    log("tsdf_mesh_room", vertices=n, **st)
    assert st["triangles"] == nt > 1000 and st["nonmanifold_edges"] == 0 and st["area"] > 0
    assert MM.edge_report(tri)[0] == 0
    path = tmp_path / "room.mesh.ply"
    assert util.save_ply(str(path), mesh["points"][0, :n], mesh["normals"][0, :n], mesh["colors"][0, :n], tri) == n
    head, payload = path.read_bytes().split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert f"element vertex {n}" in lines and f"element face {nt}" in lines and lines[-2] == "property list uchar int vertex_indices"
    vdt = np.dtype([(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")])
    v = np.frombuffer(payload[:n * vdt.itemsize], vdt)
    f = np.frombuffer(payload[n * vdt.itemsize:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(f) == nt and (f["n"] == 3).all() and np.array_equal(f["v"], tri)
    p = mesh["points"][0, :n].cpu().numpy()
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), p.astype(np.float32))
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), mesh["normals"][0, :n].cpu().numpy().astype(np.float32))
    col = mesh["colors"][0, :n].cpu().numpy()
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), np.rint(np.clip(col.astype(np.float64), 0, 1) * 255).astype(np.uint8))
