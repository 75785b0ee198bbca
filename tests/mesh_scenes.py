"""The pinned inputs of the mesh tests (CPU and GPU): hand-built states for relpose_tsdf_mesh, next to tsdf_scenes' rooms.  A case is
{"tsdf_sum" i32 [S,nz,ny,nx], "weight" i32, "color_sum" u32 [S,3,nz,ny,nx] or None, "origin" f64 [S,3], "voxel", "min_weight"}.  Every model
result is computed once per process and must be left unchanged."""
import ctypes as C
import functools

import numpy as np

import mesh_model as MM
import tsdf_scenes as TS

TRI_FILL = -9                                                                  # what `triangles` is pre-filled with
MESH_KEYS = TS.SURF_KEYS + ("triangles", "n_triangles")
CASES = ("all_cases", "noise", "sphere", "flat", "empty_in_batch", "edge_state") + tuple(f"room_{ds}_{h}" for ds, h in TS.ROOM_KEYS)


def _colours(rs, weight):
    """a colour sum per voxel that stays below 255 weight"""
    return (rs.randint(0, 256, (weight.shape[0], 3) + weight.shape[1:]) * weight[:, None]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    rs = np.random.RandomState(sum(name.encode()))
    if name == "all_cases":
        # 256 scenes of 2 x 2 x 2 voxels: scene s realises case s with weight 1 and tsdf_sum = +-(1 + corner) 1000
        mag = ((1 + np.arange(8)) * 1000).reshape(1, 2, 2, 2)
        neg = (np.arange(256)[:, None] >> np.arange(8)[None] & 1).reshape(256, 2, 2, 2).astype(bool)       # corner c = x + 2 y + 4 z: [z, y, x]
        ts = np.where(neg, -mag, mag).astype(np.int32)
        wt = np.ones_like(ts)
        origin = rs.uniform(-1, 1, (256, 3))
        return {"tsdf_sum": ts, "weight": wt, "color_sum": _colours(rs, wt), "origin": origin, "voxel": 0.25, "min_weight": 1}
    if name == "noise":
        # 13 x 11 x 9 (no multiple of any tile): random signs and magnitudes, about 5 % unknown, a few exact zeros
        shape = (1, 9, 11, 13)
        wt = rs.randint(1, 5, shape).astype(np.int32)
        ts = (rs.randint(-32768, 32769, shape) * wt).astype(np.int32)
        wt[rs.uniform(size=shape) < 0.05] = 0
        ts[rs.uniform(size=shape) < 0.02] = 0
        return {"tsdf_sum": ts, "weight": wt, "color_sum": _colours(rs, wt), "origin": np.array([[0.3, -1.7, 2.9]]), "voxel": 0.3, "min_weight": 1}
    if name == "sphere":
        # a signed distance in 24^3, all known: t > 0 outside the ball (the space that was seen through), truncated at 4 voxels
        n = 24
        k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        d = np.sqrt((i - 11.3) ** 2 + (j - 11.6) ** 2 + (k - 12.1) ** 2) - 8.4
        wt = np.full((1, n, n, n), 2, np.int32)
        ts = (np.rint(np.clip(d / 4.0, -1, 1) * 32768) * 2).astype(np.int32)[None]
        return {"tsdf_sum": ts, "weight": wt, "color_sum": None, "origin": np.array([[-1.5, -1.5, -1.5]]), "voxel": 0.125, "min_weight": 1}
    if name == "flat":
        # a dimension of 1: crossings, but no cell
        shape = (2, 1, 7, 6)
        wt = np.ones(shape, np.int32)
        ts = rs.randint(-32768, 32769, shape).astype(np.int32)
        return {"tsdf_sum": ts, "weight": wt, "color_sum": _colours(rs, wt), "origin": np.zeros((2, 3)), "voxel": 0.5, "min_weight": 1}
    if name == "empty_in_batch":
        # three scenes, the middle one without a known voxel; the last under min_weight = 2 in places
        shape = (3, 5, 6, 7)
        wt = rs.randint(1, 4, shape).astype(np.int32)
        ts = (rs.randint(-32768, 32769, shape) * wt).astype(np.int32)
        wt[1] = 0
        return {"tsdf_sum": ts, "weight": wt, "color_sum": _colours(rs, wt), "origin": rs.uniform(-1, 1, (3, 3)), "voxel": 0.2, "min_weight": 2}
    if name == "edge_state":
        e = TS.edge_state()
        return {k: e[k] for k in ("tsdf_sum", "weight", "color_sum", "origin", "voxel", "min_weight")}
    if name.startswith("room_"):
        ds, h = name[5:].rsplit("_", 1)
        c, st = TS.room(ds, int(h)), TS.room_state(ds, int(h))
        return {"tsdf_sum": st["tsdf_sum"], "weight": st["weight"], "color_sum": st["color_sum"], "origin": c["origin"], "voxel": c["voxel"], "min_weight": 1}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def counts(name):
    """-> (n_points [S], n_triangles [S]) of the model"""
    c = case(name)
    S = c["tsdf_sum"].shape[0]
    nv = [int(((MM.TM.surface(c["tsdf_sum"][s], c["weight"][s], None, c["origin"][s], c["voxel"], c["min_weight"]))["n"])) for s in range(S)]
    nt = [len(MM.triangles(c["tsdf_sum"][s], c["weight"][s], c["min_weight"])[0]) for s in range(S)]
    return np.array(nv), np.array(nt)


@functools.lru_cache(maxsize=None)
def expected(name, cap=None, cap_tri=None):
    """mesh_model.mesh_outputs of a case; a None cap is the largest scene's count + 3, so rows beyond the count keep their fill"""
    c = case(name)
    nv, nt = counts(name)
    cap = int(nv.max()) + 3 if cap is None else cap
    cap_tri = int(nt.max()) + 3 if cap_tri is None else cap_tri
    st = {k: c[k] for k in TS.STATE_KEYS}
    return cap, cap_tri, MM.mesh_outputs(st, c["origin"], c["voxel"], c["min_weight"], cap, cap_tri, TS.FILL, TRI_FILL)


# ---------------------------------------------------------------------------------------------- invalid calls
def mesh_einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, a 3 x 2 x 2 volume, cap 8, cap_tri 8, min_weight 1) that must each
    return RELPOSE_EINVAL; values as tsdf_scenes.surface_einval_calls'."""
    return [("no_tsdf", {"tsdf_sum": 0}), ("no_weight", {"weight": 0}), ("no_origin", {"origin_host": 0}), ("no_points", {"points": 0}),
            ("no_normals", {"normals": 0}), ("no_valid", {"valid": 0}), ("no_n_points", {"n_points": 0}), ("no_triangles", {"triangles": 0}),
            ("no_n_triangles", {"n_triangles": 0}), ("no_workspace", {"workspace": 0}),
            ("colors_without_color_sum", {"color_sum": 0}), ("min_weight_0", {"min_weight": 0}), ("min_weight_neg", {"min_weight": -1}),
            ("cap_0", {"cap": 0}), ("cap_neg", {"cap": -5}), ("cap_big", {"cap": 1 << 28}),
            ("cap_tri_0", {"cap_tri": 0}), ("cap_tri_neg", {"cap_tri": -5}), ("cap_tri_big", {"cap_tri": 1 << 28}),
            ("voxel_0", {"voxel": 0.0}), ("voxel_neg", {"voxel": -0.1}), ("voxel_nan", {"voxel": float("nan")}), ("voxel_inf", {"voxel": float("inf")}),
            ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("nx_0", {"nx": 0}), ("ny_neg", {"ny": -1}), ("nz_0", {"nz": 0}),
            ("voxels_2_31", {"nx": 2048, "ny": 1024, "nz": 1024}), ("crossings_2_31", {"nx": 1024, "ny": 1024, "nz": 700, "n_scenes": 1}),
            ("triangles_2_31", {"nx": 1024, "ny": 1024, "nz": 512, "n_scenes": 1}),
            ("origin_nan", {"origin_host": "org_nan"}), ("origin_inf", {"origin_host": "org_inf"}), ("workspace_small", {"workspace_bytes": 255}),
            ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


MESH_POINTERS = ("tsdf_sum", "weight", "color_sum", "points", "normals", "colors", "valid", "n_points", "triangles", "n_triangles")


def mesh_args(_lib, p, host, kw, ws=256 * 1024, ws_bytes=1 << 40, ptrs=None):
    """the valid base call of mesh_einval_calls with the changes kw; p: the address every device pointer gets (ptrs overrides)"""
    a = _lib.TsdfMeshArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap, a.cap_tri = 2, 3, 2, 2, 1, 8, 8
    a.voxel = 0.5
    for k in MESH_POINTERS:
        setattr(a, k, p if ptrs is None else ptrs[k])
    a.origin_host = C.addressof(host["org"])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        else:
            setattr(a, k, C.addressof(host[v]) if isinstance(v, str) else v)
    return a
