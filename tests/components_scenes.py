"""The pinned inputs of the mesh-component tests (CPU and GPU): hand-built meshes, the meshes of mesh_scenes' volumes, a `two_balls` volume,
and the invalid calls of relpose_mesh_components / relpose_mesh_filter.  A mesh is {"points", "normals" f64 [S,cap,3], "colors" f32 [S,cap,3]
or None, "n_points" i32 [S], "triangles" i32 [S,cap_tri,3], "n_triangles" i32 [S], "area_scale"}.  Every result is computed once per process
and must be left unchanged."""
import ctypes as C
import functools

import numpy as np

import components_model as CM
import mesh_scenes as MS

HAND = ("two_triangles", "bow_tie", "strip", "comb", "random", "bad_rows", "batch")
VOLUMES = ("noise", "edge_state", "empty_in_batch", "sphere", "two_balls")
STRIP = 1500                                                                   # triangles of the strip: its diameter


def _pack(scenes, rs, area_scale=1024.0, spare=3, colours=True):
    """scenes: a list of (points f64 [n,3], tri [m,3], n_points or None, n_triangles or None) -> the batch, capacities = the largest + spare"""
    S = len(scenes)
    cap = max(len(p) for p, _, _, _ in scenes) + spare
    cap_tri = max(len(t) for _, t, _, _ in scenes) + spare
    m = {"points": rs.uniform(-2, 2, (S, cap, 3)), "normals": rs.uniform(-1, 1, (S, cap, 3)),
         "colors": rs.uniform(0, 1, (S, cap, 3)).astype(np.float32) if colours else None, "n_points": np.zeros(S, np.int32),
         "triangles": rs.randint(-3, cap + 3, (S, cap_tri, 3)).astype(np.int32), "n_triangles": np.zeros(S, np.int32), "area_scale": area_scale}
    for s, (p, t, nv, nt) in enumerate(scenes):
        m["points"][s, :len(p)] = p
        m["triangles"][s, :len(t)] = t
        m["n_points"][s] = len(p) if nv is None else nv
        m["n_triangles"][s] = len(t) if nt is None else nt
    return m


def _shuffled(tri, n, rs, low=None):
    """the triangle rows and the vertex ids of tri (on n vertices) shuffled; `low`: the old vertex that gets the new index 0"""
    perm = rs.permutation(n)
    if low is not None:
        j = int(np.nonzero(perm == 0)[0][0])
        perm[j], perm[low] = perm[low], 0
    t = perm[np.asarray(tri, np.int64)]
    t = t[rs.permutation(len(t))]
    for r in range(len(t)):                                                    # and the corners within a row
        t[r] = t[r][rs.permutation(3)]
    return t.astype(np.int32)


def _strip(first, n):
    """n triangles in a chain, neighbours sharing ONE vertex: triangle i = (first + 2i, first + 2i + 1, first + 2i + 2)"""
    i = first + 2 * np.arange(n)
    return np.stack([i, i + 1, i + 2], 1)


@functools.lru_cache(maxsize=None)
def hand(name):
    rs = np.random.RandomState(sum(name.encode()))
    pts = lambda n: rs.uniform(-1, 1, (n, 3))
    if name == "two_triangles":
        return _pack([(pts(6), _shuffled([[0, 1, 2], [3, 4, 5]], 6, rs), None, None)], rs)
    if name == "bow_tie":                                                      # one shared vertex: one component
        return _pack([(pts(5), _shuffled([[0, 1, 2], [2, 3, 4]], 5, rs), None, None)], rs)
    if name == "strip":                                                        # diameter STRIP, several workgroups, the smallest index in the middle
        n = 2 * STRIP + 1
        return _pack([(pts(n), _shuffled(_strip(0, STRIP), n, rs, low=STRIP), None, None)], rs)
    if name == "comb":                                                         # 40 strips of 25 triangles joined only at their last triangle
        k, m = 40, 25
        per = 2 * m + 1
        tri = np.concatenate([_strip(q * per, m) for q in range(k)])
        hub = k * per                                                          # every strip's last triangle gets the hub as its third corner
        tri[m - 1::m, 2] = hub
        return _pack([(pts(hub + 1), _shuffled(tri, hub + 1, rs), None, None)], rs)
    if name == "random":                                                       # many components, many unused vertices, repeated corners
        return _pack([(pts(2000), rs.randint(0, 2000, (1500, 3)).astype(np.int32), None, None)], rs)
    if name == "bad_rows":                                                     # index -1, index = nv, index = cap + 5; a huge and a non-finite area
        nv = 40
        tri = rs.randint(0, nv, (30, 3)).astype(np.int32)
        m = _pack([(pts(nv), tri, None, None)], rs)
        cap = m["points"].shape[1]
        m["triangles"][0, 4, 1], m["triangles"][0, 11, 0], m["triangles"][0, 23, 2] = -1, nv, cap + 5
        m["points"][0, tri[0, 0]] = 1.0e9                                      # above the clamp
        m["points"][0, tri[1, 1]] = np.nan
        m["points"][0, tri[2, 2], 1] = np.inf
        return m
    if name == "batch":                                                        # an empty scene between two; the last says more triangles than fit
        a = (pts(300), rs.randint(0, 300, (260, 3)).astype(np.int32), None, None)
        c = (pts(280), rs.randint(0, 280, (263, 3)).astype(np.int32), None, 400)    # cap_tri = 263 + 3 < 400: the spare rows are random and read
        return _pack([a, (np.zeros((0, 3)), np.zeros((0, 3), np.int32), None, None), c], rs)
    raise KeyError(name)


def scene_of(m, s):
    """scene s of a batch as a mesh of its own"""
    return {k: (v[s:s + 1] if isinstance(v, np.ndarray) else v) for k, v in m.items()}


@functools.lru_cache(maxsize=None)
def volume_case(name):
    """a mesh_scenes case, or two_balls: a 16 x 16 x 28 volume, all known, with two disjoint balls of radius 4.5 and 3 voxels"""
    if name != "two_balls":
        return MS.case(name)
    nx, ny, nz = 16, 16, 28
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.minimum(np.sqrt((i - 7.6) ** 2 + (j - 7.4) ** 2 + (k - 7.3) ** 2) - 4.5, np.sqrt((i - 7.5) ** 2 + (j - 7.7) ** 2 + (k - 20.4) ** 2) - 3.0)
    wt = np.full((1, nz, ny, nx), 2, np.int32)
    ts = (np.rint(np.clip(d / 2.0, -1, 1) * 32768) * 2).astype(np.int32)[None]
    return {"tsdf_sum": ts, "weight": wt, "color_sum": None, "origin": np.array([[-1.0, -1.0, -1.75]]), "voxel": 0.125, "min_weight": 1}


@functools.lru_cache(maxsize=None)
def volume_mesh(name):
    """the model's mesh of a volume case (mesh_model.mesh_outputs with zero fill and exact capacities + 3)"""
    c = volume_case(name)
    S = c["tsdf_sum"].shape[0]
    nv = [int(MS.MM.TM.surface(c["tsdf_sum"][s], c["weight"][s], None, c["origin"][s], c["voxel"], c["min_weight"])["n"]) for s in range(S)]
    nt = [len(MS.MM.triangles(c["tsdf_sum"][s], c["weight"][s], c["min_weight"])[0]) for s in range(S)]
    st = {k: c[k] for k in MS.TS.STATE_KEYS}
    m = MS.MM.mesh_outputs(st, c["origin"], c["voxel"], c["min_weight"], max(nv) + 3, max(nt) + 3, {"points": 0.0, "normals": 0.0, "colors": 0.0}, 0)
    m["area_scale"] = float(2 ** 20) / c["voxel"] ** 2
    return m


@functools.lru_cache(maxsize=None)
def expected(kind, name, cap_comp=None):
    """(cap_comp, components_model.components) of a hand-built mesh or a volume's model mesh; None = the largest scene's count + 2"""
    m = hand(name) if kind == "hand" else volume_mesh(name)
    if cap_comp is None:
        cap_comp = int(CM.components(m, 0, m["area_scale"])["n_components"].max()) + 2
    return cap_comp, CM.components(m, cap_comp, m["area_scale"])


# ---------------------------------------------------------------------------------------------- invalid calls
COMPONENT_POINTERS = ("triangles", "n_triangles", "n_points", "points", "vertex_label", "tri_label", "n_components", "bad_triangles", "comp_root",
                      "comp_vertices", "comp_triangles", "comp_area")
FILTER_POINTERS = ("points", "normals", "colors", "n_points", "triangles", "n_triangles", "vertex_label", "tri_label", "keep", "out_points",
                   "out_normals", "out_colors", "out_valid", "out_n_points", "out_triangles", "out_n_triangles", "vertex_map")


def components_einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, cap 8, cap_tri 6, cap_comp 4, max_rounds 16, area_scale 1024) that must
    each return RELPOSE_EINVAL"""
    return [("no_triangles", {"triangles": 0}), ("no_n_triangles", {"n_triangles": 0}), ("no_n_points", {"n_points": 0}),
            ("no_vertex_label", {"vertex_label": 0}), ("no_tri_label", {"tri_label": 0}), ("no_n_components", {"n_components": 0}),
            ("no_bad_triangles", {"bad_triangles": 0}), ("no_workspace", {"workspace": 0}),
            ("no_comp_root", {"comp_root": 0}), ("no_comp_vertices", {"comp_vertices": 0}), ("no_comp_triangles", {"comp_triangles": 0}),
            ("no_comp_area", {"comp_area": 0}),
            ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("cap_0", {"cap": 0}), ("cap_neg", {"cap": -5}), ("cap_big", {"cap": 1 << 28}),
            ("cap_tri_0", {"cap_tri": 0}), ("cap_tri_neg", {"cap_tri": -5}), ("cap_tri_big", {"cap_tri": 1 << 28}),
            ("cap_comp_neg", {"cap_comp": -1}), ("cap_comp_big", {"cap_comp": 1 << 28}),
            ("scale_0", {"area_scale": 0.0}), ("scale_neg", {"area_scale": -1.0}), ("scale_nan", {"area_scale": float("nan")}),
            ("scale_inf", {"area_scale": float("inf")}), ("rounds_0", {"max_rounds": 0}), ("rounds_neg", {"max_rounds": -3}),
            ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


def filter_einval_calls():
    """the same for relpose_mesh_filter (2 scenes, cap 8, cap_tri 6, cap_comp 4, drop_unused 1)"""
    return [("no_" + k, {k: 0}) for k in FILTER_POINTERS if k not in ("colors", "out_colors", "vertex_map")] + \
           [("colors_without_out", {"out_colors": 0}), ("out_without_colors", {"colors": 0}),
            ("scenes_0", {"n_scenes": 0}), ("cap_0", {"cap": 0}), ("cap_big", {"cap": 1 << 28}), ("cap_tri_0", {"cap_tri": 0}),
            ("cap_tri_big", {"cap_tri": 1 << 28}), ("cap_comp_neg", {"cap_comp": -1}), ("cap_comp_big", {"cap_comp": 1 << 28}),
            ("drop_2", {"drop_unused": 2}), ("drop_neg", {"drop_unused": -1}),
            ("points_in_place", {"out_points": "points"}), ("normals_in_place", {"out_normals": "normals"}), ("colors_in_place", {"out_colors": "colors"}),
            ("triangles_in_place", {"out_triangles": "triangles"}), ("n_points_in_place", {"out_n_points": "n_points"}),
            ("n_triangles_in_place", {"out_n_triangles": "n_triangles"}), ("map_is_label", {"vertex_map": "vertex_label"}),
            ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


def _args(a, pointers, ptrs, kw, ws, ws_bytes):
    for k in pointers:
        setattr(a, k, ptrs[k])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        else:
            setattr(a, k, ptrs[v] if isinstance(v, str) else v)                # a str names the pointer to alias
    return a


def components_args(_lib, ptrs, kw, ws=256 * 1024, ws_bytes=1 << 40, rounds_host=0):
    """the valid base call of components_einval_calls with the changes kw; ptrs: field -> address"""
    a = _lib.MeshComponentsArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.max_rounds, a.area_scale = 2, 8, 6, 4, 16, 1024.0
    a.rounds_host = rounds_host
    return _args(a, COMPONENT_POINTERS, ptrs, kw, ws, ws_bytes)


def filter_args(_lib, ptrs, kw, ws=256 * 1024, ws_bytes=1 << 40):
    a = _lib.MeshFilterArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.drop_unused = 2, 8, 6, 4, 1
    return _args(a, FILTER_POINTERS, ptrs, kw, ws, ws_bytes)
