"""The pinned inputs of the mesh-decimation tests (CPU and GPU): hand-built meshes with their grids, the meshes of mesh_scenes' volumes and of
components_scenes' two balls on the volume's grid coarsened by 2 and 3, and the invalid calls of relpose_mesh_decimate.  A scene is {"mesh":
components_scenes' mesh dict, "origin" f64 [S,3], "cell", "dims" (gx, gy, gz)}.  Every result is computed once per process and must be left
unchanged."""
import ctypes as C
import functools

import numpy as np

import components_scenes as CS
import decimate_model as DM

HAND = ("shared_edge", "bow_tie", "fan", "one_cell", "faces", "nonfinite", "bad_rows", "sheet", "sheet_once", "no_colors", "batch")
VOLUMES = ("sphere", "noise", "edge_state", "two_balls", "empty_in_batch")
FACTORS = (2, 3)
VOLUME_SCENES = tuple(f"{n}@{f}" for n in VOLUMES for f in FACTORS) + ("truncated@2",)
ALL = HAND + VOLUME_SCENES
ONE_CELL = 1500                                                                # vertices of `one_cell`: all on one accumulator row


def _scene(mesh, origin, cell, dims):
    S = mesh["points"].shape[0]
    return {"mesh": mesh, "origin": np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 3), (S, 3))), "cell": float(cell),
            "dims": tuple(int(d) for d in dims)}


def _shuffle(points, tri, rs):
    """components_scenes' shuffler on the triangles (rows, vertex ids, corners), and the vertex rows moved along with their ids"""
    several = isinstance(points, (list, tuple))
    arrays = list(points) if several else [points]
    n = len(arrays[0])
    twin = np.random.RandomState()
    twin.set_state(rs.get_state())
    perm = twin.permutation(n)                                                 # the shuffler's first draw: old id -> new id
    t = CS._shuffled(tri, n, rs)
    moved = [np.empty_like(p) for p in arrays]
    for src, dst in zip(arrays, moved):
        dst[perm] = src
    return (moved if several else moved[0]), t


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sheet(rs, copies):
    """a jittered 30 x 30 lattice sheet (spacing 0.08, jitter 0.01: no two vertices closer than 0.06 on some axis), its 1682 triangles listed
    `copies` times and, with copies > 1, once more the other way round"""
    n = 30
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p = np.stack([-1.16 + 0.08 * i, -1.16 + 0.08 * j, 0.3 * np.sin(0.2 * i) * np.cos(0.15 * j)], -1).reshape(-1, 3) + rs.uniform(-0.01, 0.01, (n * n, 3))
    v = (j * n + i)[:-1, :-1].reshape(-1)
    tri = np.concatenate([np.stack([v, v + 1, v + n], 1), np.stack([v + 1, v + n + 1, v + n], 1)])
    rows = [tri] * copies + ([tri[:, ::-1]] if copies > 1 else [])
    return p, np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def hand(name):
    rs = np.random.RandomState(sum(name.encode()) + 22)
    org, cell = np.array([-1.0, 0.5, 2.0]), 0.25                               # every multiple of the cell is exact
    inside = lambda c, n: org + cell * (np.asarray(c, np.float64) + rs.uniform(0.05, 0.95, (n, 3)))     # n points inside cell c
    if name == "shared_edge":                                                  # two triangles sharing an edge inside one cell: one vertex, nothing else
        return _scene(CS._pack([(inside((1, 1, 1), 4), np.array([[0, 1, 2], [2, 1, 3]], np.int32), None, None)], rs), org, cell, (3, 3, 3))
    if name == "bow_tie":                                                      # the knot and one wing in one cell, the other wing in the next
        p = np.concatenate([inside((0, 2, 1), 3), inside((1, 2, 1), 2)])
        return _scene(CS._pack([(p, np.array([[0, 1, 2], [2, 3, 4]], np.int32), None, None)], rs), org, cell, (3, 5, 2))
    if name == "fan":                                                          # the hub in one cell, the rim wandering over three others
        rim = [(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (1, 0, 0), (0, 1, 0)] * 6
        p = np.concatenate([inside((0, 0, 0), 1)] + [inside(c, 1) for c in rim])
        k = 1 + np.arange(len(rim))
        tri = np.stack([np.zeros(len(rim), np.int64), k, 1 + k % len(rim)], 1)
        p, tri = _shuffle(p, tri, rs)
        return _scene(CS._pack([(p, tri, None, None)], rs), org, cell, (2, 2, 1))
    if name == "one_cell":                                                     # full contention on one accumulator row
        p = np.array([0.3, -0.2, 0.1]) + 0.7 * rs.uniform(0.0, 1.0, (ONE_CELL, 3))
        return _scene(CS._pack([(p, rs.randint(0, ONE_CELL, (700, 3)).astype(np.int32), None, None)], rs), [0.3, -0.2, 0.1], 0.7, (1, 1, 1))
    if name == "faces":                                                        # vertices exactly on cell faces, on the grid's far faces and one ulp off
        dims = (3, 5, 2)
        ks = [np.arange(-1, d + 2) for d in dims]
        lat = np.stack(np.meshgrid(*ks, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        p = org + cell * lat                                                   # exact: u is the integer, inside iff 0 <= k < g
        far = org + cell * np.asarray(dims, np.float64)
        extra = []
        for a in range(3):
            for base, to in ((far[a], np.inf), (far[a], -np.inf), (org[a], -np.inf), (org[a], np.inf)):
                q = org + cell * 0.5
                q[a] = np.nextafter(base, to)                                  # outside by one ulp / inside by one ulp
                extra.append(q)
        p = np.concatenate([p, np.array(extra)])
        return _scene(CS._pack([(p, rs.randint(0, len(p), (400, 3)).astype(np.int32), None, None)], rs), org, cell, dims)
    if name == "nonfinite":
        n = 600
        m = CS._pack([(org + cell * rs.uniform(-0.3, 4.3, (n, 3)), rs.randint(0, n, (900, 3)).astype(np.int32), None, None)], rs)
        for arr, vals in ((m["points"], (np.nan, np.inf, -np.inf, 1e308, -1e308)), (m["normals"], (np.nan, np.inf, -np.inf, 1e300, 65536.0, -65536.5, 0.0)),
                          (m["colors"], (np.nan, np.inf, -np.inf, -0.25, 1.5, 0.0, 1.0))):
            for v in vals:
                for _ in range(12):
                    arr[0, rs.randint(n), rs.randint(3)] = v
        m["normals"][0, :5] = 0.0                                              # and a cluster whose normals cancel
        m["points"][0, :5] = org + cell * 0.5
        m["points"][0, 5:7] = org + cell * np.array([5.5, 0.5, 0.5])          # a cell of their own
        m["normals"][0, 5], m["normals"][0, 6] = (0.25, -0.5, 0.75), (-0.25, 0.5, -0.75)
        return _scene(m, org, cell, (6, 4, 4))
    if name == "bad_rows":                                                     # index -1, index = nv, index = cap + 5
        nv = 40
        m = CS._pack([(org + cell * rs.uniform(0, 3, (nv, 3)), rs.randint(0, nv, (30, 3)).astype(np.int32), None, None)], rs)
        m["triangles"][0, 4, 1], m["triangles"][0, 11, 0], m["triangles"][0, 23, 2] = -1, nv, m["points"].shape[1] + 5
        return _scene(m, org, cell, (3, 3, 3))
    if name in ("sheet", "sheet_once", "no_colors"):                           # several workgroups; every triangle twice and once flipped
        p, tri = _sheet(rs, 1 if name == "sheet_once" else 2)
        nrm = _unit(rs.normal(size=p.shape))
        (p, nrm), tri = _shuffle([p, nrm], tri, rs)
        m = CS._pack([(p, tri, None, None)], rs, colours=name != "no_colors")
        m["normals"][0, :len(nrm)] = nrm
        return _scene(m, [-1.0, -1.0, -0.5], 0.2, (10, 10, 5))                  # the sheet's rim lies outside the grid
    if name == "batch":                                                        # an empty scene between two; the last says more than fits, twice
        a = (rs.uniform(-1, 1, (300, 3)), rs.randint(0, 300, (260, 3)).astype(np.int32), None, None)
        c = (rs.uniform(-1, 1, (280, 3)), rs.randint(0, 280, (263, 3)).astype(np.int32), 1000, 400)
        m = CS._pack([a, (np.zeros((0, 3)), np.zeros((0, 3), np.int32), None, None), c], rs)
        return _scene(m, rs.uniform(-1.1, -0.9, (3, 3)), 0.45, (5, 4, 5))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def volume(name):
    """`case@factor`: components_scenes.volume_mesh(case) on the volume's own grid coarsened by factor (util.mesh_decimate_volume_dev's grid);
    `truncated@f`: empty_in_batch with cap_tri below the first scene's count"""
    case, factor = name.split("@")
    factor = int(factor)
    src = "empty_in_batch" if case == "truncated" else case
    c = CS.volume_case(src)
    m = dict(CS.volume_mesh(src))
    if case == "truncated":
        m["triangles"] = np.ascontiguousarray(m["triangles"][:, :12])
        assert m["n_triangles"][0] > 12
    _, nz, ny, nx = c["tsdf_sum"].shape
    return _scene(m, c["origin"], factor * c["voxel"], tuple(-(-n // factor) for n in (nx, ny, nz)))


def scene(name):
    return volume(name) if "@" in name else hand(name)


def scene_of(sc, s):
    """scene s of a batch as a scene of its own"""
    return {"mesh": CS.scene_of(sc["mesh"], s), "origin": sc["origin"][s:s + 1], "cell": sc["cell"], "dims": sc["dims"]}


def model(sc, dedupe, fill=DM.FILL, loops=False):
    return (DM.decimate_loops if loops else DM.decimate)(sc["mesh"], sc["origin"], sc["cell"], sc["dims"], dedupe, DM.before(sc["mesh"], fill))


@functools.lru_cache(maxsize=None)
def expected(name, dedupe=1):
    """decimate_model.decimate of a scene into outputs pre-filled with decimate_model.FILL"""
    return model(scene(name), dedupe)


# ---------------------------------------------------------------------------------------------- invalid calls
POINTERS = ("points", "normals", "colors", "n_points", "triangles", "n_triangles", "out_points", "out_normals", "out_colors", "out_valid",
            "out_n_points", "out_count", "out_triangles", "out_n_triangles", "vertex_map", "tri_map") + DM.COUNTERS
OPTIONAL = ("colors", "out_colors", "tri_map")
HOST = {"org": [-1.0, 0.5, 2.0, 0.0, 0.0, 0.0], "org_nan": [-1.0, 0.5, 2.0, 0.0, float("nan"), 0.0], "org_inf": [float("inf"), 0.5, 2.0, 0.0, 0.0, 0.0]}


def einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, cap 8, cap_tri 6, a 3 x 5 x 2 grid of cell 0.5, dedupe 1) that must each
    return RELPOSE_EINVAL; a str value names the pointer to alias, or the host origin to pass"""
    return [("no_" + k, {k: 0}) for k in POINTERS if k not in OPTIONAL] + \
           [("no_origin", {"origin_host": 0}), ("no_workspace", {"workspace": 0}), ("colors_without_out", {"out_colors": 0}),
            ("out_without_colors", {"colors": 0}),
            ("cell_0", {"cell": 0.0}), ("cell_neg", {"cell": -0.5}), ("cell_nan", {"cell": float("nan")}), ("cell_inf", {"cell": float("inf")}),
            ("gx_0", {"gx": 0}), ("gy_neg", {"gy": -1}), ("gz_0", {"gz": 0}), ("gx_1025", {"gx": 1025}), ("gy_1025", {"gy": 1025}), ("gz_1025", {"gz": 1025}),
            ("cells_2_27", {"gx": 1024, "gy": 1024, "gz": 64}), ("cells_2_30", {"gx": 1024, "gy": 1024, "gz": 1024}),
            ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("cap_0", {"cap": 0}), ("cap_neg", {"cap": -5}), ("cap_big", {"cap": 1 << 28}),
            ("cap_tri_0", {"cap_tri": 0}), ("cap_tri_neg", {"cap_tri": -5}), ("cap_tri_big", {"cap_tri": 1 << 28}),
            ("dedupe_2", {"dedupe": 2}), ("dedupe_neg", {"dedupe": -1}), ("origin_nan", {"origin_host": "org_nan"}), ("origin_inf", {"origin_host": "org_inf"}),
            ("points_in_place", {"out_points": "points"}), ("normals_in_place", {"out_normals": "normals"}), ("colors_in_place", {"out_colors": "colors"}),
            ("triangles_in_place", {"out_triangles": "triangles"}), ("n_points_in_place", {"out_n_points": "n_points"}),
            ("n_triangles_in_place", {"out_n_triangles": "n_triangles"}),
            ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


def host_arrays():
    return {k: (C.c_double * len(v))(*v) for k, v in HOST.items()}


def decimate_args(_lib, ptrs, host, kw, ws=256 * 1024, ws_bytes=1 << 40):
    """the valid base call of einval_calls with the changes kw; ptrs: field -> device address, host: host_arrays()"""
    a = _lib.MeshDecimateArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.gx, a.gy, a.gz, a.dedupe, a.cell = 2, 8, 6, 3, 5, 2, 1, 0.5
    for k in POINTERS:
        setattr(a, k, ptrs[k])
    a.origin_host = C.addressof(host["org"])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        elif k == "origin_host" and isinstance(v, str):
            a.origin_host = C.addressof(host[v])
        else:
            setattr(a, k, ptrs[v] if isinstance(v, str) else v)
    return a
