"""The contract of relpose_mesh_decimate (include/relpose.h) in numpy.  Test infrastructure, not product code: the GPU tests
demand that the kernels reproduce every array here bit for bit.  The contract is stated twice: `decimate` works on whole arrays (np.unique,
np.add.at), `decimate_loops` is plain Python over the vertices and the triangles (dicts, Python ints and floats, which are IEEE float64);
tests/test_decimate_cpu.py demands that the two agree bit for bit."""
import math

import numpy as np

from components_model import counts

COUNTERS = ("bad_triangles", "outside_triangles", "degenerate_triangles", "duplicate_triangles")
KEYS = ("points", "normals", "colors", "valid", "n_points", "count", "triangles", "n_triangles", "vertex_map", "tri_map") + COUNTERS
BAD, OUTSIDE, DEGENERATE, DUPLICATE, BEYOND = -1, -2, -3, -4, -5
GRID_MAX = float(2 ** 30)                                                      # what default_grid clamps a dimension to (far outside the limits)
POS_SCALE, NRM_SCALE, COL_SCALE, NRM_MAX = 65536.0, 32768.0, 65535.0, 65536.0
FILL = {"points": -7.5, "normals": 9.25, "colors": -3.0, "valid": 77, "n_points": -7, "count": -11, "triangles": -9, "n_triangles": -7,
        "vertex_map": -5, "tri_map": -6, "bad_triangles": -7, "outside_triangles": -7, "degenerate_triangles": -7, "duplicate_triangles": -7}
DTYPES = {"points": np.float64, "normals": np.float64, "colors": np.float32, "valid": np.uint8, "count": np.int32, "triangles": np.int32,
          "vertex_map": np.int32, "tri_map": np.int32}


def before(mesh, fill=FILL):
    """the pre-filled outputs of a call on `mesh`: every row that the call does not write keeps its fill (fill = 0: what the Python layers
    allocate)"""
    S, cap = mesh["points"].shape[:2]
    cap_tri = mesh["triangles"].shape[1]
    shape = {"points": (S, cap, 3), "normals": (S, cap, 3), "colors": (S, cap, 3), "valid": (S, cap), "count": (S, cap), "triangles": (S, cap_tri, 3),
             "vertex_map": (S, cap), "tri_map": (S, cap_tri)}
    f = (lambda k: 0) if fill == 0 else (lambda k: fill[k])
    out = {k: np.full(shape.get(k, (S,)), f(k), DTYPES.get(k, np.int32)) for k in KEYS}
    if mesh.get("colors") is None:
        out["colors"] = None
    return out


def cells(points, origin, cell, dims):
    """points f64 [n,3] -> (u f64 [n,3], the cell's integer coordinates i64 [n,3] (0 where not inside), inside bool [n])"""
    with np.errstate(all="ignore"):
        u = (np.asarray(points, np.float64) - np.asarray(origin, np.float64)[None]) / np.float64(cell)
        f = np.floor(u)
        inside = (np.isfinite(u) & (f >= 0) & (f < np.asarray(dims, np.float64)[None])).all(1)
    return u, np.where(inside[:, None], f, 0.0).astype(np.int64), inside


def quantised(u, normals, colors):
    """the ten integers of every vertex, i64 [n,10]: 3 position, 3 normal, 3 colour (0 without colours), 1"""
    n = len(u)
    v = np.zeros((n, 10), np.int64)
    with np.errstate(all="ignore"):
        v[:, 0:3] = np.rint(u * POS_SCALE).astype(np.int64)
        nn = np.asarray(normals, np.float64)
        ok = np.isfinite(nn) & (np.abs(nn) <= NRM_MAX)
        v[:, 3:6] = np.rint(np.where(ok, nn, 0.0) * NRM_SCALE).astype(np.int64)
        if colors is not None:
            c = np.asarray(colors, np.float32).astype(np.float64)
            c = np.where(np.isnan(c), 0.0, np.minimum(np.maximum(c, 0.0), 1.0))
            v[:, 6:9] = np.rint(c * COL_SCALE).astype(np.int64)
    v[:, 9] = 1
    return v


def cluster_outputs(acc, origin, cell, colours):
    """acc i64 [n,10] -> (points f64 [n,3], normals f64 [n,3], colors f32 [n,3] or None, count i32 [n])"""
    n = acc[:, 9].astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        pts = np.asarray(origin, np.float64)[None] + (acc[:, 0:3].astype(np.float64) / (POS_SCALE * n)) * np.float64(cell)
        s = acc[:, 3:6].astype(np.float64)
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None]
        nrm = np.where(ln == 0.0, 0.0, s / np.where(ln == 0.0, 1.0, ln))
        col = (acc[:, 6:9].astype(np.float64) / (COL_SCALE * n)).astype(np.float32) if colours else None
    return pts, nrm, col, acc[:, 9].astype(np.int32)


def _scene_arrays(points, normals, colors, tri, nv, cap, origin, cell, dims, dedupe):
    u, f, inside = cells(points[:nv], origin, cell, dims)
    idx = np.nonzero(inside)[0]
    lin = (f[idx, 2] * dims[1] + f[idx, 1]) * dims[0] + f[idx, 0]
    _, first, inv = np.unique(lin, return_index=True, return_inverse=True)      # first: the first, so the smallest, member of each cell
    inv = inv.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))              # clusters in ascending order of their representative
    vmap = np.full(cap, -1, np.int32)
    vmap[idx] = rank[inv]
    acc = np.zeros((len(first), 10), np.int64)
    np.add.at(acc, rank[inv], quantised(u[idx], normals[:nv][idx], None if colors is None else colors[:nv][idx]))    # integer sums: any order
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    good = ((t >= 0) & (t < nv)).all(1)
    m = vmap[np.clip(t, 0, cap - 1)].astype(np.int64)
    out = good & (m < 0).any(1)
    deg = good & ~out & ((m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2]))
    cand = good & ~out & ~deg
    tmap = np.full(len(t), 0, np.int32)
    tmap[~good], tmap[out], tmap[deg] = BAD, OUTSIDE, DEGENERATE
    rows = np.nonzero(cand)[0]
    if dedupe and len(rows):
        k = np.argmin(m[rows], 1)
        rot = np.stack([m[rows, (k + j) % 3] for j in range(3)], 1)            # the smallest index first, the orientation kept
        _, keep = np.unique(rot, axis=0, return_index=True)                      # the first, so the lowest, row of each set
        lost = np.ones(len(rows), bool)
        lost[keep] = False
        tmap[rows[lost]] = DUPLICATE
        rows = rows[~lost]
    tmap[rows] = np.arange(len(rows))
    return vmap, acc, tmap, m[rows].astype(np.int32), (int((~good).sum()), int(out.sum()), int(deg.sum()), int((tmap == DUPLICATE).sum()))


def _scene_loops(points, normals, colors, tri, nv, cap, origin, cell, dims, dedupe):
    cell = float(cell)
    org = [float(x) for x in origin]
    cell_of, members = {}, {}                                                   # vertex -> cell; cell -> its vertices in ascending order
    us = {}
    for v in range(nv):
        u = [(float(points[v, a]) - org[a]) / cell for a in range(3)]
        if not all(math.isfinite(x) and 0 <= math.floor(x) < dims[a] for a, x in enumerate(u)):
            continue
        c = tuple(math.floor(x) for x in u)
        cell_of[v], us[v] = c, u
        members.setdefault(c, []).append(v)
    reps = sorted(vs[0] for vs in members.values())
    number = {cell_of[r]: k for k, r in enumerate(reps)}
    vmap = np.full(cap, -1, np.int32)
    acc = np.zeros((len(reps), 10), np.int64)
    for v, c in cell_of.items():
        k = number[c]
        vmap[v] = k
        row = [0] * 10
        for a in range(3):
            row[a] = round(us[v][a] * POS_SCALE)                                 # Python's round: to nearest, ties to even, exact integers
            n = float(normals[v, a])
            row[3 + a] = round(n * NRM_SCALE) if math.isfinite(n) and abs(n) <= NRM_MAX else 0
            if colors is not None:
                x = float(colors[v, a])
                row[6 + a] = 0 if math.isnan(x) else round(min(max(x, 0.0), 1.0) * COL_SCALE)
        row[9] = 1
        for j in range(10):
            acc[k, j] += row[j]
    tmap = np.zeros(len(tri), np.int32)
    rows, seen = [], set()
    n_bad = n_out = n_deg = n_dup = 0
    for r in range(len(tri)):
        i = [int(x) for x in tri[r]]
        if not all(0 <= x < nv for x in i):
            tmap[r], n_bad = BAD, n_bad + 1
            continue
        m = [int(vmap[x]) for x in i]
        if min(m) < 0:
            tmap[r], n_out = OUTSIDE, n_out + 1
            continue
        if m[0] == m[1] or m[1] == m[2] or m[0] == m[2]:
            tmap[r], n_deg = DEGENERATE, n_deg + 1
            continue
        k = m.index(min(m))
        key = (m[k], m[(k + 1) % 3], m[(k + 2) % 3])
        if dedupe and key in seen:
            tmap[r], n_dup = DUPLICATE, n_dup + 1
            continue
        seen.add(key)
        tmap[r] = len(rows)
        rows.append(m)
    return vmap, acc, tmap, np.array(rows, np.int32).reshape(-1, 3), (n_bad, n_out, n_deg, n_dup)


def _cluster_outputs_loops(acc, origin, cell, colours):
    n = len(acc)
    pts, nrm, col = np.zeros((n, 3)), np.zeros((n, 3)), (np.zeros((n, 3), np.float32) if colours else None)
    for k in range(n):
        cnt = float(int(acc[k, 9]))
        s = [float(int(acc[k, 3 + a])) for a in range(3)]
        ln = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        for a in range(3):
            pts[k, a] = float(origin[a]) + (float(int(acc[k, a])) / (POS_SCALE * cnt)) * float(cell)
            nrm[k, a] = 0.0 if ln == 0.0 else s[a] / ln
            if colours:
                col[k, a] = np.float32(float(int(acc[k, 6 + a])) / (COL_SCALE * cnt))
    return pts, nrm, col, acc[:, 9].astype(np.int32)


def _decimate(mesh, origin, cell, dims, dedupe, prefilled, scene, outputs):
    out = {k: (None if v is None else v.copy()) for k, v in prefilled.items()}
    S, cap = mesh["points"].shape[:2]
    cap_tri = mesh["triangles"].shape[1]
    dims = tuple(int(d) for d in dims)
    origin = np.asarray(origin, np.float64).reshape(S, 3)
    for s in range(S):
        nv, nt = counts(mesh["n_points"][s], mesh["n_triangles"][s], cap, cap_tri)
        col = None if mesh.get("colors") is None else mesh["colors"][s]
        vmap, acc, tmap, tri, cnt = scene(mesh["points"][s], mesh["normals"][s], col, mesh["triangles"][s, :nt], nv, cap, origin[s], cell, dims, bool(dedupe))
        n = len(acc)
        pts, nrm, colours, count = outputs(acc, origin[s], cell, col is not None)
        out["points"][s, :n], out["normals"][s, :n], out["count"][s, :n] = pts, nrm, count
        if col is not None:
            out["colors"][s, :n] = colours
        out["valid"][s] = np.arange(cap) < n
        out["n_points"][s], out["n_triangles"][s] = n, len(tri)
        out["triangles"][s, :len(tri)] = tri
        out["vertex_map"][s] = vmap
        out["tri_map"][s, :nt], out["tri_map"][s, nt:] = tmap, BEYOND
        for k, c in zip(COUNTERS, cnt):
            out[k][s] = c
    return out


def decimate(mesh, origin, cell, dims, dedupe, prefilled):
    """What relpose_mesh_decimate leaves in the pre-filled outputs `prefilled` (a dict of KEYS arrays, "colors" None without colours; see
    `before`), on whole arrays.  mesh: {"points", "normals" f64 [S,cap,3], "colors" f32 [S,cap,3] or None, "n_points" [S], "triangles" i32
    [S,cap_tri,3], "n_triangles" [S]}; origin f64 [S,3]; dims (gx, gy, gz)."""
    return _decimate(mesh, origin, cell, dims, dedupe, prefilled, _scene_arrays, cluster_outputs)


def decimate_loops(mesh, origin, cell, dims, dedupe, prefilled):
    """the same as plain loops over the vertices, the clusters and the triangles"""
    return _decimate(mesh, origin, cell, dims, dedupe, prefilled, _scene_loops, _cluster_outputs_loops)


def default_grid(mesh, cell):
    """util.mesh_decimate_grid in numpy: -> (origin f64 [S,3], dims)"""
    S, cap = mesh["points"].shape[:2]
    origin, top = np.zeros((S, 3)), np.zeros((S, 3))
    for s in range(S):
        nv = min(max(int(mesh["n_points"][s]), 0), cap)
        p = mesh["points"][s, :nv]
        p = p[np.isfinite(p).all(1)]
        if len(p):
            origin[s], top[s] = p.min(0), p.max(0)
    with np.errstate(all="ignore"):
        return origin, tuple(int(v) for v in np.minimum(np.floor((top - origin) / np.float64(cell)).max(0) + 1, GRID_MAX))
