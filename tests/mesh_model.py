"""The contract of relpose_tsdf_mesh (include/relpose.h) in numpy: the vertices are tsdf_model.surface's crossings, the
triangles come from the generated case table (tools/gen_mc_table.py).  Test infrastructure, not product code: the GPU tests demand that the
kernels reproduce every array here bit for bit.  The rule is stated twice, on whole arrays (what the tests compare the GPU with) and as
plain loops (the check of the array form)."""
import os
import sys

import numpy as np

import tsdf_model as TM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table as GEN  # noqa: E402

TABLE = GEN.table()                                                            # [256] lists of (e0, e1, e2)
COUNT = np.array([len(t) for t in TABLE], np.int64)
EDGES = np.full((256, GEN.MAX_TRIANGLES, 3), -1, np.int64)                     # the table as an array, -1 beyond a case's count
for _c, _t in enumerate(TABLE):
    if _t:
        EDGES[_c, :len(_t)] = _t
EDGE_AXIS = np.array([e // 4 for e in range(12)], np.int64)
EDGE_OFFSET = np.array([GEN.edge_ends(e)[0] for e in range(12)], np.int64)     # the owning corner's (x, y, z) offset


def triangles(tsdf_sum, weight, min_weight=1):
    """One scene -> (tri i32 [n,3]: indices into tsdf_model.surface's rows, cell i64 [n]: each triangle's linear voxel index of its cell's
    lowest corner).  Cells in ascending linear index with x fastest, within a cell the table's order."""
    nz, ny, nx = tsdf_sum.shape
    known, t = TM.values(tsdf_sum, weight, min_weight)
    edge = TM.surface(tsdf_sum, weight, None, np.zeros(3), 1.0, min_weight)["edge"]
    vid = np.full(3 * nx * ny * nz, -1, np.int64)                              # (voxel, axis) -> vertex index
    vid[edge[:, 0] * 3 + edge[:, 1]] = np.arange(len(edge))
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    neg = t < 0
    full = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, c >> 1 & 1, c >> 2 & 1
        sl = (slice(oz, oz + nz - 1), slice(oy, oy + ny - 1), slice(ox, ox + nx - 1))
        full &= known[sl]
        case |= neg[sl].astype(np.int64) << c
    k, j, i = np.nonzero(full & (COUNT[case] > 0))                             # row-major: ascending cell index, x fastest
    ed = EDGES[case[k, j, i]]                                                  # [m, 5, 3]
    keep = ed[..., 0] >= 0
    e = np.where(ed >= 0, ed, 0)
    lin = ((k[:, None, None] + EDGE_OFFSET[e, 2]) * ny + (j[:, None, None] + EDGE_OFFSET[e, 1])) * nx + (i[:, None, None] + EDGE_OFFSET[e, 0])
    tri = vid[lin * 3 + EDGE_AXIS[e]][keep]
    assert (tri >= 0).all()
    cell = np.broadcast_to((((k * ny) + j) * nx + i)[:, None], keep.shape)[keep]
    return tri.astype(np.int32).reshape(-1, 3), cell.astype(np.int64)


def triangles_loops(tsdf_sum, weight, min_weight=1):
    """triangles() as plain loops (its check; small volumes only)"""
    nz, ny, nx = tsdf_sum.shape
    kn = lambda i, j, k: int(weight[k, j, i]) >= min_weight
    ng = lambda i, j, k: int(tsdf_sum[k, j, i]) < 0                           # t < 0 iff tsdf_sum < 0: the weight of a known voxel is >= 1
    first, mask, n = {}, {}, 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                m = 0
                if kn(i, j, k):
                    for a, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                        if i + di < nx and j + dj < ny and k + dk < nz and kn(i + di, j + dj, k + dk) and ng(i, j, k) != ng(i + di, j + dj, k + dk):
                            m |= 1 << a
                first[i, j, k], mask[i, j, k] = n, m
                n += bin(m).count("1")
    tri, cell = [], []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corners = [(i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)) for c in range(8)]
                if not all(kn(*v) for v in corners):
                    continue
                case = sum(1 << c for c in range(8) if ng(*corners[c]))
                for t3 in TABLE[case]:
                    row = []
                    for e in t3:
                        a = e // 4
                        v = corners[GEN.corner_index(GEN.edge_ends(e)[0])]
                        assert mask[v] >> a & 1
                        row.append(first[v] + bin(mask[v] & ((1 << a) - 1)).count("1"))
                    tri.append(row)
                    cell.append((k * ny + j) * nx + i)
    return np.asarray(tri, np.int32).reshape(-1, 3), np.asarray(cell, np.int64)


def mesh_outputs(state, origin, voxel, min_weight, cap, cap_tri, fill, tri_fill=-9):
    """What relpose_tsdf_mesh leaves in pre-filled outputs: tsdf_model.surface_outputs' dict plus "triangles" i32 [S,cap_tri,3] (rows beyond
    the count keep tri_fill) and "n_triangles" i32 [S]."""
    out = TM.surface_outputs(state, origin, voxel, min_weight, cap, fill)
    S = state["tsdf_sum"].shape[0]
    out["triangles"] = np.full((S, cap_tri, 3), tri_fill, np.int32)
    out["n_triangles"] = np.zeros(S, np.int32)
    for s in range(S):
        tri, _ = triangles(state["tsdf_sum"][s], state["weight"][s], min_weight)
        out["n_triangles"][s] = len(tri)
        out["triangles"][s, :min(len(tri), cap_tri)] = tri[:cap_tri]
    return out


# ---------------------------------------------------------------------------------------------- properties of a mesh
def directed_edges(tri):
    """-> i64 [3n, 2]: (a, b) for every triangle side in winding order"""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_report(tri):
    """-> (duplicates: directed edges that occur more than once, unpaired i64 [m,2]: directed edges whose reverse does not occur)"""
    d = directed_edges(tri)
    if len(d) == 0:
        return 0, d
    big = int(d.max()) + 1
    key = d[:, 0] * big + d[:, 1]
    uniq, cnt = np.unique(key, return_counts=True)
    rev = d[:, 1] * big + d[:, 0]
    return int((cnt > 1).sum()), d[~np.isin(rev, uniq)]
