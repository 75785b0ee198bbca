"""The contract of relpose_mesh_components and relpose_mesh_filter (include/relpose.h) in numpy.  Test infrastructure, not
product code: the GPU tests demand that the kernels reproduce every array here bit for bit.  The labelling is a plain union-find loop over
the vertices (the smaller index becomes the root, so a component's root is its smallest vertex index); the areas are numpy float64, every
operation rounded on its own."""
import numpy as np

STAT_KEYS = ("comp_root", "comp_vertices", "comp_triangles", "comp_area")
LABEL_KEYS = ("vertex_label", "tri_label", "n_components", "bad_triangles")
KEYS = LABEL_KEYS + STAT_KEYS
FILTER_KEYS = ("points", "normals", "colors", "valid", "n_points", "triangles", "n_triangles", "vertex_map")
AREA_CLAMP = 2147483648.0


def counts(n_points, n_triangles, cap, cap_tri):
    """the vertices and triangle rows of a scene that are read"""
    return min(max(int(n_points), 0), cap), min(max(int(n_triangles), 0), cap_tri)


def label_scene(tri, nv):
    """tri i32 [nt,3], nv vertices -> (vertex_label i32 [nv], tri_label i32 [nt], roots i64 [n_components] ascending, bad)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    good = ((tri >= 0) & (tri < nv)).all(1)
    parent = list(range(nv))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    used = np.zeros(nv, bool)
    for a, b, c in tri[good].tolist():
        used[[a, b, c]] = True
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    root = np.array([find(v) for v in range(nv)], np.int64)
    roots = np.unique(root[used])                                              # ascending smallest indices
    vlabel = np.full(nv, -1, np.int32)
    vlabel[used] = np.searchsorted(roots, root[used])
    tlabel = np.full(len(tri), -1, np.int32)
    tlabel[good] = vlabel[tri[good, 0]]
    return vlabel, tlabel, roots, int((~good).sum())


def area_terms(points, tri, area_scale):
    """i64 [n]: llrint(min(A area_scale, 2^31)) per triangle, 0 where the product is not finite"""
    p0, p1, p2 = (np.asarray(points, np.float64)[tri[:, k]] for k in range(3))
    with np.errstate(all="ignore"):
        u, w = p1 - p0, p2 - p0
        cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        q = np.sqrt((cx * cx + cy * cy) + cz * cz) * 0.5 * np.float64(area_scale)
        fin = np.isfinite(q)
        return np.where(fin, np.rint(np.minimum(np.where(fin, q, 0.0), AREA_CLAMP)), 0.0).astype(np.int64)


def components(mesh, cap_comp, area_scale, areas=True):
    """mesh: {"points" f64 [S,cap,3], "n_points" [S], "triangles" i32 [S,cap_tri,3], "n_triangles" [S]} -> what relpose_mesh_components writes:
    the KEYS arrays (statistics [S,cap_comp]; entries at and beyond n_components hold -1, 0, 0, 0; areas=False is the call without points)."""
    S, cap = mesh["points"].shape[:2]
    cap_tri = mesh["triangles"].shape[1]
    out = {"vertex_label": np.full((S, cap), -1, np.int32), "tri_label": np.full((S, cap_tri), -1, np.int32), "n_components": np.zeros(S, np.int32),
           "bad_triangles": np.zeros(S, np.int32), "comp_root": np.full((S, cap_comp), -1, np.int32), "comp_vertices": np.zeros((S, cap_comp), np.int32),
           "comp_triangles": np.zeros((S, cap_comp), np.int32), "comp_area": np.zeros((S, cap_comp), np.int64)}
    for s in range(S):
        nv, nt = counts(mesh["n_points"][s], mesh["n_triangles"][s], cap, cap_tri)
        tri = mesh["triangles"][s, :nt]
        vl, tl, roots, bad = label_scene(tri, nv)
        out["vertex_label"][s, :nv], out["tri_label"][s, :nt] = vl, tl
        out["n_components"][s], out["bad_triangles"][s] = len(roots), bad
        n = min(len(roots), cap_comp)
        out["comp_root"][s, :n] = roots[:n]
        out["comp_vertices"][s] = np.bincount(vl[vl >= 0], minlength=max(cap_comp, 1))[:cap_comp]
        out["comp_triangles"][s] = np.bincount(tl[tl >= 0], minlength=max(cap_comp, 1))[:cap_comp]
        if areas and (tl >= 0).any():
            g = tl >= 0
            a = area_terms(mesh["points"][s], tri[g].astype(np.int64), area_scale)
            np.add.at(out["comp_area"][s], tl[g][tl[g] < cap_comp], a[tl[g] < cap_comp])      # integer sums: any order
    return out


def filter_outputs(mesh, comps, keep, drop_unused, before):
    """What relpose_mesh_filter leaves in the pre-filled outputs `before` (a dict of FILTER_KEYS arrays, "colors" None without colours):
    survivors in order, rows beyond the new counts untouched, valid and vertex_map written whole."""
    out = {k: (None if v is None else v.copy()) for k, v in before.items()}
    S, cap = mesh["points"].shape[:2]
    cap_tri = mesh["triangles"].shape[1]
    keep = np.asarray(keep).astype(bool).reshape(S, -1)
    cap_comp = keep.shape[1]
    kept = lambda s, lab: (lab >= 0) & (lab < cap_comp) & np.concatenate([keep[s], [False]])[np.clip(lab, 0, cap_comp)]
    for s in range(S):
        nv, nt = counts(mesh["n_points"][s], mesh["n_triangles"][s], cap, cap_tri)
        vl, tl = comps["vertex_label"][s, :nv], comps["tri_label"][s, :nt]
        sv = np.where(vl < 0, not drop_unused, kept(s, vl))
        st = kept(s, tl)
        vmap = np.full(cap, -1, np.int32)
        vmap[:nv][sv] = np.arange(int(sv.sum()))
        n = int(sv.sum())
        for k in ("points", "normals", "colors"):
            if out[k] is not None:
                out[k][s, :n] = mesh[k][s, :nv][sv]
        out["valid"][s] = np.arange(cap) < n
        out["n_points"][s], out["n_triangles"][s] = n, int(st.sum())
        t = mesh["triangles"][s, :nt][st].astype(np.int64)
        inside = (t >= 0) & (t < nv)
        out["triangles"][s, :len(t)] = np.where(inside, vmap[np.clip(t, 0, cap - 1)], -1)
        out["vertex_map"][s] = vmap
    return out


def scipy_partition(tri, nv):
    """the same partition from scipy.sparse.csgraph.connected_components -> (n_components over used vertices, label per vertex or -1), the
    labels in scipy's own numbering"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    tri = tri[((tri >= 0) & (tri < nv)).all(1)]
    i = np.concatenate([tri[:, 0], tri[:, 0]])
    j = np.concatenate([tri[:, 1], tri[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(nv, nv)), directed=False)
    used = np.zeros(nv, bool)
    used[tri.reshape(-1)] = True
    lab = np.where(used, lab, -1)
    return len(np.unique(lab[used])), lab
