"""numpy statement of relpose_overlap's contract (include/relpose.h): test infrastructure, not product code.

Two models of the same numbers:
  brute   the definition.  Every valid query point is moved by the pose, row by row as ((T0 a + T1 b) + T2 c) + T3, its squared distance
          to every valid reference point is d2 = (dx dx + dy dy) + dz dz with d = q - r, the point's distance is sqrt(min d2), it hits
          when that is < max_dist; hits counts them and nn_min is the smallest distance over the valid query points (+inf without a pair
          with a finite d2).  These are nn_dist_kernel's expressions (geometry.hip), every operation rounded on its own.
  fast    brute's bits for large clouds (query_brute_fast: a k-d tree finds the few pairs worth the exact expression).
  grid    the statement the kernel's search rests on: cell(p) = floor((p - min) / edge) per axis with min the reference cloud's minimum
          over its finite valid points and edge = max_dist (1 + 2^-10); a query point's candidates are the reference points whose cell
          differs from its own by at most 1 on every axis (the 27-cell neighbourhood); hits come from the candidates alone.  nn_min is
          the candidates' minimum when a point hits and the brute closest pair otherwise (the kernel's pruned pass is exact).
All inputs are float64 numpy: pc [n,P,3], valid [n,P] (bool / uint8, or None), query / ref cloud indices [Q], pose [Q,4,4]."""
import numpy as np

EDGE_MARGIN = 1.0 + 1.0 / 1024.0


def moved(pc, T):
    a, b, c = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * a + T[r, 1] * b) + T[r, 2] * c) + T[r, 3] for r in range(3)], 1)


def _d2(q, r):
    with np.errstate(all="ignore"):
        dx, dy, dz = q[:, None, 0] - r[None, :, 0], q[:, None, 1] - r[None, :, 1], q[:, None, 2] - r[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    if np.isfinite(q).all() and np.isfinite(r).all() and np.isfinite(d2).all():
        return d2
    return np.where(np.isfinite(d2), d2, np.inf)               # a pair with a non-finite d2 is never a neighbour


def _valid(pc, valid):
    return np.ones(pc.shape[:2], bool) if valid is None else np.asarray(valid).astype(bool)


def _finish(best, vq, max_dist):
    """per-point minimum d2 [P] (inf = none) -> (hits, hit [P] u8, nn_min)"""
    dist = np.sqrt(best)
    hit = (dist < max_dist) & vq
    nn = dist[vq].min() if vq.any() else np.inf
    return int(hit.sum()), hit.astype(np.uint8), float(nn)


def query_brute(pc, valid, qc, rc, T, max_dist=0.08, chunk=512):
    v = _valid(pc, valid)
    q = moved(pc[qc], T)
    r = pc[rc][v[rc]]
    best = np.full(len(q), np.inf)
    if len(r):
        for s in range(0, len(q), chunk):
            best[s:s + chunk] = _d2(q[s:s + chunk], r).min(1)
    return _finish(best, v[qc], max_dist)


def query_brute_fast(pc, valid, qc, rc, T, max_dist=0.08):
    """query_brute for large clouds, the same bits: a k-d tree (scipy) names, for every query point, the reference points within
    (1 + 2^-20) of its nearest neighbour's distance -- the tree's distance and the contract's differ by a few roundings of 2^-53, so the
    pair with the smallest contract d2 is among them -- and the contract's expression is evaluated on those pairs only.  Falls back to
    query_brute when a coordinate is not finite."""
    from scipy.spatial import cKDTree
    v = _valid(pc, valid)
    q = moved(pc[qc], T)
    r = pc[rc][v[rc]]
    if not len(r) or not (np.isfinite(q).all() and np.isfinite(r).all()):
        return query_brute(pc, valid, qc, rc, T, max_dist)
    tree = cKDTree(r)
    d, _ = tree.query(q, k=1)
    near = tree.query_ball_point(q, d * (1.0 + 2.0 ** -20) + 1e-300)
    rows = np.repeat(np.arange(len(q)), [len(c) for c in near])
    cols = np.concatenate([np.asarray(c, np.int64) for c in near])
    dx, dy, dz = q[rows, 0] - r[cols, 0], q[rows, 1] - r[cols, 1], q[rows, 2] - r[cols, 2]
    best = np.full(len(q), np.inf)
    np.minimum.at(best, rows, (dx * dx + dy * dy) + dz * dz)
    return _finish(best, v[qc], max_dist)


def cells(p, mn, edge):
    with np.errstate(all="ignore"):
        return np.floor((p - mn) / edge)


def query_grid(pc, valid, qc, rc, T, max_dist=0.08, chunk=512):
    v = _valid(pc, valid)
    q = moved(pc[qc], T)
    r = pc[rc][v[rc] & np.isfinite(pc[rc]).all(1)]
    best = np.full(len(q), np.inf)
    if len(r):
        edge = max_dist * EDGE_MARGIN
        mn = r.min(0)
        # integer cells; a query point far outside the grid (or not finite) is parked two cells beyond any reference cell
        as_int = lambda c: np.where(np.isfinite(c), np.clip(c, -4.0, 2.0 ** 30), -4.0).astype(np.int32)
        cr, cq = as_int(cells(r, mn, edge)), as_int(cells(q, mn, edge))
        for s in range(0, len(q), chunk):
            with np.errstate(all="ignore"):
                cand = np.abs(cq[s:s + chunk, None, 0] - cr[None, :, 0]) <= 1
                for a in (1, 2):
                    cand &= np.abs(cq[s:s + chunk, None, a] - cr[None, :, a]) <= 1
            best[s:s + chunk] = np.where(cand, _d2(q[s:s + chunk], r), np.inf).min(1)
    hits, hit, nn = _finish(best, v[qc], max_dist)
    if hits == 0:                                               # clouds that do not touch: the closest pair
        nn = query_brute(pc, valid, qc, rc, T, max_dist)[2]
    return hits, hit, nn


def overlap(pc, valid, query_cloud, ref_cloud, pose, max_dist=0.08, model="brute"):
    """-> {"hits" [Q] i32, "nn_min" [Q] f64, "n_valid" [n] i32, "hit" [Q,P] u8}"""
    fn = {"brute": query_brute, "grid": query_grid, "fast": query_brute_fast}[model]
    pc = np.asarray(pc, np.float64)
    Q = len(query_cloud)
    out = {"hits": np.zeros(Q, np.int32), "nn_min": np.zeros(Q), "hit": np.zeros((Q, pc.shape[1]), np.uint8),
           "n_valid": _valid(pc, valid).sum(1).astype(np.int32)}
    for k in range(Q):
        out["hits"][k], out["hit"][k], out["nn_min"][k] = fn(pc, valid, int(query_cloud[k]), int(ref_cloud[k]), np.asarray(pose[k], np.float64), max_dist)
    return out


def matrix_queries(R):
    """The M (M - 1) directed queries of M posed clouds (world -> camera poses R): (query cloud, ref cloud, pose) with T_ij = R_j inv(R_i)."""
    M = len(R)
    ij = [(i, j) for i in range(M) for j in range(M) if i != j]
    inv = [np.linalg.inv(R[i]) for i in range(M)]
    return np.array([i for i, _ in ij], np.int32), np.array([j for _, j in ij], np.int32), np.stack([np.matmul(R[j], inv[i]) for i, j in ij])


def fractions(res, qc, rc, M):
    """overlap() of matrix_queries -> frac [M,M] (the diagonal is 1 for a non-empty cloud)"""
    n = res["n_valid"].astype(np.float64)
    frac = np.diag((n > 0).astype(np.float64))
    for k, (i, j) in enumerate(zip(qc, rc)):
        frac[i, j] = res["hits"][k] / n[i] if n[i] > 0 else 0.0
    return frac


def pair_statistics(pc, valid, R_gt, max_dist=0.08, model="brute"):
    """util.point_cloud_overlap's four numbers for the paired layout (cloud 2b the source, 2b + 1 the target), through the model:
    -> [B,4] (overlap, cam_dist, pc_dist, pc_nn); pc_dist with the reference's numpy expression on the valid points."""
    pc = np.asarray(pc, np.float64)
    v = _valid(pc, valid)
    B = len(R_gt)
    out = np.zeros((B, 4))
    for b in range(B):
        R = np.asarray(R_gt[b], np.float64)
        res = overlap(pc, valid, [2 * b, 2 * b + 1], [2 * b + 1, 2 * b], [R, np.linalg.inv(R)], max_dist, model)
        ps, pt = pc[2 * b][v[2 * b]], pc[2 * b + 1][v[2 * b + 1]]
        src_trans = np.matmul(R[:3, :3], ps.T) + R[:3, 3:4]
        out[b] = (max(res["hits"][0] / len(ps), res["hits"][1] / len(pt)), np.linalg.norm(R[:3, 3]),
                  np.linalg.norm(src_trans.mean(1) - pt.T.mean(1)), (res["nn_min"][0] + res["nn_min"][1]) / 2)
    return out
