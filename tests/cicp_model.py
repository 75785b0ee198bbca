"""numpy model of the coloured ICP contract, the three refinement levels of the reference's `--method cgs` baseline
(baselines.py:110-168; Park, Zhou, Koltun, ICCV 2017).  Not a test file: test_cicp_cpu.py and test_gpu_cicp.py import it.

Every stage is restated in the order csrc/cicp.hip evaluates it and takes its inputs as arrays, so a test can feed it the GPU's own
upstream results (normals, gradients, the transform of an iteration) and compare one stage at a time.  Searches are by value: the
candidate lattice below only has to return a superset of the ball, the distances and orders are the contract's."""
import numpy as np

from fgr_model import cholesky_solve, covariances, jacobi3, rot_zyx
from ransac_model import reduce_sum

RADII = (0.04, 0.02, 0.01)             # baselines.py:141
MAX_ITER = (50, 30, 14)                # :142
SLOT_OFF = (0, 50, 80)
SLOTS = 94                             # RELPOSE_CICP_TRACE_SLOTS
MAX_NN = 30                            # KDTreeSearchParamHybrid(radius * 2, 30), :156-159
LAMBDA_GEOMETRIC = 0.968               # Open3D's default
REL_FITNESS = REL_RMSE = 1e-6          # ICPConvergenceCriteria, :164-165
MAX_POINTS = 32768
STATUS_OK, STATUS_FEW_POINTS, STATUS_OVERFLOW = 0, 1, 3


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def intensity(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / 3.0


def transform(T, p):
    """q = T p per row, ((T_a0 p0 + T_a1 p1) + T_a2 p2) + T_a3."""
    return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1)


# ------------------------------------------------------------------------------------------------ 1. coloured voxel grid
def voxel_down(pts, colors, voxel):
    """pts, colors [P,3] f64 (the valid points, input order) -> (points [n,3], colours [n,3]) in ascending key order: §4.6 stage 1 with
    the voxel size as a parameter, colours averaged by the same sums and counts."""
    pts, colors = np.asarray(pts, np.float64), np.asarray(colors, np.float64)
    if len(pts) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    mb = pts.min(0) - 0.5 * voxel
    ijk = np.floor((pts - mb) / voxel).astype(np.int64)
    dy, dz = ijk[:, 1].max() + 1, ijk[:, 2].max() + 1
    key = (ijk[:, 0] * dy + ijk[:, 1]) * dz + ijk[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cnt = np.diff(np.r_[start, len(ks)])
    sp, sc = np.zeros((len(start), 3)), np.zeros((len(start), 3))
    for j in range(int(cnt.max())):                       # sequential sum of every voxel, in input order
        m = cnt > j
        sp[m] += pts[order[start[m] + j]]
        sc[m] += colors[order[start[m] + j]]
    cf = cnt[:, None].astype(np.float64)
    return sp / cf, sc / cf


# ------------------------------------------------------------------------------------------------ searches by value
def candidates(tgt, q, r):
    """-> [m, K] i64 indices into tgt (-1 padded) holding at least every target within r of each query (cubic cells of 1.001 r)."""
    m, h = len(q), r * 1.001
    if len(tgt) == 0 or m == 0:
        return np.full((m, 1), -1, np.int64)
    lo = tgt.min(0) - 2 * h
    c = np.floor((tgt - lo) / h).astype(np.int64)
    dim = c.max(0) + 3
    key = (c[:, 0] * dim[1] + c[:, 1]) * dim[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    keys = key[order]
    with np.errstate(invalid="ignore"):
        f = np.floor((q - lo) / h)
    inside = np.all(np.isfinite(f) & (f >= 1) & (f <= dim - 2), 1)
    qi, fc = np.flatnonzero(inside), f[inside].astype(np.int64)
    a, b = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                k = ((fc[:, 0] + ox) * dim[1] + (fc[:, 1] + oy)) * dim[2] + (fc[:, 2] + oz)
                a.append(np.searchsorted(keys, k, "left"))
                b.append(np.searchsorted(keys, k, "right"))
    a, b = np.array(a), np.array(b)
    cnt = b - a
    start = np.cumsum(cnt, 0) - cnt
    K = int(cnt.sum(0).max()) if len(qi) else 0
    cand = np.full((m, max(K, 1)), -1, np.int64)
    for o in range(27):
        for j in range(int(cnt[o].max()) if len(qi) else 0):
            sel = j < cnt[o]
            cand[qi[sel], start[o][sel] + j] = order[a[o][sel] + j]
    return cand


def _cand_d2(tgt, q, cand):
    d = tgt[np.maximum(cand, 0)] - q[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.where(cand >= 0, d2, np.inf)


def nearest(tgt, q, radius):
    """Nearest target of every query by d2 = (dx^2 + dy^2) + dz^2 (d = target - query), ties to the lower index; a correspondence iff
    d2 < radius^2 -> (corr [m] i32, -1 = none; d2 [m], 0 where none)."""
    cand = candidates(tgt, q, radius)
    d2 = _cand_d2(tgt, q, cand)
    with np.errstate(invalid="ignore"):
        d2 = np.where(d2 < radius * radius, d2, np.inf)
    best = d2.min(1)
    idx = np.where(d2 == best[:, None], cand, np.iinfo(np.int64).max).min(1)
    hit = np.isfinite(best)
    return np.where(hit, idx, -1).astype(np.int32), np.where(hit, best, 0.0)


def neighbors(pts, radius, max_nn=MAX_NN):
    """Hybrid search: up to max_nn points with d2 < radius^2, ordered by (d2, index) -> (idx [n, max_nn] i32 (-1 padded), count [n])."""
    n = len(pts)
    cand = candidates(pts, pts, radius)
    d2 = _cand_d2(pts, pts, cand)
    d2 = np.where(d2 < radius * radius, d2, np.inf)
    order = np.lexsort((cand, d2), axis=-1)
    cs, ds = np.take_along_axis(cand, order, 1), np.take_along_axis(d2, order, 1)
    if cs.shape[1] < max_nn:
        cs = np.concatenate([cs, np.full((n, max_nn - cs.shape[1]), -1, np.int64)], 1)
        ds = np.concatenate([ds, np.full((n, max_nn - ds.shape[1]), np.inf)], 1)
    cs, ds = cs[:, :max_nn], ds[:, :max_nn]
    return np.where(np.isfinite(ds), cs, -1).astype(np.int32), np.isfinite(ds).sum(1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 3. normals
def normals(pts, idx, cnt, origin=(0.0, 0.0, 0.0)):
    """§4.6 stage 3 over the whole list: covariance in list order, 6 Jacobi sweeps, the smallest-eigenvalue eigenvector (ties: lower
    index), normalised, turned so that n . (origin - p) >= 0; fewer than 3 neighbours: (0, 0, 1), turned the same way."""
    n = len(pts)
    m = np.asarray(cnt, np.int32)
    ev, V = jacobi3(covariances(pts, np.maximum(idx, 0), m))
    k = np.where(ev[:, 1] < ev[:, 0], 1, 0)
    k = np.where(ev[:, 2] < ev[np.arange(n), k], 2, k)
    nv = V[np.arange(n), :, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
        nv = nv / nn[:, None]
    nv[m < 3] = (0.0, 0.0, 1.0)
    w = np.asarray(origin, np.float64) - pts
    nv[_dot(nv, w) < 0] *= -1.0
    return nv


# ------------------------------------------------------------------------------------------------ solves
def chol_solve_batch(A, b):
    """cholesky_solve (fgr_model) for [n,k,k], [n,k] at once, the same expression order -> (x [n,k], ok [n]); a non-positive pivot
    gives ok False and x = 0."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    n, k = b.shape
    L = np.zeros((n, k, k))
    ok = np.ones(n, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(k):
            acc = np.zeros(n)
            for e in range(j):
                acc = acc + L[:, j, e] * L[:, j, e]
            s = A[:, j, j] - acc
            ok &= s > 0
            L[:, j, j] = np.sqrt(np.where(ok, s, 1.0))
            for i in range(j + 1, k):
                acc = np.zeros(n)
                for e in range(j):
                    acc = acc + L[:, i, e] * L[:, j, e]
                L[:, i, j] = (A[:, i, j] - acc) / L[:, j, j]
        y = np.zeros((n, k))
        for i in range(k):
            acc = np.zeros(n)
            for e in range(i):
                acc = acc + L[:, i, e] * y[:, e]
            y[:, i] = (b[:, i] - acc) / L[:, i, i]
        x = np.zeros((n, k))
        for i in reversed(range(k)):
            acc = np.zeros(n)
            for e in range(i + 1, k):
                acc = acc + L[:, e, i] * x[:, e]
            x[:, i] = (y[:, i] - acc) / L[:, i, i]
    x[~ok] = 0.0
    return x, ok


def pivots_positive(A):
    """True if cholesky_solve (fgr_model) meets no non-positive pivot on A."""
    return bool(chol_solve_batch(np.asarray(A)[None], np.zeros((1, len(A))))[1][0])


# ------------------------------------------------------------------------------------------------ 4. colour gradients
def gradients(pts, inten, nrm, idx, cnt):
    """Open3D's InitializePointCloudForColoredICP: per point with nn >= 4 the least-squares x of rows A_k = p_k - ((p_k - p) . n) n - p,
    b_k = I_k - I over the neighbours k = 1 .. nn-1 in list order and the last row (nn - 1) n, 0; A^T A x = A^T b by Cholesky; a
    non-positive pivot or nn < 4: zero."""
    n = len(pts)
    ata, atb = np.zeros((n, 6)), np.zeros((n, 3))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cnt = np.asarray(cnt)
    go = cnt >= 4
    for k in range(1, idx.shape[1]):
        a = np.flatnonzero(go & (k < cnt))
        if len(a) == 0:
            break
        j = idx[a, k]
        d = pts[j] - pts[a]
        s = _dot(d, nrm[a])
        A = (pts[j] - s[:, None] * nrm[a]) - pts[a]
        bk = inten[j] - inten[a]
        for e, (u, v) in enumerate(pairs):
            ata[a, e] += A[:, u] * A[:, v]
        atb[a] += A * bk[:, None]
    A = (cnt - 1).astype(np.float64)[:, None] * nrm
    for e, (u, v) in enumerate(pairs):
        ata[go, e] += (A[:, u] * A[:, v])[go]
    M = np.empty((n, 3, 3))
    for e, (u, v) in enumerate(pairs):
        M[:, u, v] = M[:, v, u] = ata[:, e]
    M[~go] = np.eye(3)
    x, ok = chol_solve_batch(M, atb)
    x[~(ok & go)] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ per level
def prepare_level(pc_src, col_src, pc_tgt, col_tgt, radius):
    """Stages 1-4 of one level -> dict: ps, cs (source voxels and colours), pt, ct, nbr, ncnt, normals, gradient (the target's)."""
    ps, cs = voxel_down(pc_src, col_src, radius)
    pt, ct = voxel_down(pc_tgt, col_tgt, radius)
    lv = {"ps": ps, "cs": cs, "pt": pt, "ct": ct}
    if len(pt):
        lv["nbr"], lv["ncnt"] = neighbors(pt, 2.0 * radius)
        lv["normals"] = normals(pt, lv["nbr"], lv["ncnt"])
        lv["gradient"] = gradients(pt, intensity(ct), lv["normals"], lv["nbr"], lv["ncnt"])
    return lv


# ------------------------------------------------------------------------------------------------ iteration
def evaluate(ps, pt, T, radius):
    """-> (q = T ps, corr [n] i32, ncorr, fitness, rmse): the sum of d2 in the fixed order of §4.7 stage 7."""
    q = transform(T, ps)
    corr, d2 = nearest(pt, q, radius)
    ncorr = int((corr >= 0).sum())
    tot = reduce_sum(d2[None])[0]
    rmse = float(np.sqrt(tot / float(ncorr))) if ncorr > 0 else 0.0
    return q, corr, ncorr, ncorr / float(len(ps)), rmse


def build_system(q, inten_s, corr, pt, inten_t, nrm, grad, lam=LAMBDA_GEOMETRIC):
    """The 21 + 6 sums of J^T J (upper triangle, row-major) and J^T r over the correspondences, in the fixed reduction order -> [27]."""
    hit = corr >= 0
    j = np.maximum(corr, 0)
    sg, sc = np.sqrt(lam), np.sqrt(1.0 - lam)
    vs, vt, nt, dit = q, pt[j], nrm[j], grad[j]
    d = vs - vt
    dn = _dot(d, nt)
    JG = np.concatenate([sg * _cross(vs, nt), sg * nt], 1)
    rG = sg * dn
    pr = (vs - dn[:, None] * nt) - vt
    is_proj = _dot(dit, pr) + inten_t[j]
    dd = _dot(dit, nt)
    dm = -(dit - dd[:, None] * nt)
    JI = np.concatenate([sc * _cross(vs, dm), sc * dm], 1)
    rI = sc * (inten_s - is_proj)
    rows = [JG[:, u] * JG[:, v] + JI[:, u] * JI[:, v] for u in range(6) for v in range(u, 6)]
    rows += [JG[:, u] * rG + JI[:, u] * rI for u in range(6)]
    with np.errstate(invalid="ignore"):
        return reduce_sum(np.where(hit[None, :], np.array(rows), 0.0))


def unpack_system(tot):
    A = np.zeros((6, 6))
    e = 0
    for u in range(6):
        for v in range(u, 6):
            A[u, v] = A[v, u] = tot[e]
            e += 1
    return A, np.asarray(tot[21:27], np.float64)


def step(lv, T, radius, lam=LAMBDA_GEOMETRIC, prev=None):
    """One iteration from the transform T (prev = (fitness, rmse) of the previous evaluation of the level, None for the first) -> dict:
    corr, ncorr, fitness, rmse, ended (the level ends here: stop rule, no correspondence or a non-positive pivot), x (the step or
    None) and T_next."""
    q, corr, ncorr, fit, rmse = evaluate(lv["ps"], lv["pt"], T, radius)
    out = {"corr": corr, "ncorr": ncorr, "fitness": fit, "rmse": rmse, "ended": False, "x": None, "T_next": T}
    if prev is not None and abs(fit - prev[0]) < REL_FITNESS and abs(rmse - prev[1]) < REL_RMSE:
        out["ended"] = True
        return out
    A, r = unpack_system(build_system(q, intensity(lv["cs"]), corr, lv["pt"], intensity(lv["ct"]), lv["normals"], lv["gradient"], lam))
    if ncorr == 0 or not pivots_positive(A):
        out["ended"] = True
        return out
    x = -cholesky_solve(A, r)
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = rot_zyx(x), x[3:]
    out.update(x=x, T_next=U @ T)
    return out


def run_level(lv, T, radius, max_iter, lam=LAMBDA_GEOMETRIC):
    """-> (T, fitness, rmse, n_iterations (evaluations made), trace: the list of step() results with 'T' added)."""
    prev, trace = None, []
    fit = rmse = 0.0
    for _ in range(max_iter):
        s = step(lv, T, radius, lam, prev)
        s["T"] = T
        trace.append(s)
        fit, rmse, prev = s["fitness"], s["rmse"], (s["fitness"], s["rmse"])
        T = s["T_next"]
        if s["ended"]:
            break
    return T, fit, rmse, len(trace), trace


def register(pc_src, col_src, pc_tgt, col_tgt, init=None, lam=LAMBDA_GEOMETRIC, max_points=MAX_POINTS, radii=RADII, max_iter=MAX_ITER):
    """numpy [P,3] x 4 (valid points only) -> dict: pose, status, per level fitness / inlier_rmse / n_iterations / level_pose, the
    levels' stages and traces."""
    L = len(radii)
    out = {"pose": np.eye(4), "status": STATUS_OK, "fitness": np.zeros(L), "inlier_rmse": np.zeros(L), "n_iterations": np.zeros(L, np.int32),
           "level_pose": np.tile(np.eye(4), (L, 1, 1)), "trace": [[] for _ in range(L)]}
    lvs = [prepare_level(pc_src, col_src, pc_tgt, col_tgt, r) for r in radii]
    out["levels"] = lvs
    counts = [len(lv[k]) for lv in lvs for k in ("ps", "pt")]
    if max(counts) > max_points:
        out["status"] = STATUS_OVERFLOW
        return out
    if min(counts) < 3:
        out["status"] = STATUS_FEW_POINTS
        return out
    T = np.eye(4) if init is None else np.array(init, np.float64)
    for l, (r, mi) in enumerate(zip(radii, max_iter)):
        T, out["fitness"][l], out["inlier_rmse"][l], out["n_iterations"][l], out["trace"][l] = run_level(lvs[l], T, r, mi, lam)
        out["level_pose"][l] = T
    out["pose"] = T
    return out
