"""numpy model of the RANSAC feature-registration contract, the baseline `--method gs` of the reference
(baselines.py:52-81).  Not a test file: test_ransac_cpu.py and test_gpu_ransac.py import it.

The front end is fgr_model's (§4.6 stages 1-4 and the fp32 feature nearest neighbour).  Every RANSAC step is restated in the order
csrc/ransac.hip evaluates it (csrc/rp_math.h's Horn included), so the validated set, the inlier counts and rmse compare bitwise."""
import numpy as np

import fgr_model as F

MAX_DIST = 0.075             # voxel * 1.5, baselines.py:61
EDGE = 0.9                   # CorrespondenceCheckerBasedOnEdgeLength(0.9), :71
MAX_ITERATIONS, MAX_VALIDATIONS = 4000000, 500      # RANSACConvergenceCriteria(4000000, 500), :72
MAX_POINTS = F.MAX_POINTS
STATUS_OK, STATUS_FEW_POINTS, STATUS_OVERFLOW, STATUS_NO_HYPOTHESIS = 0, 1, 3, 4
THREADS, WAVES = 256, 4      # the validation block: 256 threads, 4 waves of 64


# ------------------------------------------------------------------------------------------------ 2. draws
def draw(seed, t, k, n):
    """Source voxel of draw k of iteration t: splitmix64(seed * 0x9E3779B97F4A7C15 + 4 t + k) mod n (all mod 2^64)."""
    base = np.uint64((int(seed) * 0x9E3779B97F4A7C15) & F.M64)
    with np.errstate(over="ignore"):
        x = base + np.asarray(t, np.uint64) * np.uint64(4) + np.uint64(k)
    return (F.splitmix(x) % np.uint64(n)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 4. Horn (rp_math.h)
def horn(M):
    """rp_horn_rotation for [m,3,3] f64: Horn's 4x4 N from M = sum s t^T, its leading eigenvector by cyclic Jacobi (at most 32 sweeps
    of the rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), stopping when off == 0 or off <= 1e-34 diag), then the quaternion's
    rotation -> R [m,3,3] with t ~ R s."""
    M = np.asarray(M, np.float64)
    m = len(M)
    g = lambda a, b: M[:, a, b]
    N = np.empty((m, 4, 4))
    N[:, 0, 0] = (g(0, 0) + g(1, 1)) + g(2, 2)
    N[:, 0, 1] = N[:, 1, 0] = g(1, 2) - g(2, 1)
    N[:, 0, 2] = N[:, 2, 0] = g(2, 0) - g(0, 2)
    N[:, 0, 3] = N[:, 3, 0] = g(0, 1) - g(1, 0)
    N[:, 1, 1] = (g(0, 0) - g(1, 1)) - g(2, 2)
    N[:, 1, 2] = N[:, 2, 1] = g(0, 1) + g(1, 0)
    N[:, 1, 3] = N[:, 3, 1] = g(0, 2) + g(2, 0)
    N[:, 2, 2] = (g(1, 1) - g(0, 0)) - g(2, 2)
    N[:, 2, 3] = N[:, 3, 2] = g(1, 2) + g(2, 1)
    N[:, 3, 3] = (g(2, 2) - g(0, 0)) - g(1, 1)
    V = np.tile(np.eye(4), (m, 1, 1))
    active = np.ones(m, bool)
    sq = lambda a, b: N[:, a, b] * N[:, a, b]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(32):
            off = ((sq(0, 1) + sq(0, 2)) + (sq(0, 3) + sq(1, 2))) + (sq(1, 3) + sq(2, 3))
            diag = (sq(0, 0) + sq(1, 1)) + (sq(2, 2) + sq(3, 3))
            active &= ~((off == 0.0) | (off <= 1e-34 * diag))
            if not active.any():
                break
            for P, Q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                apq = N[:, P, Q].copy()
                go = active & (apq != 0.0)
                theta = (N[:, Q, Q] - N[:, P, P]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                c3, s3, g3 = c[:, None], s[:, None], go[:, None]
                rot = lambda x, y: (np.where(g3, c3 * x - s3 * y, x), np.where(g3, s3 * x + c3 * y, y))
                N[:, :, P], N[:, :, Q] = rot(N[:, :, P].copy(), N[:, :, Q].copy())      # columns, then rows, then V's columns
                N[:, P, :], N[:, Q, :] = rot(N[:, P, :].copy(), N[:, Q, :].copy())
                V[:, :, P], V[:, :, Q] = rot(V[:, :, P].copy(), V[:, :, Q].copy())
    best = N[:, 0, 0].copy()
    v = V[:, :, 0].copy()
    for k in (1, 2, 3):
        up = N[:, k, k] > best
        best = np.where(up, N[:, k, k], best)
        v = np.where(up[:, None], V[:, :, k], v)
    nrm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + (v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]))
    a, b, c, d = (v[:, i] / nrm for i in range(4))
    R = np.empty((m, 3, 3))
    R[:, 0, 0] = ((a * a + b * b) - c * c) - d * d
    R[:, 0, 1] = 2 * (b * c - a * d)
    R[:, 0, 2] = 2 * (b * d + a * c)
    R[:, 1, 0] = 2 * (c * b + a * d)
    R[:, 1, 1] = ((a * a - b * b) + c * c) - d * d
    R[:, 1, 2] = 2 * (c * d - a * b)
    R[:, 2, 0] = 2 * (d * b - a * c)
    R[:, 2, 1] = 2 * (d * c + a * b)
    R[:, 2, 2] = ((a * a - b * b) - c * c) + d * d
    return R


def apply(R, t, p):
    """q = R p + t per row, ((R_a0 p0 + R_a1 p1) + R_a2 p2) + t_a; R [m,3,3], t [m,3], p [m,3] -> [m,3]."""
    return np.stack([((R[:, a, 0] * p[:, 0] + R[:, a, 1] * p[:, 1]) + R[:, a, 2] * p[:, 2]) + t[:, a] for a in range(3)], 1)


# ------------------------------------------------------------------------------------------------ 3-5. one hypothesis per iteration
def edge_ok(s, q):
    """CorrespondenceCheckerBasedOnEdgeLength(0.9) on samples s, q [m,4,3]: False if any pair j < k has ds < 0.9 dt or dt < 0.9 ds."""
    ok = np.ones(len(s), bool)
    for j in range(4):
        for k in range(j + 1, 4):
            ds, dt = F._norm_rows(s[:, j] - s[:, k]), F._norm_rows(q[:, j] - q[:, k])
            ok &= ~((ds < EDGE * dt) | (dt < EDGE * ds))
    return ok


def estimate(s, q):
    """Point-to-point estimate of samples s -> q [m,4,3]: centroids (((x0 + x1) + x2) + x3) / 4, M summed in k order, Horn,
    t = c_t - R c_s -> (R [m,3,3], t [m,3])."""
    cs = (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]) / 4.0
    ct = (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]) / 4.0
    ds, dq = s - cs[:, None], q - ct[:, None]
    M = ds[:, 0, :, None] * dq[:, 0, None, :]
    for k in range(1, 4):
        M = M + ds[:, k, :, None] * dq[:, k, None, :]
    R = horn(M)
    return R, ct - apply(R, np.zeros_like(cs), cs)


def distance_ok(R, t, s, q):
    """CorrespondenceCheckerBasedOnDistance(0.075): False if any k has |R s_k + t - q_k| > 0.075."""
    ok = np.ones(len(s), bool)
    for k in range(4):
        ok &= ~(F._norm_rows(apply(R, t, s[:, k]) - q[:, k]) > MAX_DIST)
    return ok


def hypotheses(ps, pt, nn, t, seed):
    """Iterations t [m] -> (passed both checkers [m], R [m,3,3], tr [m,3]); R, tr are NaN where the edge test failed."""
    t = np.asarray(t, np.int64)
    idx = np.stack([draw(seed, t, k, len(ps)) for k in range(4)], 1)
    s, q = ps[idx], pt[nn[idx]]
    ok = edge_ok(s, q)
    R, tr = np.full((len(t), 3, 3), np.nan), np.full((len(t), 3), np.nan)
    if ok.any():
        R[ok], tr[ok] = estimate(s[ok], q[ok])
        ok[ok] = distance_ok(R[ok], tr[ok], s[ok], q[ok])
    return ok, R, tr


def screen(ps, pt, nn, seed=0, max_iterations=MAX_ITERATIONS, max_validations=MAX_VALIDATIONS, chunk=65536):
    """Step 6: the first max_validations iterations that pass both checkers -> (val_iter [k], n_iterations)."""
    out = []
    for t0 in range(0, max_iterations, chunk):
        t = np.arange(t0, min(t0 + chunk, max_iterations), dtype=np.int64)
        ok, _, _ = hypotheses(ps, pt, nn, t, seed)
        out.extend(t[ok][:max_validations - len(out)].tolist())
        if len(out) == max_validations:
            return np.array(out, np.int64), out[-1] + 1
    return np.array(out, np.int64), max_iterations


# ------------------------------------------------------------------------------------------------ 7. validation
class CellGrid:
    """Target voxels bucketed in cubic cells of 0.08 (> 0.075: a query's ball meets its 27 surrounding cells at most)."""
    H = 0.08

    def __init__(self, pts):
        self.pts = pts
        self.lo = pts.min(0) - 2 * self.H
        c = np.floor((pts - self.lo) / self.H).astype(np.int64)
        self.dim = c.max(0) + 3
        key = (c[:, 0] * self.dim[1] + c[:, 1]) * self.dim[2] + c[:, 2]
        self.order = np.argsort(key, kind="stable")
        self.keys = key[self.order]

    def min_d2(self, q):
        """Smallest d2 = (dx^2 + dy^2) + dz^2 (d = target - query) below 0.075^2 of every query [m,3]; inf where none is."""
        r2 = MAX_DIST * MAX_DIST
        best = np.full(len(q), np.inf)
        with np.errstate(invalid="ignore"):
            f = np.floor((q - self.lo) / self.H)
        inside = np.all((f >= 0) & (f < self.dim - 1) & np.isfinite(f), 1)
        qi, c = np.flatnonzero(inside), f[inside].astype(np.int64)
        qq = q[qi]
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                for oz in (-1, 0, 1):
                    key = ((c[:, 0] + ox) * self.dim[1] + (c[:, 1] + oy)) * self.dim[2] + (c[:, 2] + oz)
                    a, b = np.searchsorted(self.keys, key, "left"), np.searchsorted(self.keys, key, "right")
                    for j in range(int((b - a).max()) if len(a) else 0):
                        m = a + j < b
                        p = self.pts[self.order[a[m] + j]]
                        d = p - qq[m]
                        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                        sel = qi[m]
                        best[sel] = np.where(d2 < np.minimum(best[sel], r2), d2, best[sel])
        return best


def reduce_sum(x):
    """The validation block's fixed order for x [h, n] (one row per hypothesis): thread i % 256 sums its points in order, a xor tree
    (offsets 32 .. 1) over each wave's 64 lanes, then the 4 wave sums left to right -> [h]."""
    h, n = x.shape
    J = -(-n // THREADS)
    xp = np.zeros((h, J * THREADS), x.dtype)
    xp[:, :n] = x
    xp = xp.reshape(h, J, THREADS)
    s = xp[:, 0].copy()
    for j in range(1, J):
        s = s + xp[:, j]
    w = s.reshape(h, WAVES, 64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lanes ^ m]
    w = w[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def validate(ps, grid, R, tr, chunk=16):
    """For each hypothesis: q = R p + t over the source voxels in order, the nearest target voxel, inlier if d2 < 0.075^2 ->
    (inlier counts [h] i32, rmse [h] = sqrt(sum of inlier d2 / inliers), 0 without inliers)."""
    inl, err = [], []
    for h0 in range(0, len(R), chunk):
        Rc, tc = R[h0:h0 + chunk], tr[h0:h0 + chunk]
        h, n = len(Rc), len(ps)
        q = apply(np.repeat(Rc, n, 0), np.repeat(tc, n, 0), np.tile(ps, (h, 1)))
        d2 = grid.min_d2(q).reshape(h, n)
        hit = np.isfinite(d2)
        cnt = hit.sum(1).astype(np.int32)
        tot = reduce_sum(np.where(hit, d2, 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            err.append(np.where(cnt > 0, np.sqrt(tot / cnt.astype(np.float64)), 0.0))
        inl.append(cnt)
    return (np.concatenate(inl) if inl else np.zeros(0, np.int32)), (np.concatenate(err) if err else np.zeros(0))


# ------------------------------------------------------------------------------------------------ 8. selection + the pipeline
def select(inliers, err):
    """Open3D's rule from (0 inliers, rmse 0): more inliers, or as many and a smaller rmse -> best slot or -1."""
    best, bi, br = -1, 0, 0.0
    for v, (n, e) in enumerate(zip(inliers.tolist(), err.tolist())):
        if n > bi or (n == bi and e < br):
            best, bi, br = v, n, e
    return best


def register(pc_src, pc_tgt, seed=0, max_points=MAX_POINTS, max_iterations=MAX_ITERATIONS, max_validations=MAX_VALIDATIONS):
    """numpy [P,3] x 2 (valid points only) -> dict: pose [4,4], status, the per-pair outputs and every stage."""
    out = {"pose": np.eye(4), "status": STATUS_OK, "fitness": 0.0, "inlier_rmse": 0.0, "n_iterations": 0, "n_validations": 0,
           "best_index": -1}
    ds, _, _ = F.voxel_down(pc_src)
    dt, _, _ = F.voxel_down(pc_tgt)
    out.update(down_src=ds, down_tgt=dt)
    if len(ds) > max_points or len(dt) > max_points:
        out["status"] = STATUS_OVERFLOW
        return out
    if len(ds) < 3 or len(dt) < 3:
        out["status"] = STATUS_FEW_POINTS
        return out
    fs, ft = F.features(ds), F.features(dt)
    nn = F.nn_f32(fs["fpfh"].astype(np.float32), ft["fpfh"].astype(np.float32))
    out.update(fpfh_src=fs["fpfh"], fpfh_tgt=ft["fpfh"], nn=nn)
    vi, nit = screen(ds, dt, nn, seed, max_iterations, max_validations)
    _, R, tr = hypotheses(ds, dt, nn, vi, seed)
    inl, err = validate(ds, CellGrid(dt), R, tr)
    best = select(inl, err)
    out.update(val_iter=vi, val_inliers=inl, val_err=err, n_iterations=nit, n_validations=len(vi), best_index=best)
    if best < 0:
        out["status"] = STATUS_NO_HYPOTHESIS
        return out
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R[best], tr[best]
    out.update(pose=T, fitness=inl[best] / len(ds), inlier_rmse=err[best])
    return out
