"""numpy model of the FPFH + fast global registration contract, the baseline `--method fgs` of the reference
(baselines.py:36-50, 83-106).  Not a test file: test_fgr_cpu.py and test_gpu_fgr.py import it.

Every stage is restated in the order csrc/fgr.hip evaluates it, so the per-stage outputs compare bitwise (voxels, neighbour lists,
correspondences) or to rounding (normals, FPFH, pose)."""
import numpy as np

VOXEL = 0.05                 # baselines.py:91
R_NORMAL, NN_NORMAL = 0.10, 30          # voxel * 2, :40
R_FPFH, NN_FPFH = 0.25, 100             # voxel * 5, :45
MAX_CORR = 0.075             # voxel * 1.5, :92
DIVISION_FACTOR, ITERATIONS, TUPLE_SCALE, MAX_TUPLES = 1.4, 64, 0.95, 1000     # FastGlobalRegistrationOption defaults
MIN_CORR = 10                # fewer tuple correspondences than this: identity
MAX_POINTS = 32768           # RELPOSE_FGR_MAX_POINTS
STATUS_OK, STATUS_FEW_POINTS, STATUS_FEW_CORR, STATUS_OVERFLOW = 0, 1, 2, 3

# the 10 inner bin edges of the atan2 feature, theta_k = -pi + 2 pi k / 11, as directions (cos, sin); the same literals are in fgr.hip
EDGE_COS = np.array([-0.8412535328311811, -0.4154150130018863, 0.14231483827328512, 0.6548607339452851, 0.9594929736144975,
                     0.9594929736144975, 0.6548607339452851, 0.14231483827328512, -0.41541501300188616, -0.8412535328311813])
EDGE_SIN = np.array([-0.5406408174555978, -0.9096319953545184, -0.9898214418809327, -0.7557495743542583, -0.2817325568414295,
                     0.2817325568414295, 0.7557495743542583, 0.9898214418809327, 0.9096319953545186, 0.5406408174555974])

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ 1. voxel downsample
def voxel_down(pts):
    """pts [P,3] f64 (the valid points, input order) -> (points [n,3] in ascending key order, voxel x index [n], keys [n])."""
    pts = np.asarray(pts, np.float64)
    if len(pts) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64)
    mb = pts.min(0) - 0.5 * VOXEL
    ijk = np.floor((pts - mb) / VOXEL).astype(np.int64)
    dy, dz = ijk[:, 1].max() + 1, ijk[:, 2].max() + 1
    key = (ijk[:, 0] * dy + ijk[:, 1]) * dz + ijk[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cnt = np.diff(np.r_[start, len(ks)])
    sums = np.zeros((len(start), 3))
    for j in range(int(cnt.max())):                       # sequential sum of every voxel, in input order
        m = cnt > j
        sums[m] += pts[order[start[m] + j]]
    out = sums / cnt[:, None].astype(np.float64)
    return out, ks[start] // (dy * dz), ks[start]


# ------------------------------------------------------------------------------------------------ 2. hybrid neighbours
def neighbors(pts, radius=R_FPFH, max_nn=NN_FPFH):
    """Up to max_nn points with d2 < radius^2, ordered by (d2, index) -> (idx [n,max_nn] i32 (-1 padded), d2 [n,max_nn], count [n])."""
    n = len(pts)
    idx = np.full((n, max_nn), -1, np.int32)
    dd = np.zeros((n, max_nn))
    cnt = np.zeros(n, np.int32)
    r2 = radius * radius
    for q in range(n):
        d = pts - pts[q]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        c = np.flatnonzero(d2 < r2)
        c = c[np.lexsort((c, d2[c]))][:max_nn]
        cnt[q] = len(c)
        idx[q, :len(c)] = c
        dd[q, :len(c)] = d2[c]
    return idx, dd, cnt


# ------------------------------------------------------------------------------------------------ 3. normals
def jacobi3(A, sweeps=6):
    """Cyclic Jacobi on symmetric [n,3,3] f64, `sweeps` x the rotations (0,1), (0,2), (1,2); a rotation with a_pq == 0 is skipped.
    -> (eigenvalues [n,3] (the diagonal), eigenvectors [n,3,3] as columns)."""
    A = np.array(A, np.float64)
    n = len(A)
    V = np.tile(np.eye(3), (n, 1, 1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(sweeps):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[:, p, q]
                go = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                arp, arq = A[:, r, p], A[:, r, q]
                nrp, nrq = c * arp - s * arq, s * arp + c * arq
                for (a, b), v in (((p, p), app), ((q, q), aqq), ((p, q), 0.0 * apq), ((q, p), 0.0 * apq), ((r, p), nrp), ((p, r), nrp),
                                  ((r, q), nrq), ((q, r), nrq)):
                    A[:, a, b] = np.where(go, v, A[:, a, b])
                for k in range(3):
                    vkp, vkq = V[:, k, p], V[:, k, q]
                    V[:, k, p], V[:, k, q] = np.where(go, c * vkp - s * vkq, vkp), np.where(go, s * vkp + c * vkq, vkq)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V


def covariances(pts, idx, m):
    """Mean-centred covariance (1/m) of the first m[i] neighbours idx[i], summed sequentially in list order -> [n,3,3]."""
    n = len(pts)
    mf = np.maximum(m, 1).astype(np.float64)
    s = np.zeros((n, 3))
    for j in range(int(m.max()) if n else 0):
        a = j < m
        s[a] += pts[idx[a, j]]
    mean = s / mf[:, None]
    C = np.zeros((n, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(int(m.max()) if n else 0):
        a = j < m
        d = pts[idx[a, j]] - mean[a]
        for e, (u, v) in enumerate(pairs):
            C[a, e] += d[:, u] * d[:, v]
    C /= mf[:, None]
    out = np.empty((n, 3, 3))
    for e, (u, v) in enumerate(pairs):
        out[:, u, v] = out[:, v, u] = C[:, e]
    return out


def normals(pts, idx, d2, cnt, origin=(0.0, 0.0, 0.0)):
    """The first min(30, #{d2 < 0.1^2}) entries of the FPFH neighbour list (= the hybrid search r = 0.10, max_nn = 30); the
    smallest-eigenvalue eigenvector (ties: lower index), normalised, turned so that n . (origin - p) >= 0.  Fewer than 3
    neighbours: (0, 0, 1), turned the same way."""
    n = len(pts)
    rn2 = R_NORMAL * R_NORMAL
    inr = (d2 < rn2) & (np.arange(idx.shape[1])[None, :] < cnt[:, None])
    m = np.minimum(np.where(inr.all(1), idx.shape[1], np.argmin(inr, 1)), NN_NORMAL).astype(np.int32)
    ev, V = jacobi3(covariances(pts, idx, m))
    k = np.where(ev[:, 1] < ev[:, 0], 1, 0)
    k = np.where(ev[:, 2] < ev[np.arange(n), k], 2, k)
    nv = V[np.arange(n), :, k]
    nn = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
    nv = nv / nn[:, None]
    nv[m < 3] = (0.0, 0.0, 1.0)
    o = np.asarray(origin, np.float64)
    w = o - pts
    dot = (nv[:, 0] * w[:, 0] + nv[:, 1] * w[:, 1]) + nv[:, 2] * w[:, 2]
    nv[dot < 0] *= -1.0
    return nv


# ------------------------------------------------------------------------------------------------ 4. FPFH
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def angle_bin(x, y):
    """Bin of atan2(y, x) in 11 bins over (-pi, pi]: the number of edges theta_k <= the angle, by sign tests (no atan2)."""
    upper = y >= 0
    b = np.zeros(len(x), np.int32)
    for k in range(10):
        eu = EDGE_SIN[k] >= 0
        cr = x * EDGE_SIN[k] - y * EDGE_COS[k]
        less = ((~upper) & eu) | ((upper == eu) & (cr > 0))
        b += (~less).astype(np.int32)
    return b


def _lin_bin(f):
    return np.clip(np.floor(11 * (f + 1.0) * 0.5), 0, 10).astype(np.int32)


def pair_bins(p1, n1, p2, n2):
    """Open3D's ComputePairFeatures followed by the SPFH binning -> three bin indices [k] each (the zero feature -> bins 5, 5, 5)."""
    dp = p2 - p1
    L = np.sqrt(_dot(dp, dp))
    with np.errstate(divide="ignore", invalid="ignore"):
        a1, a2 = _dot(n1, dp) / L, _dot(n2, dp) / L
        swap = np.abs(a1) < np.abs(a2)              # acos(|a1|) > acos(|a2|)
        f2 = np.where(swap, -a2, a1)
        m1, m2 = np.where(swap[:, None], n2, n1), np.where(swap[:, None], n1, n2)
        dp = np.where(swap[:, None], -dp, dp)
        v = _cross(dp, m1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(m1, v)
        f1 = _dot(v, m2)
        b0, b1, b2 = angle_bin(_dot(m1, m2), _dot(w, m2)), _lin_bin(f1), _lin_bin(f2)
    zero = (L == 0) | (vn == 0)
    return np.where(zero, 5, b0), np.where(zero, 5, b1), np.where(zero, 5, b2)


def spfh(pts, nrm, idx, cnt):
    n = len(pts)
    h = np.zeros((n, 33))
    with np.errstate(divide="ignore"):
        incr = 100.0 / (cnt - 1).astype(np.float64)
    rows = np.arange(n)
    for k in range(1, idx.shape[1]):
        a = rows[k < cnt]
        if len(a) == 0:
            break
        j = idx[a, k]
        b0, b1, b2 = pair_bins(pts[a], nrm[a], pts[j], nrm[j])
        h[a, b0] += incr[a]
        h[a, 11 + b1] += incr[a]
        h[a, 22 + b2] += incr[a]
    return h


def fpfh(pts, nrm, idx, d2, cnt):
    """FPFH(i) = SPFH(i) + (100 / S_b) * sum_k SPFH(k) / d2_k per feature block b (S_b = the block's weighted sum), k over the
    neighbours after the first, d2 == 0 skipped; a point with no neighbour but itself: zeros (Open3D's ComputeFPFHFeature)."""
    S = spfh(pts, nrm, idx, cnt)
    n = len(pts)
    F = np.zeros((n, 33))
    sb = np.zeros((n, 3))
    rows = np.arange(n)
    for k in range(1, idx.shape[1]):
        a = rows[(k < cnt)]
        a = a[d2[a, k] != 0]
        if len(a) == 0:
            if not (k < cnt).any():
                break
            continue
        Sk, dist = S[idx[a, k]], d2[a, k]
        for j in range(33):
            val = Sk[:, j] / dist
            sb[a, j // 11] += val
            F[a, j] += val
    with np.errstate(divide="ignore"):
        sb = np.where(sb != 0, 100.0 / sb, sb)
    F = F * np.repeat(sb, 11, axis=1)
    F = F + S
    F[cnt <= 1] = 0.0
    return F


# ------------------------------------------------------------------------------------------------ 5. correspondences
def nn_f32(fa, fb, chunk=512):
    """Exact fp32 nearest neighbour of every row of fa among the rows of fb: 33 sequential squared-difference terms, ties -> lower index."""
    fa, fb = np.asarray(fa, np.float32), np.asarray(fb, np.float32)
    out = np.full(len(fa), -1, np.int32)
    if len(fb) == 0:
        return out
    for s in range(0, len(fa), chunk):
        a = fa[s:s + chunk]
        d = np.zeros((len(a), len(fb)), np.float32)
        for k in range(fa.shape[1]):
            e = a[:, k, None] - fb[None, :, k]
            d = d + e * e
        out[s:s + chunk] = np.argmin(d, 1)
    return out


def mutual(nn_st, nn_ts):
    i = np.flatnonzero((nn_st >= 0) & (nn_ts[np.maximum(nn_st, 0)] == np.arange(len(nn_st)))) if len(nn_ts) else np.zeros(0, np.int64)
    return np.stack([i, nn_st[i]], 1).astype(np.int32)


def splitmix(x):
    x = np.asarray(x, np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def tuple_draw(seed, t, k, ncorr):
    """Index of the k-th correspondence of trial t: splitmix64(seed * 0x9E3779B97F4A7C15 + 3 t + k) mod ncorr (all mod 2^64)."""
    base = np.uint64((int(seed) * 0x9E3779B97F4A7C15) & M64)
    with np.errstate(over="ignore"):
        x = base + np.asarray(t, np.uint64) * np.uint64(3) + np.uint64(k)
    return (splitmix(x) % np.uint64(ncorr)).astype(np.int64)


def _norm_rows(a):
    return np.sqrt(_dot(a, a))


def tuples(ps, pt, corr, seed=0, scale=TUPLE_SCALE, max_tuples=MAX_TUPLES):
    """Trials t = 0 .. 100 * ncorr - 1; the first `max_tuples` accepted in trial order -> [ntup, 3] indices into corr."""
    nc = len(corr)
    if nc < 3:
        return np.zeros((0, 3), np.int64)
    out = []
    for t0 in range(0, 100 * nc, 65536):
        t = np.arange(t0, min(t0 + 65536, 100 * nc), dtype=np.int64)
        r = [tuple_draw(seed, t, k, nc) for k in range(3)]
        a = [corr[rk, 0] for rk in r]
        b = [corr[rk, 1] for rk in r]
        li = [_norm_rows(ps[a[0]] - ps[a[1]]), _norm_rows(ps[a[1]] - ps[a[2]]), _norm_rows(ps[a[2]] - ps[a[0]])]
        lj = [_norm_rows(pt[b[0]] - pt[b[1]]), _norm_rows(pt[b[1]] - pt[b[2]]), _norm_rows(pt[b[2]] - pt[b[0]])]
        ok = np.ones(len(t), bool)
        for x, y in zip(li, lj):
            ok &= (x * scale < y) & (y < x / scale)
        out.append(np.stack(r, 1)[ok])
        if sum(len(o) for o in out) >= max_tuples:
            break
    return np.concatenate(out)[:max_tuples]


# ------------------------------------------------------------------------------------------------ 6. FGR optimisation
def rot_zyx(x):
    """Rz(x[2]) Ry(x[1]) Rx(x[0]) (Open3D's TransformVector6dToMatrix4d)."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ (Ry @ Rx)


def cholesky_solve(A, b):
    """A x = b for the 6x6 normal equations; a non-positive pivot -> x = 0 (no update)."""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if not s > 0:
            return np.zeros(n)
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - sum(L[i, k] * y[k] for k in range(i))) / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = (y[i] - sum(L[k, i] * x[k] for k in range(i + 1, n))) / L[i, i]
    return x


def optimize(ps, pt, cs, ct):
    """Both clouds centred on their means and divided by the largest centred norm of either (use_absolute_scale = false); 64
    Gauss-Newton steps moving the target onto the source with Geman-McClure weights (par / (|r|^2 + par))^2, par = 1 divided by 1.4
    every 4th step while par > 0.075 -> T [4,4] with T p_src ~ p_tgt in the input units."""
    ms, mt = ps.mean(0), pt.mean(0)
    scale = max(_norm_rows(ps - ms).max(), _norm_rows(pt - mt).max())
    P = (ps[cs] - ms) / scale
    Q0 = (pt[ct] - mt) / scale
    R, t = np.eye(3), np.zeros(3)
    par = 1.0
    for itr in range(ITERATIONS):
        if itr % 4 == 0 and par > MAX_CORR:
            par /= DIVISION_FACTOR
        Q = Q0 @ R.T + t
        r = P - Q
        s = (par / (_dot(r, r) + par)) ** 2
        z = np.zeros(len(Q))
        o = np.ones(len(Q))
        J = np.stack([np.stack([z, -Q[:, 2], Q[:, 1], -o, z, z], 1), np.stack([Q[:, 2], z, -Q[:, 0], z, -o, z], 1),
                      np.stack([-Q[:, 1], Q[:, 0], z, z, z, -o], 1)], 1)              # [m, 3 (x,y,z residual), 6]
        JTJ = np.einsum("m,mri,mrj->ij", s, J, J)
        JTr = np.einsum("m,mri,mr->i", s, J, r)
        x = -cholesky_solve(JTJ, JTr)
        dR = rot_zyx(x)
        R, t = dR @ R, dR @ t + x[3:]
    tt = -R @ mt + t * scale + ms              # target -> source in the input units
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -R.T @ tt
    return T


# ------------------------------------------------------------------------------------------------ the whole pipeline
def features(pts, origin=(0.0, 0.0, 0.0)):
    idx, d2, cnt = neighbors(pts)
    nrm = normals(pts, idx, d2, cnt, origin)
    return {"idx": idx, "d2": d2, "cnt": cnt, "normal": nrm, "fpfh": fpfh(pts, nrm, idx, d2, cnt)}


def register(pc_src, pc_tgt, seed=0, max_points=MAX_POINTS):
    """numpy [P,3] x 2 (valid points only) -> dict: pose [4,4], status and every stage."""
    out = {"pose": np.eye(4), "status": STATUS_OK}
    ds, _, _ = voxel_down(pc_src)
    dt, _, _ = voxel_down(pc_tgt)
    out.update(down_src=ds, down_tgt=dt)
    if len(ds) > max_points or len(dt) > max_points:
        out["status"] = STATUS_OVERFLOW
        return out
    if len(ds) < 3 or len(dt) < 3:
        out["status"] = STATUS_FEW_POINTS
        return out
    fs, ft = features(ds), features(dt)
    out.update(feat_src=fs, feat_tgt=ft)
    nn_st = nn_f32(fs["fpfh"].astype(np.float32), ft["fpfh"].astype(np.float32))
    nn_ts = nn_f32(ft["fpfh"].astype(np.float32), fs["fpfh"].astype(np.float32))
    corr = mutual(nn_st, nn_ts)
    tup = tuples(ds, dt, corr, seed)
    tc = corr[tup.reshape(-1)] if len(tup) else np.zeros((0, 2), np.int32)
    out.update(nn_st=nn_st, nn_ts=nn_ts, corr=corr, tuples=tup, tuple_corr=tc)
    if len(corr) < 3 or len(tc) < MIN_CORR:
        out["status"] = STATUS_FEW_CORR
        return out
    out["pose"] = optimize(ds, dt, tc[:, 0], tc[:, 1])
    return out
