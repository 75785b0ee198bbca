"""The pose-graph synchronisation contract of relpose_pose_sync (include/relpose.h) in numpy, twice: `sync_scene` works on
whole arrays, `sync_scene_loops` states the same operations as plain loops over scalars.  Both round every float64 operation on its own and
add in the same order, so they agree bit for bit (tests/test_sync_cpu.py); sin and atan2 are numpy's in both.

A scene has M views and E edges.  Edge e carries src, dst (view indices), T (4x4, T ~ X_dst inv(X_src) for world -> camera poses X) and a
prior weight w0.  State per view: R_v (3x3) and u_v = R_v^T t_v; the pose written out is [R_v | R_v u_v]."""
import numpy as np

MAX_VIEWS, MAX_EDGES, MAX_ITERATIONS = 64, 4096, 100000
USED, BAD_INDEX, SELF_EDGE, BAD_WEIGHT, BAD_POSE = 0, 1, 2, 3, 4
LOG_SMALL = 1e-6            # |v| below it: the fallbacks of so3 log
EXP_SMALL = 1e-8            # |d|^2 below it: the series of so3 exp
DEFAULTS = dict(sigma_r=0.1, sigma_t=0.1, mu0=64.0, div=1.4, n_final=10, robust=True)


def schedule(mu0=64.0, div=1.4, n_final=10):
    """The mu of every iteration: mu0, then mu / div (a float64 division, repeated) with a floor of 1; n_final iterations at 1."""
    mus, mu = [], float(mu0)
    while mu > 1.0:
        mus.append(mu)
        mu = max(mu / float(div), 1.0)
        if len(mus) > MAX_ITERATIONS:
            raise ValueError("more than MAX_ITERATIONS iterations")
    return mus + [1.0] * int(n_final)


def edge_states(M, src, dst, T, w0):
    src, dst, w0 = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w0, np.float64)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    st = np.zeros(len(src), np.int32)
    bad_idx = (src < 0) | (src >= M) | (dst < 0) | (dst >= M)
    with np.errstate(invalid="ignore"):
        bad_w = ~(np.isfinite(w0) & (w0 > 0))
    bad_T = ~np.isfinite(T[:, :3, :]).all((1, 2))
    for code, m in ((BAD_POSE, bad_T), (BAD_WEIGHT, bad_w), (SELF_EDGE, src == dst), (BAD_INDEX, bad_idx)):      # the first that applies wins
        st[m] = code
    return st


# ------------------------------------------------------------------------------------------------------------- whole arrays
def mm(A, B):
    """A B for [..., 3, 3]: (a0 b0 + a1 b1) + a2 b2 per entry."""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def mtm(A, B):
    """A^T B for [..., 3, 3]."""
    return (A[..., 0, :, None] * B[..., None, 0, :] + A[..., 1, :, None] * B[..., None, 1, :]) + A[..., 2, :, None] * B[..., None, 2, :]


def mtv(A, t):
    """A^T t for [..., 3, 3] and [..., 3]."""
    return (A[..., 0, :] * t[..., 0, None] + A[..., 1, :] * t[..., 1, None]) + A[..., 2, :] * t[..., 2, None]


def mv(A, t):
    return (A[..., :, 0] * t[..., 0, None] + A[..., :, 1] * t[..., 1, None]) + A[..., :, 2] * t[..., 2, None]


def so3_log(E):
    """[N,3,3] -> [N,3].  v = the antisymmetric part (2 sin(th) axis), th = atan2(|v| / 2, (tr - 1) / 2), w = v * (th / |v|).  |v| < 1e-6 and
    cos > 0: w = v / 2.  |v| < 1e-6 and cos <= 0 (near pi): the axis from the symmetric part, a_k = sqrt((E_kk - c) / (1 - c)) at the first
    largest diagonal entry k, a_m = (E_km + E_mk) / ((2 (1 - c)) a_k), signed so that a . v >= 0."""
    v = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    c = (((E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]) - 1.0) * 0.5
    th = np.arctan2(n * 0.5, c)
    with np.errstate(all="ignore"):
        out = v * (th / n)[:, None]
        small = n < LOG_SMALL
        out = np.where((small & (c > 0))[:, None], v * 0.5, out)
        near_pi = small & ~(c > 0)
        if near_pi.any():
            idx = np.nonzero(near_pi)[0]
            for e in idx:
                out[e] = _log_near_pi([[float(E[e, a, b]) for b in range(3)] for a in range(3)], [float(x) for x in v[e]], float(c[e]), float(th[e]))
    return out


def _log_near_pi(E, v, c, th):
    k = 0
    for m in (1, 2):
        if E[m][m] > E[k][k]:
            k = m
    om = 1.0 - c
    a = [0.0, 0.0, 0.0]
    a[k] = float(np.sqrt(max((E[k][k] - c) / om, 0.0)))
    for m in range(3):
        if m != k:
            a[m] = (E[k][m] + E[m][k]) / ((2.0 * om) * a[k])
    sg = -1.0 if ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]) < 0 else 1.0
    ths = th * sg
    return [ths * a[0], ths * a[1], ths * a[2]]


def so3_exp(d):
    """[N,3] -> [N,3,3]: I + A K + B K^2 with A = sin(th) / th, B = 2 sin(th / 2)^2 / th^2; th^2 < 1e-8: A = 1 - th^2 / 6, B = 0.5 - th^2 / 24."""
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    t2 = (d0 * d0 + d1 * d1) + d2 * d2
    th = np.sqrt(t2)
    with np.errstate(all="ignore"):
        sh = np.sin(th * 0.5)
        A = np.where(t2 < EXP_SMALL, 1.0 - t2 / 6.0, np.sin(th) / th)
        B = np.where(t2 < EXP_SMALL, 0.5 - t2 / 24.0, (2.0 * (sh * sh)) / t2)
    X = np.empty((len(d), 3, 3))
    X[:, 0, 0] = 1.0 - B * (d1 * d1 + d2 * d2)
    X[:, 0, 1] = B * (d0 * d1) - A * d2
    X[:, 0, 2] = B * (d0 * d2) + A * d1
    X[:, 1, 0] = B * (d0 * d1) + A * d2
    X[:, 1, 1] = 1.0 - B * (d0 * d0 + d2 * d2)
    X[:, 1, 2] = B * (d1 * d2) - A * d0
    X[:, 2, 0] = B * (d0 * d2) - A * d1
    X[:, 2, 1] = B * (d1 * d2) + A * d0
    X[:, 2, 2] = 1.0 - B * (d0 * d0 + d1 * d1)
    return X


def norm2(x):
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]


def cholesky_solve(L, rhs):
    """Right-looking Cholesky of the symmetric L [M,M] (lower triangle read), then the forward and the backward substitution of rhs [M,K],
    column by column: y_i = ((b_i - l_i0 x_0) - l_i1 x_1) - ..."""
    L = L.copy()
    M = len(L)
    dg = np.zeros(M)
    with np.errstate(all="ignore"):
        for k in range(M):
            dg[k] = np.sqrt(L[k, k])
            L[k + 1:, k] = L[k + 1:, k] / dg[k]
            col = L[k + 1:, k]
            n = M - k - 1
            upd = L[k + 1:, k + 1:] - col[:, None] * col[None, :]
            L[k + 1:, k + 1:] = np.where(np.tril(np.ones((n, n), bool)), upd, L[k + 1:, k + 1:])
        x = rhs.copy()
        for k in range(M):
            x[k] = x[k] / dg[k]
            x[k + 1:] = x[k + 1:] - L[k + 1:, k, None] * x[k][None]
        for k in range(M - 1, -1, -1):
            x[k] = x[k] / dg[k]
            x[:k] = x[:k] - L[k, :k, None] * x[k][None]
    return x


def prim(M, src, dst, w0, used):
    """Components and the maximum-weight spanning forest: M steps; each adds the used edge of largest w0 (ties: the smaller index) that joins a
    visited and an unvisited view, or, where none does, starts a component at the smallest unvisited view.  -> component, tree, order: the
    steps as (view, edge or -1, the edge's other end or -1)."""
    vis = np.zeros(M, bool)
    comp = np.zeros(M, np.int32)
    tree = np.zeros(len(src), np.int32)
    order = []
    s, d = np.clip(src, 0, max(M - 1, 0)), np.clip(dst, 0, max(M - 1, 0))
    for _ in range(M):
        cand = used & (vis[s] != vis[d]) if len(src) else np.zeros(0, bool)
        if cand.any():
            e = int(np.argmax(np.where(cand, w0, -np.inf)))
            new, old = (int(d[e]), int(s[e])) if vis[s[e]] else (int(s[e]), int(d[e]))
            comp[new] = comp[old]
            tree[e] = 1
            order.append((new, e, old))
        else:
            new = int(np.argmin(vis))
            comp[new] = new
            order.append((new, -1, -1))
        vis[new] = True
    return comp, tree, order


def adjacency(M, src, dst, used):
    """Per view, its used edges in ascending edge index: entry arrays (view, edge, other end, sign: +1 where the view is the edge's dst)."""
    e = np.nonzero(used)[0]
    view = np.concatenate([src[e], dst[e]])
    edge = np.concatenate([e, e])
    other = np.concatenate([dst[e], src[e]])
    sign = np.concatenate([-np.ones(len(e)), np.ones(len(e))])
    o = np.lexsort((edge, view))
    return view[o], edge[o], other[o], sign[o]


def sync_scene(M, src, dst, T, w0, sigma_r=0.1, sigma_t=0.1, mu0=64.0, div=1.4, n_final=10, robust=True):
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    w0 = np.asarray(w0, np.float64).reshape(-1)
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    E = len(src)
    state = edge_states(M, src, dst, T, w0)
    used = state == USED
    comp, tree, order = prim(M, src, dst, w0, used)
    R = np.zeros((M, 3, 3))
    u = np.zeros((M, 3))
    for new, e, old in order:
        if e < 0:
            R[new] = np.eye(3)
        elif new == dst[e]:
            R[new] = mm(T[e, :3, :3], R[old])
            u[new] = u[old] + mtv(R[new], T[e, :3, 3])
        else:
            R[new] = mtm(T[e, :3, :3], R[old])
            u[new] = u[old] - mtv(R[old], T[e, :3, 3])
    gauge = comp == np.arange(M)
    ue = np.nonzero(used)[0]
    si, di = src[ue], dst[ue]
    Rij, tij, w0u = T[ue, :3, :3], T[ue, :3, 3], w0[ue]
    av, ae, ao, asg = adjacency(M, src, dst, used)
    pos = np.full(E, -1)
    pos[ue] = np.arange(len(ue))
    ap = pos[ae]                                                    # the entries' edges as indices into the used edges
    free = ~gauge[av] & ~gauge[ao]
    sr2, st2 = sigma_r * sigma_r, sigma_t * sigma_t

    def residuals():
        om = so3_log(mtm(R[di], mm(Rij, R[si])))
        rho = mtv(R[di], tij) - (u[di] - u[si])
        return om, rho

    def r2_of(om, rho, mu):
        return (norm2(om) / sr2 + norm2(rho) / st2) / (mu * mu)

    def assemble(vec, w):
        b = np.zeros((M, 3))
        np.add.at(b, av, asg[:, None] * (w[ap, None] * vec[ap]))
        b[gauge] = 0.0
        return b

    conf = np.ones(len(ue))
    last_step = 0.0
    for mu in schedule(mu0, div, n_final):
        om, rho = residuals()
        if robust:
            q = 1.0 + r2_of(om, rho, mu)
            with np.errstate(all="ignore"):
                conf = 1.0 / (q * q)
        w = w0u * conf
        L = np.zeros((M, M))
        diag = np.zeros(M)
        np.add.at(diag, av, w[ap])
        np.add.at(L, (av[free], ao[free]), -w[ap[free]])
        L[np.arange(M), np.arange(M)] = np.where(gauge, 1.0, diag)
        d = cholesky_solve(L, assemble(om, w))
        d[gauge] = 0.0
        R = mm(R, so3_exp(d))
        last_step = float(np.max(np.abs(d))) if M else 0.0
        u = cholesky_solve(L, assemble(mtv(R[di], tij), w))
        u[gauge] = 0.0
    om, rho = residuals()
    out = {"component": comp, "tree": tree, "edge_state": state, "n_components": int(gauge.sum()), "last_step": last_step}
    pose = np.zeros((M, 4, 4))
    pose[:, :3, :3] = R
    pose[:, :3, 3] = mv(R, u)
    pose[:, 3, 3] = 1.0
    out["pose"] = pose
    out["confidence"] = np.zeros(E)
    out["confidence"][ue] = conf
    out["res_rot"] = np.full(E, np.nan)
    out["res_trans"] = np.full(E, np.nan)
    out["res_rot"][ue] = np.sqrt(norm2(om))
    out["res_trans"][ue] = np.sqrt(norm2(rho))
    r2 = r2_of(om, rho, 1.0)
    with np.errstate(all="ignore"):
        term = w0u * (r2 / (1.0 + r2)) if robust else w0u * r2
    # the cost: per view, over its adjacency entries where it is the dst, ascending; then the views in ascending order
    per_view = np.zeros(M)
    isdst = asg > 0
    np.add.at(per_view, av[isdst], term[ap[isdst]])
    cost = 0.0
    for v in range(M):
        cost = cost + float(per_view[v])
    out["cost"] = cost
    return out


# ------------------------------------------------------------------------------------------------------------- plain loops
def _sin(x):
    return float(np.sin(np.float64(x)))


def _atan2(y, x):
    return float(np.arctan2(np.float64(y), np.float64(x)))


def _sqrt(x):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mm(A, B):
    return [[(A[a][0] * B[0][b] + A[a][1] * B[1][b]) + A[a][2] * B[2][b] for b in range(3)] for a in range(3)]


def _mtm(A, B):
    return [[(A[0][a] * B[0][b] + A[1][a] * B[1][b]) + A[2][a] * B[2][b] for b in range(3)] for a in range(3)]


def _mtv(A, t):
    return [(A[0][a] * t[0] + A[1][a] * t[1]) + A[2][a] * t[2] for a in range(3)]


def _log(E):
    v = [E[2][1] - E[1][2], E[0][2] - E[2][0], E[1][0] - E[0][1]]
    n = _sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = (((E[0][0] + E[1][1]) + E[2][2]) - 1.0) * 0.5
    th = _atan2(n * 0.5, c)
    if n < LOG_SMALL:
        if c > 0:
            return [v[0] * 0.5, v[1] * 0.5, v[2] * 0.5]
        return _log_near_pi(E, v, c, th)
    f = _div(th, n)
    return [v[0] * f, v[1] * f, v[2] * f]


def _exp(d):
    d0, d1, d2 = d
    t2 = (d0 * d0 + d1 * d1) + d2 * d2
    if t2 < EXP_SMALL:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        th = _sqrt(t2)
        sh = _sin(th * 0.5)
        A, B = _div(_sin(th), th), _div(2.0 * (sh * sh), t2)
    return [[1.0 - B * (d1 * d1 + d2 * d2), B * (d0 * d1) - A * d2, B * (d0 * d2) + A * d1],
            [B * (d0 * d1) + A * d2, 1.0 - B * (d0 * d0 + d2 * d2), B * (d1 * d2) - A * d0],
            [B * (d0 * d2) - A * d1, B * (d1 * d2) + A * d0, 1.0 - B * (d0 * d0 + d1 * d1)]]


def _solve(L, dg, b):
    """the substitutions of cholesky_solve for one factor and rhs [M][3]"""
    M = len(dg)
    x = [list(r) for r in b]
    for k in range(M):
        for c in range(3):
            x[k][c] = _div(x[k][c], dg[k])
        for i in range(k + 1, M):
            for c in range(3):
                x[i][c] = x[i][c] - L[i][k] * x[k][c]
    for k in range(M - 1, -1, -1):
        for c in range(3):
            x[k][c] = _div(x[k][c], dg[k])
        for i in range(k):
            for c in range(3):
                x[i][c] = x[i][c] - L[k][i] * x[k][c]
    return x


def sync_scene_loops(M, src, dst, T, w0, sigma_r=0.1, sigma_t=0.1, mu0=64.0, div=1.4, n_final=10, robust=True):
    src, dst = [int(v) for v in np.asarray(src).reshape(-1)], [int(v) for v in np.asarray(dst).reshape(-1)]
    w0 = [float(v) for v in np.asarray(w0, np.float64).reshape(-1)]
    T = np.asarray(T, np.float64).reshape(-1, 4, 4).tolist()
    E = len(src)
    state = []
    for e in range(E):
        if src[e] < 0 or src[e] >= M or dst[e] < 0 or dst[e] >= M:
            state.append(BAD_INDEX)
        elif src[e] == dst[e]:
            state.append(SELF_EDGE)
        elif not (np.isfinite(w0[e]) and w0[e] > 0):
            state.append(BAD_WEIGHT)
        elif not all(np.isfinite(T[e][a][b]) for a in range(3) for b in range(4)):
            state.append(BAD_POSE)
        else:
            state.append(USED)
    vis, comp, tree = [False] * M, [0] * M, [0] * E
    R = [None] * M
    u = [[0.0, 0.0, 0.0] for _ in range(M)]
    for _ in range(M):
        best = -1
        for e in range(E):
            if state[e] == USED and vis[src[e]] != vis[dst[e]] and (best < 0 or w0[e] > w0[best]):
                best = e
        if best >= 0:
            e = best
            Rij, t = [T[e][a][:3] for a in range(3)], [T[e][a][3] for a in range(3)]
            if vis[src[e]]:
                new, old = dst[e], src[e]
                R[new] = _mm(Rij, R[old])
                c = _mtv(R[new], t)
                u[new] = [u[old][a] + c[a] for a in range(3)]
            else:
                new, old = src[e], dst[e]
                R[new] = _mtm(Rij, R[old])
                c = _mtv(R[old], t)
                u[new] = [u[old][a] - c[a] for a in range(3)]
            comp[new] = comp[old]
            tree[e] = 1
        else:
            new = vis.index(False)
            comp[new] = new
            R[new] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        vis[new] = True
    adj = [[] for _ in range(M)]
    for e in range(E):
        if state[e] == USED:
            adj[src[e]].append((e, dst[e], False))
            adj[dst[e]].append((e, src[e], True))
    gauge = [comp[v] == v for v in range(M)]
    sr2, st2 = sigma_r * sigma_r, sigma_t * sigma_t

    def residual(e):
        i, j = src[e], dst[e]
        Rij, t = [T[e][a][:3] for a in range(3)], [T[e][a][3] for a in range(3)]
        om = _log(_mtm(R[j], _mm(Rij, R[i])))
        c = _mtv(R[j], t)
        return om, [c[a] - (u[j][a] - u[i][a]) for a in range(3)]

    def r2_of(om, rho, mu):
        a = _div((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2], sr2)
        b = _div((rho[0] * rho[0] + rho[1] * rho[1]) + rho[2] * rho[2], st2)
        return _div(a + b, mu * mu)

    def assemble(vec, w):
        b = [[0.0, 0.0, 0.0] for _ in range(M)]
        for v in range(M):
            if gauge[v]:
                continue
            for e, _, isdst in adj[v]:
                for c in range(3):
                    p = w[e] * vec[e][c]
                    b[v][c] = b[v][c] + p if isdst else b[v][c] - p
        return b

    conf = [1.0 if state[e] == USED else 0.0 for e in range(E)]
    w = [0.0] * E
    last_step = 0.0
    for mu in schedule(mu0, div, n_final):
        om = [None] * E
        for e in range(E):
            if state[e] != USED:
                continue
            om[e], rho = residual(e)
            if robust:
                q = 1.0 + r2_of(om[e], rho, mu)
                conf[e] = _div(1.0, q * q)
            w[e] = w0[e] * conf[e]
        L = [[0.0] * M for _ in range(M)]
        for v in range(M):
            if gauge[v]:
                L[v][v] = 1.0
                continue
            dsum = 0.0
            for e, o, _ in adj[v]:
                dsum = dsum + w[e]
                if not gauge[o]:
                    L[v][o] = L[v][o] - w[e]
            L[v][v] = dsum
        dg = [0.0] * M
        for k in range(M):
            dg[k] = _sqrt(L[k][k])
            for i in range(k + 1, M):
                L[i][k] = _div(L[i][k], dg[k])
            for i in range(k + 1, M):
                for j in range(k + 1, i + 1):
                    L[i][j] = L[i][j] - L[i][k] * L[j][k]
        d = _solve(L, dg, assemble(om, w))
        last_step = 0.0
        for v in range(M):
            if gauge[v]:
                continue
            R[v] = _mm(R[v], _exp(d[v]))
            for c in range(3):
                a = abs(d[v][c])
                if a > last_step or a != a:
                    last_step = a
        cvec = [None] * E
        for e in range(E):
            if state[e] == USED:
                cvec[e] = _mtv(R[dst[e]], [T[e][a][3] for a in range(3)])
        x = _solve(L, dg, assemble(cvec, w))
        for v in range(M):
            u[v] = [0.0, 0.0, 0.0] if gauge[v] else x[v]
    out = {"component": np.array(comp, np.int32).reshape(M), "tree": np.array(tree, np.int32).reshape(E),
           "edge_state": np.array(state, np.int32).reshape(E), "n_components": sum(gauge), "last_step": last_step}
    pose = np.zeros((M, 4, 4))
    for v in range(M):
        for a in range(3):
            pose[v, a, :3] = R[v][a]
            pose[v, a, 3] = (R[v][a][0] * u[v][0] + R[v][a][1] * u[v][1]) + R[v][a][2] * u[v][2]
        pose[v, 3, 3] = 1.0
    out["pose"] = pose
    out["confidence"] = np.array(conf, np.float64).reshape(E)
    rr, rt, term = np.full(E, np.nan), np.full(E, np.nan), [0.0] * E
    for e in range(E):
        if state[e] != USED:
            continue
        om_e, rho = residual(e)
        rr[e] = _sqrt((om_e[0] * om_e[0] + om_e[1] * om_e[1]) + om_e[2] * om_e[2])
        rt[e] = _sqrt((rho[0] * rho[0] + rho[1] * rho[1]) + rho[2] * rho[2])
        r2 = r2_of(om_e, rho, 1.0)
        term[e] = w0[e] * _div(r2, 1.0 + r2) if robust else w0[e] * r2
    cost = 0.0
    for v in range(M):
        pv = 0.0
        for e, _, isdst in adj[v]:
            if isdst:
                pv = pv + term[e]
        cost = cost + pv
    out.update(res_rot=rr, res_trans=rt, cost=cost)
    return out


# ------------------------------------------------------------------------------------------------------------- the batch
KEYS = ("pose", "component", "tree", "edge_state", "confidence", "res_rot", "res_trans", "n_components", "cost", "last_step")


def sync(T, src, dst, w0, view_begin, edge_begin, form=sync_scene, **kw):
    """The batched call: scene s owns the views view_begin[s] .. view_begin[s+1] and the edges edge_begin[s] .. edge_begin[s+1]; src / dst are
    local to the scene.  -> the outputs of relpose_pose_sync as arrays (component is local to the scene too)."""
    vb, eb = np.asarray(view_begin).reshape(-1), np.asarray(edge_begin).reshape(-1)
    S = len(vb) - 1
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    per = [form(int(vb[s + 1] - vb[s]), np.asarray(src)[eb[s]:eb[s + 1]], np.asarray(dst)[eb[s]:eb[s + 1]], T[eb[s]:eb[s + 1]],
                np.asarray(w0)[eb[s]:eb[s + 1]], **kw) for s in range(S)]
    out = {}
    for k in ("pose", "component", "tree", "edge_state", "confidence", "res_rot", "res_trans"):
        out[k] = np.concatenate([p[k] for p in per]) if per else None
    out["n_components"] = np.array([p["n_components"] for p in per], np.int32)
    out["cost"] = np.array([p["cost"] for p in per], np.float64)
    out["last_step"] = np.array([p["last_step"] for p in per], np.float64)
    return out
