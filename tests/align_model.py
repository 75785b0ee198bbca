"""The contract of relpose_tsdf_align (include/relpose.h) in numpy: float64 geometry with every operation rounded on its
own, rows quantised to integers, integer sums, and a step made of + - * / sqrt only.  Test infrastructure, not product code: the GPU tests
demand that the kernels reproduce the integer sums and the stepped poses here bit for bit.  The per-point rule is stated twice, vectorised
(what the tests compare the GPU with) and as plain loops over Python floats (the check of the vectorised form); the per-view step is scalar
by nature and stated once, in Python floats."""
import math

import numpy as np

FIX = 32768.0                       # tsdf_sum counts t in 1 / 32768 (relpose_tsdf_fuse)
SCALE_ROT = 256.0                   # the rotation block of a row, l x g, is summed in 1 / 2^8
SCALE_TRANS = 65536.0               # the translation block, g, in 1 / 2^16
SCALE_RES = 65536.0                 # the residual r in 1 / 2^16
SWEEPS = 8                          # cyclic Jacobi sweeps of the 6 x 6
NSUM = 32                           # 21 JtJ (upper triangle, row-major) + 6 Jtr + r^2 + outside, unknown, saturated, used
OUTSIDE, UNKNOWN, SATURATED, USED = 28, 29, 30, 31
MAX_ITERS, MAX_DIM, MAX_POINTS = 64, 2048, 1 << 22
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]
ROW_SCALE = np.array([SCALE_ROT] * 3 + [SCALE_TRANS] * 3)


def face_index(dataset, slot):
    return slot if "suncg" in dataset else (slot + 3) & 3


def _face_rot(k, x, y, z):
    """Rs[k] v: an exact signed permutation (csrc/skybox.h rp_face_rot)"""
    k &= 3
    if k == 0:
        return x, y, z
    if k == 1:
        return -z, y, x
    if k == 2:
        return -x, y, -z
    return z, y, -x


def depth_ok(z):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


def unproject(depth, dataset, stride=1):
    """depth [h,4h] f32 -> (p [N,3] f64 camera-frame points, pix [N] i64): every stride-th pixel in row-major order whose depth is data.
    Pixel (py, px) of slot s has xn = (2 px) / h - 1, yn = 1 - (2 py) / h: the centre rp_skybox_project rounds to."""
    depth = np.asarray(depth, np.float32)
    h = depth.shape[0]
    pix = np.arange(0, 4 * h * h, int(stride), dtype=np.int64)
    D32 = depth.reshape(-1)[pix]
    ok = depth_ok(D32)
    pix, D = pix[ok], D32[ok].astype(np.float64)
    row, col = pix // (4 * h), pix % (4 * h)
    slot, px = col // h, col % h
    xn = (2.0 * px.astype(np.float64)) / float(h) - 1.0
    yn = 1.0 - (2.0 * row.astype(np.float64)) / float(h)
    fx, fy, fz = xn * D, yn * D, -D
    p = np.zeros((len(pix), 3))
    for s in range(4):
        m = slot == s
        x, y, z = _face_rot(face_index(dataset, s), fx[m], fy[m], fz[m])
        p[m, 0], p[m, 1], p[m, 2] = x, y, z
    return p, pix


def inverse(T):
    """world -> camera T 4x4 -> camera -> world W [3,4]: W_ab = T_ba, W_a3 = -((T_0a t0 + T_1a t1) + T_2a t2)"""
    T = np.asarray(T, np.float64)
    W = np.zeros((3, 4))
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                W[a, b] = T[b, a]
            W[a, 3] = -((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3])
    return W


def centre(origin, dims, voxel):
    return np.array([float(origin[a]) + (float(dims[a]) * 0.5) * float(voxel) for a in range(3)])


def _llrint(x):
    return np.rint(x).astype(np.int64)


def accumulate(p, T, tsdf_sum, weight, origin, voxel, min_weight=1, exact=False):
    """p [N,3] camera points, T 4x4 world -> camera, tsdf_sum / weight i32 [nz,ny,nx] -> sums i64 [32].
    exact=True: also (A [6,6], b [6], r2, n) of the unquantised float64 rows (test 7's reference; summed by numpy, not part of the contract)."""
    nz, ny, nx = tsdf_sum.shape
    dims = (nx, ny, nz)
    W = inverse(T)
    vx = np.float64(voxel)
    c = centre(origin, dims, voxel)
    sums = np.zeros(NSUM, np.int64)
    with np.errstate(all="ignore"):
        q = np.stack([((W[a, 0] * p[:, 0] + W[a, 1] * p[:, 1]) + W[a, 2] * p[:, 2]) + W[a, 3] for a in range(3)], 1)
        u = np.stack([(q[:, a] - float(origin[a])) / vx - 0.5 for a in range(3)], 1)
        fl = np.floor(u)
        inside = np.isfinite(q).all(1)
        for a in range(3):
            inside &= (fl[:, a] >= 0) & (fl[:, a] <= dims[a] - 2)
    sums[OUTSIDE] = int((~inside).sum())
    q, u, fl = q[inside], u[inside], fl[inside]
    f = u - fl
    i0 = fl.astype(np.int64)
    tf, wf = tsdf_sum.reshape(-1), weight.reshape(-1)
    t = np.zeros((len(q), 8))
    known = np.ones(len(q), bool)
    for cn in range(8):
        lin = ((i0[:, 2] + (cn >> 2 & 1)) * ny + (i0[:, 1] + (cn >> 1 & 1))) * nx + (i0[:, 0] + (cn & 1))
        w = wf[lin]
        k = w >= min_weight
        known &= k
        t[:, cn] = np.where(k, tf[lin].astype(np.float64) / (FIX * np.where(k, w, 1).astype(np.float64)), 0.0)
    sums[UNKNOWN] = int((~known).sum())
    sat = known & (np.abs(t) >= 1.0).any(1)
    sums[SATURATED] = int(sat.sum())
    use = known & ~sat
    sums[USED] = int(use.sum())
    t, f, q = t[use], f[use], q[use]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    d00, d10, d01, d11 = t[:, 1] - t[:, 0], t[:, 3] - t[:, 2], t[:, 5] - t[:, 4], t[:, 7] - t[:, 6]
    a00, a10, a01, a11 = t[:, 0] + fx * d00, t[:, 2] + fx * d10, t[:, 4] + fx * d01, t[:, 6] + fx * d11
    c0, c1 = a10 - a00, a11 - a01
    b0, b1 = a00 + fy * c0, a01 + fy * c1
    gz = b1 - b0
    r = b0 + fz * gz
    gy = c0 + fz * (c1 - c0)
    e0, e1 = d00 + fy * (d10 - d00), d01 + fy * (d11 - d01)
    gx = e0 + fz * (e1 - e0)
    l = [(q[:, a] - c[a]) / vx for a in range(3)]
    J = np.stack([l[1] * gz - l[2] * gy, l[2] * gx - l[0] * gz, l[0] * gy - l[1] * gx, gx, gy, gz], 1)
    Jq = _llrint(J * ROW_SCALE[None])
    rq = _llrint(r * SCALE_RES)
    for n, (i, j) in enumerate(PAIRS):
        sums[n] = int((Jq[:, i] * Jq[:, j]).sum())
    for i in range(6):
        sums[21 + i] = int((Jq[:, i] * rq).sum())
    sums[27] = int((rq * rq).sum())
    if exact:
        return sums, (J.T @ J, J.T @ r, float(r @ r), len(r))
    return sums


def accumulate_loops(p, T, tsdf_sum, weight, origin, voxel, min_weight=1):
    """accumulate() with one Python-float statement per operation of the rule (its check)"""
    nz, ny, nx = tsdf_sum.shape
    dims = (nx, ny, nz)
    T = [[float(x) for x in row] for row in np.asarray(T, np.float64)]
    W = [[T[b][a] for b in range(3)] + [_neg_dot(T, a)] for a in range(3)]
    o = [float(v) for v in origin]
    voxel = float(voxel)
    c = [o[a] + (float(dims[a]) * 0.5) * voxel for a in range(3)]
    sums = [0] * NSUM
    for x, y, z in np.asarray(p, np.float64).tolist():
        q = [_f(lambda: ((W[a][0] * x + W[a][1] * y) + W[a][2] * z) + W[a][3]) for a in range(3)]
        if not all(math.isfinite(v) for v in q):
            sums[OUTSIDE] += 1
            continue
        u = [(q[a] - o[a]) / voxel - 0.5 for a in range(3)]
        fl = [math.floor(v) for v in u]
        if not all(0 <= fl[a] <= dims[a] - 2 for a in range(3)):
            sums[OUTSIDE] += 1
            continue
        f = [u[a] - float(fl[a]) for a in range(3)]
        t, known = [], True
        for cn in range(8):
            i, j, k = fl[0] + (cn & 1), fl[1] + (cn >> 1 & 1), fl[2] + (cn >> 2 & 1)
            w = int(weight[k, j, i])
            if w < min_weight:
                known = False
                break
            t.append(float(tsdf_sum[k, j, i]) / (FIX * float(w)))
        if not known:
            sums[UNKNOWN] += 1
            continue
        if any(abs(v) >= 1.0 for v in t):
            sums[SATURATED] += 1
            continue
        sums[USED] += 1
        d00, d10, d01, d11 = t[1] - t[0], t[3] - t[2], t[5] - t[4], t[7] - t[6]
        a00, a10, a01, a11 = t[0] + f[0] * d00, t[2] + f[0] * d10, t[4] + f[0] * d01, t[6] + f[0] * d11
        c0, c1 = a10 - a00, a11 - a01
        b0, b1 = a00 + f[1] * c0, a01 + f[1] * c1
        gz = b1 - b0
        r = b0 + f[2] * gz
        gy = c0 + f[2] * (c1 - c0)
        e0, e1 = d00 + f[1] * (d10 - d00), d01 + f[1] * (d11 - d01)
        gx = e0 + f[2] * (e1 - e0)
        l = [(q[a] - c[a]) / voxel for a in range(3)]
        J = [l[1] * gz - l[2] * gy, l[2] * gx - l[0] * gz, l[0] * gy - l[1] * gx, gx, gy, gz]
        Jq = [int(np.rint(J[i] * float(ROW_SCALE[i]))) for i in range(6)]
        rq = int(np.rint(r * SCALE_RES))
        for n, (i, j) in enumerate(PAIRS):
            sums[n] += Jq[i] * Jq[j]
        for i in range(6):
            sums[21 + i] += Jq[i] * rq
        sums[27] += rq * rq
    return np.array(sums, np.int64)


def _f(fn):
    try:
        return fn()
    except OverflowError:
        return float("inf")


def _neg_dot(T, a):
    return -((T[0][a] * T[0][3] + T[1][a] * T[1][3]) + T[2][a] * T[2][3])


# ---------------------------------------------------------------------------------------------- the step (Python floats)
def normal_equations(sums):
    """integer sums -> (A 6x6 list of lists, b [6]) in float64: one rounding int64 -> double (exact below 2^53), then exact power-of-two scales"""
    A = [[0.0] * 6 for _ in range(6)]
    for n, (i, j) in enumerate(PAIRS):
        A[i][j] = A[j][i] = float(int(sums[n])) / (float(ROW_SCALE[i]) * float(ROW_SCALE[j]))
    b = [float(int(sums[21 + i])) / (float(ROW_SCALE[i]) * SCALE_RES) for i in range(6)]
    return A, b


def jacobi(A):
    """cyclic Jacobi, SWEEPS sweeps over (p, q), p < q, row-major -> (lam [6] = the diagonal, V: column k is the k-th vector)"""
    A = [row[:] for row in A]
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    for _ in range(SWEEPS):
        for p in range(5):
            for q in range(p + 1, 6):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                tt = theta * theta
                den = abs(theta) + math.sqrt(tt + 1.0)
                t = (1.0 / den) if theta >= 0.0 else -(1.0 / den)
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = 0.0
                for k in range(6):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                for k in range(6):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[k][k] for k in range(6)], V


def step(sums, T, origin, dims, voxel, eig_min):
    """One view's step -> {"pose": the new world -> camera pose (T itself, bit for bit, when fewer than 6 points were used), "eig" [6]
    ascending (lambda / n_used; 0 without a used point), "held", "coef" [6] and "vec" (the step's coefficient per Jacobi column and the
    columns: a held column's coefficient is exactly 0), "delta" [6] (rotation vector, translation in voxels)}"""
    T = np.asarray(T, np.float64)
    n = int(sums[USED])
    A, b = normal_equations(sums)
    lam, V = jacobi(A)
    nn = float(n)
    eig = sorted((lam[k] / nn) if n > 0 else 0.0 for k in range(6))
    floor = float(eig_min) * nn
    coef = [0.0] * 6
    held = 0
    for k in range(6):
        if n >= 6 and lam[k] > floor:
            vb = 0.0
            for i in range(6):
                vb = vb + V[i][k] * b[i]
            coef[k] = -(vb / lam[k])
        else:
            held += 1
    delta = [0.0] * 6
    for k in range(6):
        for i in range(6):
            delta[i] = delta[i] + V[i][k] * coef[k]
    out = {"eig": np.array(eig), "held": held, "coef": np.array(coef), "vec": np.array(V), "delta": np.array(delta), "lam": np.array(lam)}
    if n < 6:
        out["pose"] = T.copy()
        return out
    out["pose"] = apply_delta(T, delta, origin, dims, voxel)
    return out


def apply_delta(T, delta, origin, dims, voxel):
    """T' = T D^-1 with D the world-frame motion x -> c + Rd (x - c) + voxel tau; Rd is the Cayley rotation of the vector delta[:3]:
    a = w / 2, Rd = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)"""
    T = [[float(x) for x in row] for row in np.asarray(T, np.float64)]
    voxel = float(voxel)
    c = [float(origin[a]) + (float(dims[a]) * 0.5) * voxel for a in range(3)]
    a = [delta[0] * 0.5, delta[1] * 0.5, delta[2] * 0.5]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den = 1.0 + aa
    om = 1.0 - aa
    Rd = [[0.0] * 3 for _ in range(3)]
    Rd[0][0] = (om + 2.0 * (a[0] * a[0])) / den
    Rd[1][1] = (om + 2.0 * (a[1] * a[1])) / den
    Rd[2][2] = (om + 2.0 * (a[2] * a[2])) / den
    Rd[0][1] = (2.0 * (a[0] * a[1] - a[2])) / den
    Rd[1][0] = (2.0 * (a[0] * a[1] + a[2])) / den
    Rd[0][2] = (2.0 * (a[0] * a[2] + a[1])) / den
    Rd[2][0] = (2.0 * (a[0] * a[2] - a[1])) / den
    Rd[1][2] = (2.0 * (a[1] * a[2] - a[0])) / den
    Rd[2][1] = (2.0 * (a[1] * a[2] + a[0])) / den
    # d = (c - Rd c) + voxel tau
    d = [(c[i] - ((Rd[i][0] * c[0] + Rd[i][1] * c[1]) + Rd[i][2] * c[2])) + voxel * delta[3 + i] for i in range(3)]
    out = np.array(T)
    for i in range(3):
        n = [(T[i][0] * Rd[j][0] + T[i][1] * Rd[j][1]) + T[i][2] * Rd[j][2] for j in range(3)]        # (R_T Rd^T)_ij
        out[i, 0], out[i, 1], out[i, 2] = n
        out[i, 3] = T[i][3] - ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2])
    return out


def rms(sums):
    n = int(sums[USED])
    return math.sqrt(float(int(sums[27])) / float(n)) / SCALE_RES if n > 0 else 0.0


def align(state, origin, voxel, depth, pose, dataset, scene_of_view=None, iters=12, eig_min=0.0, stride=1, min_weight=1, loops=False):
    """state {"tsdf_sum", "weight"} [S,nz,ny,nx], origin [S,3], depth [V,h,4h], pose [V,4,4] world -> camera.  iters + 1 evaluations: every
    one but the last is followed by a step; the outputs describe the last.
    -> {"pose" [V,4,4], "eig" [V,6], "held" [V] i32, "sums" [V,32] i64, "rms" [V,2], "trace_pose" [V,iters+1,4,4], "trace_sums" [V,iters+1,32],
        "steps": per view the list of step() dicts}"""
    V = len(depth)
    S, nz, ny, nx = state["tsdf_sum"].shape
    sov = np.zeros(V, np.int64) if scene_of_view is None else np.asarray(scene_of_view)
    origin = np.asarray(origin, np.float64).reshape(S, 3)
    out = {"pose": np.zeros((V, 4, 4)), "eig": np.zeros((V, 6)), "held": np.zeros(V, np.int32), "sums": np.zeros((V, NSUM), np.int64),
           "rms": np.zeros((V, 2)), "trace_pose": np.zeros((V, iters + 1, 4, 4)), "trace_sums": np.zeros((V, iters + 1, NSUM), np.int64),
           "steps": []}
    acc = accumulate_loops if loops else accumulate
    for v in range(V):
        s = int(sov[v])
        p, _ = unproject(depth[v], dataset, stride)
        T = np.array(pose[v], np.float64)
        steps = []
        for e in range(iters + 1):
            sums = acc(p, T, state["tsdf_sum"][s], state["weight"][s], origin[s], voxel, min_weight)
            out["trace_pose"][v, e], out["trace_sums"][v, e] = T, sums
            st = step(sums, T, origin[s], (nx, ny, nz), voxel, eig_min)
            steps.append(st)
            if e == 0:
                out["rms"][v, 0] = rms(sums)
            if e < iters:
                T = st["pose"]
        out["pose"][v], out["eig"][v], out["held"][v], out["sums"][v] = T, st["eig"], st["held"], sums
        out["rms"][v, 1] = rms(sums)
        out["steps"].append(steps)
    return out
