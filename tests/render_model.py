"""The contract of relpose_tsdf_render (include/relpose.h) in numpy: float64 geometry with every operation rounded on its
own, + - * / sqrt floor only.  Test infrastructure, not product code: the GPU tests demand that the kernels reproduce every output here bit
for bit.  The rule is stated twice: vectorised over the rays of a view, with the conservative clip and the empty-space skip the kernels use
(what the tests compare the GPU with), and as a plain loop per ray over Python floats, k = 0 .. n_steps - 1, with neither (the definition,
and the check of the vectorised form)."""
import itertools
import math

import numpy as np

import align_model as AM

FIX = AM.FIX                        # tsdf_sum counts t in 1 / 32768 (relpose_tsdf_fuse)
BRICK = 8                           # a brick is 8^3 cells
MAX_STEPS = 65536
MISS, HIT, BACK = 0, 1, 2
KEYS = ("depth", "cls", "normal", "color", "n_evaluated")
IMAGE_KEYS = KEYS[:4]               # what must not depend on skip


def rays(h, dataset):
    """-> dir [4 h h, 3]: the camera-frame direction per unit of face depth of every pixel, row-major: Rs[face(slot)] (xn, yn, -1)"""
    pix = np.arange(4 * h * h, dtype=np.int64)
    row, col = pix // (4 * h), pix % (4 * h)
    slot, px = col // h, col % h
    xn = (2.0 * px.astype(np.float64)) / float(h) - 1.0
    yn = 1.0 - (2.0 * row.astype(np.float64)) / float(h)
    d = np.zeros((len(pix), 3))
    for s in range(4):
        m = slot == s
        x, y, z = AM._face_rot(AM.face_index(dataset, s), xn[m], yn[m], np.full(int(m.sum()), -1.0))
        d[m, 0], d[m, 1], d[m, 2] = x, y, z
    return d


def bricks(n):
    return (n - 1 + BRICK - 1) // BRICK if n > 1 else 0


def brick_flags(tsdf_sum, weight, min_weight=1):
    """-> bool [bz, by, bx]: the brick holds a cell with a corner voxel of weight >= min_weight and tsdf_sum < 0"""
    nz, ny, nx = tsdf_sum.shape
    flags = np.zeros((bricks(nz), bricks(ny), bricks(nx)), bool)
    if flags.size == 0:
        return flags
    neg = (weight >= min_weight) & (tsdf_sum < 0)
    cell = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for dk, dj, di in itertools.product((0, 1), repeat=3):
        cell |= neg[dk:dk + nz - 1, dj:dj + ny - 1, di:di + nx - 1]
    kk, jj, ii = np.nonzero(cell)
    flags[kk // BRICK, jj // BRICK, ii // BRICK] = True
    return flags


def cells(W, dirs, d, origin, voxel, dims, flags=None):
    """the samples at face depth d (a scalar or one per ray) -> (in_range [N], i0 [N,3] i64 (0 where out of range), f [N,3], flagged [N])"""
    vx = np.float64(voxel)
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        x, y, z = d * dirs[:, 0], d * dirs[:, 1], d * dirs[:, 2]
        inr = np.ones(len(dirs), bool)
        fl, f = np.zeros((len(dirs), 3)), np.zeros((len(dirs), 3))
        for a in range(3):
            q = ((W[a, 0] * x + W[a, 1] * y) + W[a, 2] * z) + W[a, 3]
            u = (q - float(origin[a])) / vx - 0.5
            fl[:, a] = np.floor(u)
            inr &= np.isfinite(q) & (fl[:, a] >= 0) & (fl[:, a] <= dims[a] - 2)
            f[:, a] = u - fl[:, a]
    i0 = np.where(inr[:, None], fl, 0.0).astype(np.int64)
    flagged = np.zeros(len(dirs), bool)
    if flags is not None and flags.size:
        flagged = inr & flags[i0[:, 2] // BRICK, i0[:, 1] // BRICK, i0[:, 0] // BRICK]
    return inr, i0, f, flagged


def _lerp8(t, f, grad=False):
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    d00, d10, d01, d11 = t[:, 1] - t[:, 0], t[:, 3] - t[:, 2], t[:, 5] - t[:, 4], t[:, 7] - t[:, 6]
    a00, a10, a01, a11 = t[:, 0] + fx * d00, t[:, 2] + fx * d10, t[:, 4] + fx * d01, t[:, 6] + fx * d11
    c0, c1 = a10 - a00, a11 - a01
    b0, b1 = a00 + fy * c0, a01 + fy * c1
    gz = b1 - b0
    r = b0 + fz * gz
    if not grad:
        return r
    gy = c0 + fz * (c1 - c0)
    e0, e1 = d00 + fy * (d10 - d00), d01 + fy * (d11 - d01)
    gx = e0 + fz * (e1 - e0)
    return r, np.stack([gx, gy, gz], 1)


def sample(tsdf_sum, weight, color_sum, i0, f, min_weight=1, full=False):
    """an evaluation of in-range samples -> (known [N], t [N]) and, with full, (.., grad [N,3], colour [N,3] or None)"""
    nz, ny, nx = tsdf_sum.shape
    tf, wf = tsdf_sum.reshape(-1), weight.reshape(-1)
    lin = np.stack([((i0[:, 2] + (c >> 2 & 1)) * ny + (i0[:, 1] + (c >> 1 & 1))) * nx + (i0[:, 0] + (c & 1)) for c in range(8)], 1)
    w = wf[lin]
    known = (w >= min_weight).all(1)
    ws = np.where(w >= min_weight, w, 1).astype(np.float64)
    t8 = tf[lin].astype(np.float64) / (FIX * ws)
    if not full:
        return known, _lerp8(t8, f)
    t, g = _lerp8(t8, f, True)
    col = None
    if color_sum is not None:
        cf = color_sum.reshape(3, -1)
        col = np.stack([_lerp8(cf[ch][lin].astype(np.float64) / (255.0 * ws), f) for ch in range(3)], 1)
    return known, t, g, col


def clip_range(W, dirs, origin, dims, voxel, d_min, step, n_steps):
    """csrc/tsdfrender_math.h's render_clip: a conservative range k0 .. k1 [N] of the samples that can be in range"""
    N = len(dirs)
    voxel, d_min, step = float(voxel), float(d_min), float(step)
    d_max = d_min + float(n_steps) * step
    lo, hi = np.full(N, d_min), np.full(N, d_max)
    empty, ok = np.zeros(N, bool), np.ones(N, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            p0, p1, p2 = W[a, 0] * dirs[:, 0], W[a, 1] * dirs[:, 1], W[a, 2] * dirs[:, 2]
            w = (p0 + p1) + p2
            mag = d_max * ((np.abs(p0) + np.abs(p1)) + np.abs(p2)) + abs(W[a, 3]) + abs(float(origin[a])) + float(dims[a]) * voxel
            ok &= mag * 2.0 ** -48 <= 0.25 * voxel
            s0, s1 = float(origin[a]) - W[a, 3], (float(origin[a]) + float(dims[a]) * voxel) - W[a, 3]
            par = w == 0.0
            empty |= par & ((s0 > 0.0) | (s1 < 0.0))
            e0, e1 = s0 / w, s1 / w
            lo = np.where(par, lo, np.fmax(lo, np.fmin(e0, e1)))
            hi = np.where(par, hi, np.fmin(hi, np.fmax(e0, e1)))
        empty |= ~(lo <= hi)
        a0, a1 = np.floor((lo - d_min) / step) - 1.0, np.floor((hi - d_min) / step) + 2.0
        k0 = np.where(a0 > 0.0, np.where(a0 < n_steps, a0, n_steps), 0.0)
        k1 = np.where(a1 < n_steps - 1, np.where(a1 > -1.0, a1, -1.0), n_steps - 1.0)
    k0, k1 = np.where(empty, 1.0, k0), np.where(empty, 0.0, k1)
    k0, k1 = np.where(ok, k0, 0.0), np.where(ok, k1, n_steps - 1.0)
    return k0.astype(np.int64), k1.astype(np.int64)


def render_view(tsdf_sum, weight, color_sum, origin, voxel, T, dataset, h, d_min, step, n_steps, min_weight=1, skip=True, clip=True):
    """One view against one volume, vectorised over its rays -> {"depth" [h,4h] f32, "cls" u8, "normal" [3,h,4h] f32, "color" [3,h,4h] f32 or
    None, "n_evaluated" i32}"""
    nz, ny, nx = tsdf_sum.shape
    dims = (nx, ny, nz)
    d_min, step = float(d_min), float(step)
    dirs = rays(h, dataset)
    N = len(dirs)
    W = AM.inverse(T)
    flags = brick_flags(tsdf_sum, weight, min_weight) if skip else None
    k0, k1 = clip_range(W, dirs, origin, dims, voxel, d_min, step, n_steps) if clip else (np.zeros(N, np.int64), np.full(N, n_steps - 1, np.int64))

    def at(k):
        inr, i0, f, fg = cells(W, dirs, d_min + float(k) * step, origin, voxel, dims, flags)
        m = (k >= k0) & (k <= k1)                       # outside the clip nothing is computed: out of range by the clip's argument
        return inr & m, i0, f, fg & m

    none = (np.zeros(N, bool), None, None, np.zeros(N, bool))
    cls, nev, hitk = np.zeros(N, np.uint8), np.zeros(N, np.int32), np.full(N, -1, np.int64)
    alive, pv, pflag, pt = np.ones(N, bool), np.zeros(N, bool), np.zeros(N, bool), np.zeros(N)
    cur = at(0)
    for k in range(n_steps):
        if not alive.any() or k > k1.max():
            break
        nxt = at(k + 1) if k + 1 < n_steps else none
        ev = alive & cur[0] & ((pflag | cur[3] | nxt[3]) if skip else True)
        nev += ev
        v, t = np.zeros(N, bool), np.zeros(N)
        if ev.any():
            v[ev], t[ev] = sample(tsdf_sum, weight, None, cur[1][ev], cur[2][ev], min_weight)
        pair = alive & v & pv
        hit, back = pair & (pt >= 0.0) & (t < 0.0), pair & (pt < 0.0) & (t >= 0.0)
        cls[hit], cls[back], hitk[hit] = HIT, BACK, k
        alive &= ~(hit | back)
        pv, pt, pflag, cur = v, np.where(v, t, 0.0), cur[3], nxt
    depth, normal = np.zeros(N, np.float32), np.zeros((3, N), np.float32)
    color = None if color_sum is None else np.zeros((3, N), np.float32)
    m = cls == HIT
    if m.any():
        kb = hitk[m].astype(np.float64)
        da, db = d_min + (kb - 1.0) * step, d_min + kb * step
        _, ia, fa, _ = cells(W, dirs[m], da, origin, voxel, dims)
        _, ib, fb, _ = cells(W, dirs[m], db, origin, voxel, dims)
        _, ta, ga, ca = sample(tsdf_sum, weight, color_sum, ia, fa, min_weight, True)
        _, tb, gb, cb = sample(tsdf_sum, weight, color_sum, ib, fb, min_weight, True)
        s = ta / (ta - tb)
        depth[m] = (da + s * step).astype(np.float32)
        nv = ga + s[:, None] * (gb - ga)
        nn = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
        nv = np.where(nn[:, None] > 0.0, nv / np.where(nn > 0.0, nn, 1.0)[:, None], nv)
        for i in range(3):                              # the pose's rotation: R_ij = W_ji
            normal[i, m] = ((W[0, i] * nv[:, 0] + W[1, i] * nv[:, 1]) + W[2, i] * nv[:, 2]).astype(np.float32)
        if color is not None:
            color[:, m] = (ca + s[:, None] * (cb - ca)).astype(np.float32).T
    return {"depth": depth.reshape(h, 4 * h), "cls": cls.reshape(h, 4 * h), "normal": normal.reshape(3, h, 4 * h),
            "color": None if color is None else color.reshape(3, h, 4 * h), "n_evaluated": nev.reshape(h, 4 * h)}


# ---------------------------------------------------------------------------------------------- the plain loop (Python floats)
def _cell1(W, dr, d, o, voxel, dims):
    x, y, z = d * dr[0], d * dr[1], d * dr[2]
    i0, f = [], []
    for a in range(3):
        q = ((W[a][0] * x + W[a][1] * y) + W[a][2] * z) + W[a][3]
        if not math.isfinite(q):
            return None
        u = (q - o[a]) / voxel - 0.5
        fl = math.floor(u)
        if not 0 <= fl <= dims[a] - 2:
            return None
        i0.append(fl)
        f.append(u - float(fl))
    return i0, f


def _lerp1(t, f):
    d00, d10, d01, d11 = t[1] - t[0], t[3] - t[2], t[5] - t[4], t[7] - t[6]
    a00, a10, a01, a11 = t[0] + f[0] * d00, t[2] + f[0] * d10, t[4] + f[0] * d01, t[6] + f[0] * d11
    c0, c1 = a10 - a00, a11 - a01
    b0, b1 = a00 + f[1] * c0, a01 + f[1] * c1
    gz = b1 - b0
    r = b0 + f[2] * gz
    gy = c0 + f[2] * (c1 - c0)
    e0, e1 = d00 + f[1] * (d10 - d00), d01 + f[1] * (d11 - d01)
    gx = e0 + f[2] * (e1 - e0)
    return r, [gx, gy, gz]


def _sample1(tsdf_sum, weight, color_sum, cell, min_weight):
    i0, f = cell
    t, cols = [], [[], [], []]
    for c in range(8):
        i, j, k = i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1)
        w = int(weight[k, j, i])
        if w < min_weight:
            return None
        t.append(float(tsdf_sum[k, j, i]) / (FIX * float(w)))
        if color_sum is not None:
            for ch in range(3):
                cols[ch].append(float(color_sum[ch, k, j, i]) / (255.0 * float(w)))
    r, g = _lerp1(t, f)
    return r, g, [_lerp1(cols[ch], f)[0] for ch in range(3)] if color_sum is not None else None


def render_ray_loop(tsdf_sum, weight, color_sum, origin, voxel, T, dr, d_min, step, n_steps, min_weight=1):
    """The definition, for one ray dr: k = 0 .. n_steps - 1, every in-range sample evaluated, no clip.
    -> (depth f32, cls, normal [3] f32, colour [3] f32 or None, n_evaluated)"""
    nz, ny, nx = tsdf_sum.shape
    dims = (nx, ny, nz)
    W = [[float(x) for x in row] for row in AM.inverse(T)]
    o = [float(v) for v in origin]
    voxel, d_min, step = float(voxel), float(d_min), float(step)
    dr = [float(v) for v in dr]
    zero3 = np.zeros(3, np.float32)
    prev, nev = None, 0
    for k in range(n_steps):
        d = d_min + float(k) * step
        cell = _cell1(W, dr, d, o, voxel, dims)
        cur = None
        if cell is not None:
            nev += 1
            cur = _sample1(tsdf_sum, weight, color_sum, cell, min_weight)
        if cur is not None and prev is not None:
            ta, tb = prev[0], cur[0]
            if ta >= 0.0 and tb < 0.0:
                s = ta / (ta - tb)
                depth = np.float32((d_min + float(k - 1) * step) + s * step)
                nv = [prev[1][a] + s * (cur[1][a] - prev[1][a]) for a in range(3)]
                nn = math.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
                if nn > 0.0:
                    nv = [v / nn for v in nv]
                normal = np.array([(W[0][i] * nv[0] + W[1][i] * nv[1]) + W[2][i] * nv[2] for i in range(3)]).astype(np.float32)
                col = None if color_sum is None else np.array([prev[2][ch] + s * (cur[2][ch] - prev[2][ch]) for ch in range(3)]).astype(np.float32)
                return depth, HIT, normal, col, nev
            if ta < 0.0 and tb >= 0.0:
                return np.float32(0), BACK, zero3, None if color_sum is None else zero3, nev
        prev = cur
    return np.float32(0), MISS, zero3, None if color_sum is None else zero3, nev


def render_view_loops(tsdf_sum, weight, color_sum, origin, voxel, T, dataset, h, d_min, step, n_steps, min_weight=1, pixels=None):
    """render_view's dict (skip = 0) by the plain loop; `pixels`: only these (the others are left 0)"""
    dirs = rays(h, dataset)
    N = len(dirs)
    out = {"depth": np.zeros(N, np.float32), "cls": np.zeros(N, np.uint8), "normal": np.zeros((3, N), np.float32),
           "color": None if color_sum is None else np.zeros((3, N), np.float32), "n_evaluated": np.zeros(N, np.int32)}
    for p in (range(N) if pixels is None else pixels):
        d, c, n, col, nev = render_ray_loop(tsdf_sum, weight, color_sum, origin, voxel, T, dirs[p], d_min, step, n_steps, min_weight)
        out["depth"][p], out["cls"][p], out["normal"][:, p], out["n_evaluated"][p] = d, c, n, nev
        if col is not None:
            out["color"][:, p] = col
    return {k: (None if v is None else v.reshape(v.shape[:-1] + (h, 4 * h))) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------- the call
def steps_for(dims, voxel, d_min=0.0, d_max=None, step=None):
    """util.tsdf_render_dev's host rule: step defaults to half a voxel, d_max to the box diagonal; n_steps = the samples up to d_max"""
    voxel = float(voxel)
    step = 0.5 * voxel if step is None else float(step)
    if d_max is None:
        d_max = math.sqrt(sum((float(n) * voxel) ** 2 for n in dims))
    return step, int(min(max(math.floor((float(d_max) - float(d_min)) / step) + 1, 1), MAX_STEPS))


def render(state, origin, voxel, pose, dataset, h, scene_of_view=None, d_min=0.0, step=None, n_steps=None, min_weight=1, skip=True, clip=True,
           color=True):
    """state {"tsdf_sum", "weight", "color_sum" or None} [S,..], origin [S,3], pose [V,4,4] world -> camera
    -> {"depth" [V,h,4h] f32, "cls" u8, "normal" [V,3,h,4h] f32, "color" [V,3,h,4h] f32 or None, "n_evaluated" [V,h,4h] i32}"""
    V = len(pose)
    S, nz, ny, nx = state["tsdf_sum"].shape
    sov = np.zeros(V, np.int64) if scene_of_view is None else np.asarray(scene_of_view)
    origin = np.asarray(origin, np.float64).reshape(S, 3)
    if step is None or n_steps is None:
        step, n_steps = steps_for((nx, ny, nz), voxel, d_min, None, step)
    cs = state.get("color_sum") if color else None
    views = []
    for v in range(V):
        s = int(sov[v])
        views.append(render_view(state["tsdf_sum"][s], state["weight"][s], None if cs is None else cs[s], origin[s], voxel, pose[v], dataset, h, d_min,
                                 step, n_steps, min_weight, skip, clip))
    return {k: (None if views[0][k] is None else np.stack([w[k] for w in views])) for k in KEYS}
