"""The contracts of relpose_tsdf_fuse and relpose_tsdf_surface (include/relpose.h) in numpy: float64 geometry with every
operation rounded on its own, integer sums, the crossings in their fixed order.  Test infrastructure, not product code: the GPU tests
demand that the kernels reproduce every array here bit for bit.  Each rule is stated twice, vectorised (what the tests compare the GPU
with) and as plain loops over Python floats (the check of the vectorised form)."""
import math

import numpy as np

import visibility_model as VM

MAX_DEPTH = VM.MAX_DEPTH
FIX = 32768.0
MAX_VIEWS = 4096


def centres(origin, dims, voxel):
    """-> c [nz*ny*nx, 3] f64 in the volume's order (x fastest): c_a = origin_a + (idx_a + 0.5) * voxel"""
    nx, ny, nz = (int(v) for v in dims)
    o = np.asarray(origin, np.float64)
    vx = np.float64(voxel)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[a] + (idx.reshape(-1).astype(np.float64) + 0.5) * vx for a, idx in enumerate((i, j, k))], 1)


def quantise_rgb(c):
    """f32 -> uint32: rintf(fminf(fmaxf(c, 0), 1) * 255); a NaN counts 0 (fmaxf drops it)"""
    c = np.asarray(c, np.float32)
    return np.rint(np.fmin(np.fmax(c, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint32)


def fuse_view(c, depth, rgb, T, dataset, trunc):
    """One view's update of the voxels with centres c [N,3]: depth [h,4h] f32, rgb [3,h,4h] f32 or None, T 4x4 world -> camera
    -> (dt int64 [N], dw int64 [N], dc uint32 [3,N] or None)"""
    depth = np.asarray(depth, np.float32)
    h = depth.shape[0]
    tr = np.float64(trunc)
    pix, d = VM.project(VM.move(c, T), h, dataset)
    on = (pix >= 0) & (d < MAX_DEPTH)
    pi = np.where(on, pix, 0)
    D = depth.reshape(-1)[pi]
    ok = on & VM.depth_ok(D)
    with np.errstate(all="ignore"):
        sdf = D.astype(np.float64) - d
        ok &= ~(sdf < -tr)
        t = np.minimum(sdf / tr, 1.0)
        dt = np.where(ok, np.rint(np.where(ok, t, 0.0) * FIX), 0.0).astype(np.int64)
    dc = None
    if rgb is not None:
        dc = np.where(ok[None], quantise_rgb(np.asarray(rgb, np.float32).reshape(3, -1)[:, pi]), np.uint32(0)).astype(np.uint32)
    return dt, ok.astype(np.int64), dc


def fuse(depth, rgb, pose, view_begin, origin, dims, voxel, dataset, trunc=None, state=None):
    """depth [V,h,4h] f32, rgb [V,3,h,4h] f32 or None, pose [V,4,4] f64 world -> camera, view_begin [S+1], origin [S,3], dims (nx, ny, nz)
    -> {"tsdf_sum" i32 [S,nz,ny,nx], "weight" i32, "color_sum" u32 [S,3,nz,ny,nx] or None}; a given state is added to (and returned)."""
    nx, ny, nz = (int(v) for v in dims)
    S = len(view_begin) - 1
    trunc = 4 * float(voxel) if trunc is None else trunc
    origin = np.asarray(origin, np.float64).reshape(S, 3)
    if state is None:
        state = {"tsdf_sum": np.zeros((S, nz, ny, nx), np.int32), "weight": np.zeros((S, nz, ny, nx), np.int32),
                 "color_sum": None if rgb is None else np.zeros((S, 3, nz, ny, nx), np.uint32)}
    for s in range(S):
        assert 0 <= view_begin[s + 1] - view_begin[s] <= MAX_VIEWS
        c = centres(origin[s], dims, voxel)
        for v in range(view_begin[s], view_begin[s + 1]):
            dt, dw, dc = fuse_view(c, depth[v], None if rgb is None else rgb[v], pose[v], dataset, trunc)
            state["tsdf_sum"][s] += dt.reshape(nz, ny, nx).astype(np.int32)
            state["weight"][s] += dw.reshape(nz, ny, nx).astype(np.int32)
            if rgb is not None:
                state["color_sum"][s] += dc.reshape(3, nz, ny, nx)
    return state


# ---------------------------------------------------------------------------------------------- the fuse rule as plain loops
def _project1(q, h, dataset):
    """VM.project for one point in Python floats -> (pix or -1, d)"""
    if not all(math.isfinite(v) for v in q):
        return -1, 0.0
    for slot in range(4):
        x, y, z = VM._face_rot_t(slot if "suncg" in dataset else slot + 3, q[0], q[1], q[2])
        az = abs(z) + 1e-32
        if z < 0 and abs(x / az) < 1 and abs(y / az) < 1:
            xn, yn = x / az, y / az
            cx = int(min(max(float(np.rint((xn + 1) * 0.5 * h)), 0), h - 1))
            cy = int(min(max(float(np.rint((1 - yn) * 0.5 * h)), 0), h - 1))
            return cy * 4 * h + slot * h + cx, -z
    return -1, 0.0


def fuse_loops(depth, rgb, pose, view_begin, origin, dims, voxel, dataset, trunc):
    """fuse() with one Python-float statement per operation of the rule (its check; small volumes only)"""
    nx, ny, nz = (int(v) for v in dims)
    S = len(view_begin) - 1
    voxel, trunc = float(voxel), float(trunc)
    ts = np.zeros((S, nz, ny, nx), np.int32)
    wt = np.zeros((S, nz, ny, nx), np.int32)
    cs = None if rgb is None else np.zeros((S, 3, nz, ny, nx), np.uint32)
    h = depth.shape[1]
    for s in range(S):
        o = [float(v) for v in np.asarray(origin, np.float64).reshape(S, 3)[s]]
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    c = [o[0] + (float(i) + 0.5) * voxel, o[1] + (float(j) + 0.5) * voxel, o[2] + (float(k) + 0.5) * voxel]
                    for v in range(view_begin[s], view_begin[s + 1]):
                        T = [[float(x) for x in row] for row in pose[v]]
                        q = [((T[a][0] * c[0] + T[a][1] * c[1]) + T[a][2] * c[2]) + T[a][3] for a in range(3)]
                        pix, d = _project1(q, h, dataset)
                        if pix < 0 or d >= MAX_DEPTH:
                            continue
                        z = depth[v].reshape(-1)[pix]
                        if not (z > 0 and z <= np.finfo(np.float32).max):
                            continue
                        sdf = float(z) - d
                        if sdf < -trunc:
                            continue
                        t = min(sdf / trunc, 1.0)
                        ts[s, k, j, i] += int(np.rint(t * FIX))
                        wt[s, k, j, i] += 1
                        if rgb is not None:
                            for ch in range(3):
                                cs[s, ch, k, j, i] += quantise_rgb(rgb[v].reshape(3, -1)[ch, pix])
    return {"tsdf_sum": ts, "weight": wt, "color_sum": cs}


# ---------------------------------------------------------------------------------------------- the surface
def _shift(a, c, d, fill):
    """a at v + d e_c (c: 0 = x, the last array axis); `fill` where that is outside the volume"""
    ax = 2 - c
    out = np.full_like(a, fill)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if d > 0:
        dst[ax], src[ax] = slice(0, -1), slice(1, None)
    else:
        dst[ax], src[ax] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def values(tsdf_sum, weight, min_weight=1):
    """-> (known bool, t f64; 0 where unknown)"""
    known = weight >= min_weight
    t = np.where(known, tsdf_sum.astype(np.float64) / (FIX * np.where(known, weight, 1).astype(np.float64)), 0.0)
    return known, t


def gradient(known, t):
    """-> g [3][nz,ny,nx]: central, one-sided or 0, per component"""
    g = []
    for c in range(3):
        tp, tm = _shift(t, c, 1, 0.0), _shift(t, c, -1, 0.0)
        kp, km = _shift(known, c, 1, False), _shift(known, c, -1, False)
        g.append(np.where(kp & km, (tp - tm) * 0.5, np.where(kp, tp - t, np.where(km, t - tm, 0.0))))
    return g


def surface(tsdf_sum, weight, color_sum, origin, voxel, min_weight=1):
    """One scene: tsdf_sum, weight i32 [nz,ny,nx], color_sum u32 [3,nz,ny,nx] or None -> {"points" f64 [n,3], "normals" f64 [n,3],
    "colors" f32 [n,3] or None, "n": n, "edge" i64 [n,2]: (linear index of a, axis)} in the contract's order."""
    nz, ny, nx = tsdf_sum.shape
    o = np.asarray(origin, np.float64)
    vx = np.float64(voxel)
    known, t = values(tsdf_sum, weight, min_weight)
    g = gradient(known, t)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = [v.astype(np.float64) for v in (i, j, k)]
    ctr = [o[a] + (idx[a] + 0.5) * vx for a in range(3)]
    col = None
    if color_sum is not None:
        col = [color_sum[ch].astype(np.float64) / (255.0 * np.where(known, weight, 1).astype(np.float64)) for ch in range(3)]
    keys, pts, nrm, cols = [], [], [], []
    for c in range(3):
        tb, kb = _shift(t, c, 1, 0.0), _shift(known, c, 1, False)
        cross = known & kb & (((t >= 0) & (tb < 0)) | ((t < 0) & (tb >= 0)))
        with np.errstate(all="ignore"):
            s = np.where(cross, t / np.where(cross, t - tb, 1.0), 0.0)
            n = [g[a] + s * (_shift(g[a], c, 1, 0.0) - g[a]) for a in range(3)]
            nn = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            n = [np.where(nn > 0, n[a] / np.where(nn > 0, nn, 1.0), n[a]) for a in range(3)]
        p = [o[a] + ((idx[a] + 0.5) + s) * vx if a == c else ctr[a] for a in range(3)]
        m = cross.reshape(-1)
        lin = np.nonzero(m)[0]
        keys.append(lin * 3 + c)
        pts.append(np.stack([v.reshape(-1)[m] for v in p], 1))
        nrm.append(np.stack([v.reshape(-1)[m] for v in n], 1))
        if col is not None:
            cols.append(np.stack([(col[ch] + s * (_shift(col[ch], c, 1, 0.0) - col[ch])).reshape(-1)[m] for ch in range(3)], 1).astype(np.float32))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    key = key[order]
    return {"points": np.concatenate(pts)[order], "normals": np.concatenate(nrm)[order],
            "colors": None if col is None else np.concatenate(cols)[order], "n": len(key), "edge": np.stack([key // 3, key % 3], 1)}


def surface_loops(tsdf_sum, weight, color_sum, origin, voxel, min_weight=1):
    """surface() as plain loops over Python floats (its check; small volumes only)"""
    nz, ny, nx = tsdf_sum.shape
    o = [float(v) for v in origin]
    voxel = float(voxel)
    dims = (nx, ny, nz)

    def val(v):
        if any(v[a] < 0 or v[a] >= dims[a] for a in range(3)):
            return None
        w = int(weight[v[2], v[1], v[0]])
        return float(tsdf_sum[v[2], v[1], v[0]]) / (FIX * float(w)) if w >= min_weight else None

    def step(v, c, d):
        u = list(v)
        u[c] += d
        return u

    def grad(v):
        t, g = val(v), []
        for c in range(3):
            tp, tm = val(step(v, c, 1)), val(step(v, c, -1))
            g.append((tp - tm) * 0.5 if tp is not None and tm is not None else tp - t if tp is not None else t - tm if tm is not None else 0.0)
        return g

    def colour(v, ch):
        return float(color_sum[ch, v[2], v[1], v[0]]) / (255.0 * float(weight[v[2], v[1], v[0]]))

    pts, nrm, cols, edge = [], [], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a = [i, j, k]
                ta = val(a)
                if ta is None:
                    continue
                for c in range(3):
                    b = step(a, c, 1)
                    tb = val(b)
                    if tb is None or not ((ta >= 0 and tb < 0) or (ta < 0 and tb >= 0)):
                        continue
                    s = ta / (ta - tb)
                    ga, gb = grad(a), grad(b)
                    n = [ga[x] + s * (gb[x] - ga[x]) for x in range(3)]
                    nn = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    nrm.append([n[x] / nn if nn > 0 else n[x] for x in range(3)])
                    pts.append([o[x] + ((float(a[x]) + 0.5) + s) * voxel if x == c else o[x] + (float(a[x]) + 0.5) * voxel for x in range(3)])
                    edge.append([(k * ny + j) * nx + i, c])
                    if color_sum is not None:
                        cols.append([np.float32(colour(a, ch) + s * (colour(b, ch) - colour(a, ch))) for ch in range(3)])
    f = lambda v, dt: np.asarray(v, dt).reshape(-1, 3)
    return {"points": f(pts, np.float64), "normals": f(nrm, np.float64), "colors": None if color_sum is None else f(cols, np.float32),
            "n": len(pts), "edge": np.asarray(edge, np.int64).reshape(-1, 2)}


def surface_outputs(state, origin, voxel, min_weight, cap, fill):
    """What relpose_tsdf_surface leaves in outputs pre-filled with `fill` = {"points", "normals", "colors", "valid"}: the batch of
    state["tsdf_sum"] [S,...] -> {"points" [S,cap,3], "normals", "colors" or None, "valid" u8 [S,cap], "n_points" i32 [S]}"""
    S = state["tsdf_sum"].shape[0]
    out = {"points": np.full((S, cap, 3), fill["points"], np.float64), "normals": np.full((S, cap, 3), fill["normals"], np.float64),
           "colors": None if state["color_sum"] is None else np.full((S, cap, 3), fill["colors"], np.float32),
           "valid": np.zeros((S, cap), np.uint8), "n_points": np.zeros(S, np.int32)}
    for s in range(S):
        r = surface(state["tsdf_sum"][s], state["weight"][s], None if state["color_sum"] is None else state["color_sum"][s],
                    np.asarray(origin).reshape(S, 3)[s], voxel, min_weight)
        m = min(r["n"], cap)
        out["n_points"][s] = r["n"]
        out["valid"][s, :m] = 1
        out["points"][s, :m] = r["points"][:m]
        out["normals"][s, :m] = r["normals"][:m]
        if out["colors"] is not None:
            out["colors"][s, :m] = r["colors"][:m]
    return out
