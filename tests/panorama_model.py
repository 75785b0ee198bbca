"""The contract of relpose_frames_to_pano (include/relpose.h) in numpy: float64 geometry with every operation rounded on
its own, an integer minimum (np.minimum.at), integer sums (np.add.at) and the integer resolve.  Test infrastructure, not product code:
the GPU tests demand that the kernels reproduce every array here bit for bit."""
import numpy as np

MAX_DEPTH = np.float32(32768.0)


def _face_rot_t(k, x, y, z):
    """Rs[k]^T v: an exact signed permutation."""
    k &= 3
    if k == 0:
        return x, y, z
    if k == 1:
        return z, y, -x
    if k == 2:
        return -x, y, -z
    return -z, y, x


def unproject(depth, scale, pose=None):
    """One frame: depth [Hf,Wf] f32, scale (sx, sy), pose 4x4 or None -> (q [N,3] f64 of the pixels with data, their flat frame indices)."""
    Hf, Wf = depth.shape
    z32 = np.asarray(depth, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z32) & (z32 > 0)
    idx = np.nonzero(ok)[0]
    r, c = (idx // Wf).astype(np.float64), (idx % Wf).astype(np.float64)
    z = z32[idx].astype(np.float64)
    xs, ys = (c / Wf - 0.5) * 2, (0.5 - r / Hf) * 2
    sx, sy = float(scale[0]), float(scale[1])
    with np.errstate(all="ignore"):
        X, Y, Z = (xs * z) / sx, (ys * z) / sy, -z
        if pose is not None:
            T = np.asarray(pose, np.float64)
            X, Y, Z = (((T[a, 0] * X + T[a, 1] * Y) + T[a, 2] * Z) + T[a, 3] * 1.0 for a in range(3))
    return np.stack((X, Y, Z), 1), idx


def project(q, h, dataset, box=None):
    """q [N,3] f64 -> (pix [N] int64: row * 4h + column, or -1 for a dropped point; d [N] f32 the face depth)."""
    N = q.shape[0]
    pix = np.full(N, -1, np.int64)
    d = np.zeros(N, np.float32)
    taken = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for slot in range(4):
            x, y, z = _face_rot_t(slot if "suncg" in dataset else slot + 3, q[:, 0], q[:, 1], q[:, 2])
            az = np.abs(z) + 1e-32
            xn, yn = x / az, y / az
            hit = (z < 0) & (np.abs(xn) < 1) & (np.abs(yn) < 1) & ~taken
            cx = np.clip(np.rint((xn[hit] + 1) * 0.5 * h), 0, h - 1).astype(np.int64)
            cy = np.clip(np.rint((1 - yn[hit]) * 0.5 * h), 0, h - 1).astype(np.int64)
            pix[hit] = cy * 4 * h + slot * h + cx
            d[hit] = (-z[hit]).astype(np.float32)
            taken |= hit
    keep = taken & (d < MAX_DEPTH)
    if box is not None:
        y0, y1, x0, x1 = box
        py, px = pix // (4 * h), pix % (4 * h)
        keep &= (py >= y0) & (py < y1) & (px >= x0) & (px < x1)
    pix[~keep] = -1
    return pix, d


def view_points(depth, rgb, scale, pose, dataset, h, box):
    """All kept points of one view's F frames: (pix [M], d [M] f32, colour [M,3] u8)."""
    P, D, Cc = [], [], []
    for f in range(depth.shape[0]):
        q, idx = unproject(depth[f], scale[f], None if pose is None else pose[f])
        pix, d = project(q, h, dataset, box)
        k = pix >= 0
        P.append(pix[k]); D.append(d[k]); Cc.append(rgb[f].reshape(-1, 3)[idx[k]])
    return np.concatenate(P), np.concatenate(D), np.concatenate(Cc)


def frames_to_pano(depth, rgb, scale, pose=None, dataset="scannet", h=160, box=None, gate=0.05):
    """depth [n,F,Hf,Wf] f32, rgb [n,F,Hf,Wf,3] u8, scale [n,F,2] f64 (or one pair), pose [n,F,4,4] f64 or None, box (y0,y1,x0,x1) or None
    -> dict of zmin u32 [n,h,4h] (f32 bits, 0 when empty), count u32, sum_z u64, sum_rgb u32 [n,3,h,4h], depth f32, rgb f32 [n,3,h,4h],
    valid u8."""
    depth = np.asarray(depth, np.float32)
    n, F = depth.shape[:2]
    scale = np.broadcast_to(np.asarray(scale, np.float64), (n, F, 2))
    hw = h * 4 * h
    g = np.float32(gate)
    out = {"zmin": np.zeros((n, hw), np.uint32), "count": np.zeros((n, hw), np.uint32), "sum_z": np.zeros((n, hw), np.uint64),
           "sum_rgb": np.zeros((n, 3, hw), np.uint32)}
    for v in range(n):
        pix, d, col = view_points(depth[v], rgb[v], scale[v], None if pose is None else pose[v], dataset, h, box)
        zb = np.full(hw, 0xFFFFFFFF, np.uint32)
        np.minimum.at(zb, pix, d.view(np.uint32))                 # positive floats order like their bit patterns
        zm = zb[pix].view(np.float32)
        acc = d <= zm + zm * g                                    # f32, two roundings
        pa, da = pix[acc], d[acc]
        cnt = np.zeros(hw, np.int64)
        np.add.at(cnt, pa, 1)
        sz = np.zeros(hw, np.int64)
        np.add.at(sz, pa, np.rint(da.astype(np.float64) * 65536.0).astype(np.int64))
        for ch in range(3):
            s = np.zeros(hw, np.int64)
            np.add.at(s, pa, col[acc, ch].astype(np.int64))
            out["sum_rgb"][v, ch] = s
        out["zmin"][v] = np.where(cnt > 0, zb, 0)
        out["count"][v] = cnt
        out["sum_z"][v] = sz
    cnt = out["count"].astype(np.int64)
    has = cnt > 0
    c1 = np.where(has, cnt, 1)
    dep = (out["sum_z"].astype(np.float64) / c1.astype(np.float64) / 65536.0).astype(np.float32)
    out["depth"] = np.where(has, dep, np.float32(0)).reshape(n, h, 4 * h)
    q = (2 * out["sum_rgb"].astype(np.int64) + c1[:, None]) // (2 * c1[:, None])
    out["rgb"] = np.where(has[:, None], q.astype(np.float32) / np.float32(255.0), np.float32(0)).reshape(n, 3, h, 4 * h)
    out["valid"] = has.astype(np.uint8).reshape(n, h, 4 * h)
    for k in ("zmin", "count", "sum_z"):
        out[k] = out[k].reshape(n, h, 4 * h)
    out["sum_rgb"] = out["sum_rgb"].reshape(n, 3, h, 4 * h)
    return out
