"""The contract of relpose_visibility (include/relpose.h) in numpy: float32 window extrema, float64 geometry with every
operation rounded on its own, integer counts and the fixed-point margin sum.  Test infrastructure, not product code: the GPU tests demand
that the kernels reproduce every array here bit for bit."""
import numpy as np

MAX_DEPTH = 32768.0
CLASSES = ("invalid", "outside", "unobserved", "consistent", "violation", "occluded")
INVALID, OUTSIDE, UNOBSERVED, CONSISTENT, VIOLATION, OCCLUDED = range(6)


def depth_ok(z):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


def window_image(depth, radius):
    """depth [h,4h] f32 -> (dmin, dmax) [h,4h] f32: the extrema of the valid depths in the (2r+1)^2 window clipped to the pixel's own face
    and to the rows 0..h-1; (0, 0) where the pixel's own depth is no data."""
    depth = np.asarray(depth, np.float32)
    h = depth.shape[0]
    assert depth.shape == (h, 4 * h)
    ok = depth_ok(depth)
    lo_src = np.where(ok, depth, np.float32(np.inf))
    hi_src = np.where(ok, depth, np.float32(0))
    dmin = np.full((h, 4 * h), np.inf, np.float32)
    dmax = np.zeros((h, 4 * h), np.float32)
    r = int(radius)
    for f in range(4):
        lo_f, hi_f = lo_src[:, f * h:(f + 1) * h], hi_src[:, f * h:(f + 1) * h]
        mn, mx = dmin[:, f * h:(f + 1) * h], dmax[:, f * h:(f + 1) * h]             # views: written in place
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                # destination (y, x) reads source (y + dy, x + dx) where that lies inside the face
                ys = slice(max(0, -dy), h - max(0, dy))
                xs = slice(max(0, -dx), h - max(0, dx))
                ysrc = slice(max(0, dy), h - max(0, -dy))
                xsrc = slice(max(0, dx), h - max(0, -dx))
                mn[ys, xs] = np.minimum(mn[ys, xs], lo_f[ysrc, xsrc])
                mx[ys, xs] = np.maximum(mx[ys, xs], hi_f[ysrc, xsrc])
    dmin[~ok] = 0
    dmax[~ok] = 0
    return dmin, dmax


def window_image_loops(depth, radius):
    """window_image with plain loops (its check)."""
    depth = np.asarray(depth, np.float32)
    h = depth.shape[0]
    dmin = np.zeros((h, 4 * h), np.float32)
    dmax = np.zeros((h, 4 * h), np.float32)
    ok = depth_ok(depth)
    for y in range(h):
        for x in range(4 * h):
            if not ok[y, x]:
                continue
            f0 = x // h * h
            vals = [depth[yy, xx] for yy in range(max(y - radius, 0), min(y + radius, h - 1) + 1)
                    for xx in range(max(x - radius, f0), min(x + radius, f0 + h - 1) + 1) if ok[yy, xx]]
            dmin[y, x], dmax[y, x] = min(vals), max(vals)
    return dmin, dmax


def _face_rot_t(k, x, y, z):
    """Rs[k]^T v: an exact signed permutation (panorama_model's)."""
    k &= 3
    if k == 0:
        return x, y, z
    if k == 1:
        return z, y, -x
    if k == 2:
        return -x, y, -z
    return -z, y, x


def move(p, T):
    """p [N,3] f64, T 4x4 -> q [N,3]: q_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3."""
    T = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1)


def project(q, h, dataset):
    """q [N,3] f64 -> (pix [N] int64: row * 4h + column, or -1 for a point on no face or with a non-finite coordinate; d [N] f64 = -Z).
    relpose_frames_to_pano's rule with the depth kept in float64; the d >= 32768 test is the caller's."""
    N = q.shape[0]
    pix = np.full(N, -1, np.int64)
    d = np.zeros(N, np.float64)
    fin = np.isfinite(q).all(1)
    taken = ~fin
    with np.errstate(all="ignore"):
        for slot in range(4):
            x, y, z = _face_rot_t(slot if "suncg" in dataset else slot + 3, q[:, 0], q[:, 1], q[:, 2])
            az = np.abs(z) + 1e-32
            xn, yn = x / az, y / az
            hit = (z < 0) & (np.abs(xn) < 1) & (np.abs(yn) < 1) & ~taken
            cx = np.clip(np.rint((xn[hit] + 1) * 0.5 * h), 0, h - 1).astype(np.int64)
            cy = np.clip(np.rint((1 - yn[hit]) * 0.5 * h), 0, h - 1).astype(np.int64)
            pix[hit] = cy * 4 * h + slot * h + cx
            d[hit] = -z[hit]
            taken |= hit
    return pix, d


def classify(p, valid, T, dmin, dmax, dataset, tol_abs, tol_rel):
    """One query: p [N,3] f64, valid [N] or None, T 4x4, (dmin, dmax) the reference view's window image -> (cls [N] u8, margin [N] f64: the
    violations' m, 0 elsewhere)."""
    N = p.shape[0]
    h = dmin.shape[0]
    va = np.ones(N, bool) if valid is None else np.asarray(valid) != 0
    cls = np.zeros(N, np.uint8)
    margin = np.zeros(N, np.float64)
    pix, d = project(move(np.asarray(p, np.float64), T), h, dataset)
    on = va & (pix >= 0) & (d < MAX_DEPTH)
    cls[va] = OUTSIDE
    pi = np.where(on, pix, 0)
    lo32, hi32 = dmin.reshape(-1)[pi], dmax.reshape(-1)[pi]
    seen = on & (lo32 > 0)
    cls[on & ~seen] = UNOBSERVED
    lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)
    ta, tr = np.float64(tol_abs), np.float64(tol_rel)
    with np.errstate(all="ignore"):
        lo = lo64 - (ta + tr * lo64)
        hi = hi64 + (ta + tr * hi64)
        vio = seen & (d < lo)
        occ = seen & ~vio & (d > hi)
        cls[seen] = CONSISTENT
        cls[vio] = VIOLATION
        cls[occ] = OCCLUDED
        margin[vio] = (lo - d)[vio]
    return cls, margin


def margin_fixed(margin):
    """the violations' m -> llrint(min(m, 32768) * 65536.0) as uint64"""
    return np.rint(np.minimum(margin, MAX_DEPTH) * 65536.0).astype(np.uint64)


def visibility(pc, valid, depth, query_cloud, ref_view, pose, dataset, tol_abs=0.05, tol_rel=0.02, radius=1):
    """pc [n,P,3] f64, valid [n,P] u8 or None, depth [V,h,4h] f32, query_cloud / ref_view [Q], pose [Q,4,4] f64
    -> {"counts" [Q,6] i32, "margin_sum" [Q] u64, "cls" [Q,P] u8}."""
    pc = np.asarray(pc, np.float64)
    depth = np.asarray(depth, np.float32)
    Q, P = len(query_cloud), pc.shape[1]
    wins = {}
    counts = np.zeros((Q, 6), np.int32)
    msum = np.zeros(Q, np.uint64)
    cls = np.zeros((Q, P), np.uint8)
    for q in range(Q):
        c, v = int(query_cloud[q]), int(ref_view[q])
        if v not in wins:
            wins[v] = window_image(depth[v], radius)
        cls[q], m = classify(pc[c], None if valid is None else valid[c], pose[q], *wins[v], dataset, tol_abs, tol_rel)
        counts[q] = np.bincount(cls[q], minlength=6)
        msum[q] = margin_fixed(m[cls[q] == VIOLATION]).sum(dtype=np.uint64)
    return {"counts": counts, "margin_sum": msum, "cls": cls}


def scores(counts, margin_sum):
    """util.visibility_scores in numpy: counts [...,6], margin_sum [...] -> dict of float64 arrays, NaN where a denominator is 0."""
    cn = np.asarray(counts, np.float64)
    c, v, o = cn[..., 3], cn[..., 4], cn[..., 5]
    seen = (c + v) + o
    n = cn.sum(-1) - cn[..., 0]
    with np.errstate(all="ignore"):
        div = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
        return {"agreement": div(c, seen), "violation_rate": div(v, seen), "observed": div(seen, n),
                "mean_violation": div(np.asarray(margin_sum).astype(np.float64) / 65536.0, v)}
