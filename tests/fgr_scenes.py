"""Planted-motion fixtures of the FGR tests (not a test file): clouds sampled from a non-symmetric scene of random boxes and spheres on
a floor, cut into two overlapping crops, the target crop moved by a known rigid motion, 5 mm noise on both."""
import numpy as np


def _box_surface(rs, lo, hi, density):
    pts = []
    ext = hi - lo
    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        area = ext[u] * ext[v]
        for side in (lo[ax], hi[ax]):
            k = rs.poisson(area * density)
            p = np.empty((k, 3))
            p[:, ax] = side
            p[:, u] = rs.uniform(lo[u], hi[u], k)
            p[:, v] = rs.uniform(lo[v], hi[v], k)
            pts.append(p)
    return np.concatenate(pts)


def _sphere_surface(rs, c, r, density):
    k = rs.poisson(4 * np.pi * r * r * density)
    d = rs.normal(size=(k, 3))
    return c + r * d / np.linalg.norm(d, axis=1, keepdims=True)


def scene_points(rs, density):
    """A 3 m x 2.4 m floor, 4 boxes and 3 spheres at random places and sizes (one independent surface sampling per call)."""
    pts = [np.c_[rs.uniform(0, 3.0, int(7.2 * density)), rs.uniform(0, 2.4, int(7.2 * density)), np.zeros(int(7.2 * density))]]
    g = np.random.RandomState(1234)                      # the scene layout is fixed; only the sampling varies
    for _ in range(4):
        lo = np.r_[g.uniform(0, 2.4), g.uniform(0, 1.8), 0.0]
        hi = lo + np.r_[g.uniform(0.2, 0.6), g.uniform(0.2, 0.6), g.uniform(0.2, 0.9)]
        pts.append(_box_surface(rs, lo, hi, density))
    for _ in range(3):
        r = g.uniform(0.12, 0.3)
        pts.append(_sphere_surface(rs, np.r_[g.uniform(0.3, 2.7), g.uniform(0.3, 2.1), g.uniform(r, 0.8)], r, density))
    return np.concatenate(pts)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def planted_pair(seed, density=1200.0, noise=0.005, max_deg=60.0, max_shift=0.5):
    """-> (pc_src [n,3], pc_tgt [m,3], T [4,4]) with T p_src = p_tgt: crops x < 2.0 and x > 0.9 of two samplings of the scene, the
    scene seen from 1.5 m above a corner (so that the sensor origin is outside it)."""
    rs = np.random.RandomState(seed)
    a = scene_points(rs, density)
    b = scene_points(rs, density)
    src = a[a[:, 0] < 2.0]
    tgt = b[b[:, 0] > 0.9]
    src = src + rs.normal(0, noise, src.shape)
    tgt = tgt + rs.normal(0, noise, tgt.shape)
    off = np.r_[-1.5, -1.2, -1.5]                      # the sensor: the origin of both frames sits away from the scene
    src = src + off
    tgt = tgt + off
    R = rotation(rs.normal(size=3), rs.uniform(-max_deg, max_deg))
    t = rs.uniform(-max_shift, max_shift, 3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src, tgt @ R.T + t, T


def pose_error(T_hat, T):
    """(rotation error in degrees, translation error in m)."""
    c = (np.trace(T_hat[:3, :3] @ T[:3, :3].T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(T_hat[:3, 3] - T[:3, 3]))
