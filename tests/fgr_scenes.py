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


VOXEL_EDGE_POINTS = 2600


def voxel_edge_clouds(voxel, seed=5):
    """The situations where a voxel downsample's scan, compaction and sort can go wrong, as six clouds of VOXEL_EDGE_POINTS slots whose
    invalid slots lie BETWEEN the valid ones -> (names, pc [6, P, 3], valid [6, P] u8, colour [6, P, 3]).  Invalid slots hold a far-away
    point, so one that leaked into the bounds or the sums would show.
      empty     no valid point
      few       40 valid points (less than a wave)
      sparse    2500 valid points (two full compaction / sort rounds of 1024 and a partial one) in a cube of 20 voxels: about 2000
                voxels, 21^3 keys = 14 bits (the last digit of the sort is a partial one)
      dense     2300 valid points in 5 x 3 x 3 voxels: long runs of one key, 6 x 4 x 4 keys = 7 bits
      one_cell  1500 valid points inside 4 % of a voxel: one key, bits = 0, no sort pass
      sparse2   another sampling of `sparse` (the partner of one_cell)"""
    rs = np.random.RandomState(seed)
    P = VOXEL_EDGE_POINTS
    spec = [("empty", 0, None), ("few", 40, np.r_[6.0, 4.0, 3.0]), ("sparse", 2500, np.r_[20.0, 20.0, 20.0]),
            ("dense", 2300, np.r_[4.9, 2.9, 2.9]), ("one_cell", 1500, np.r_[0.04, 0.04, 0.04]), ("sparse2", 2500, np.r_[20.0, 20.0, 20.0])]
    pc = np.full((len(spec), P, 3), -1.0e3)
    col = rs.uniform(0, 1, (len(spec), P, 3))
    valid = np.zeros((len(spec), P), np.uint8)
    for i, (_, n, ext) in enumerate(spec):
        if n:
            slots = np.sort(rs.choice(P, n, replace=False))
            valid[i, slots] = 1
            pc[i, slots] = np.r_[0.3, -0.2, 1.0] + rs.uniform(0, 1, (n, 3)) * ext * voxel
    return [s[0] for s in spec], pc, valid, col


def key_bits(pts, voxel):
    """Bits of the largest key of §4.6 stage 1's lattice over pts (0: one cell)."""
    mb = pts.min(0) - 0.5 * voxel
    dims = np.floor((pts - mb) / voxel).astype(np.int64).max(0) + 1
    return int(int(dims.prod()) - 1).bit_length()
