"""Planted-motion fixtures of the coloured ICP tests (not a test file): fgr_scenes-style pairs, but of a small scene sampled densely
enough (about 10^4 points per m^2) that the 1 cm level still has neighbours inside its 2 cm ball, with a colour that is a smooth
function of the scene point plus noise; and a textured plane, whose only in-plane constraint is its colour."""
import numpy as np

from fgr_scenes import _box_surface, _sphere_surface, pose_error, rotation  # noqa: F401

OFFSET = np.r_[-0.5, -0.4, -1.0]                       # the sensor (the origin of both frames) sits 1 m above the scene


def scene_color(p, rs=None, noise=0.01, freq=1.0):
    """Smooth RGB in [0, 1] of scene points p [n,3], plus Gaussian noise."""
    x, y, z = freq * p[:, 0], freq * p[:, 1], freq * p[:, 2]
    c = np.stack([0.5 + 0.4 * np.sin(7.0 * x + 1.0) * np.cos(5.0 * y), 0.5 + 0.4 * np.sin(6.0 * y + 3.0 * z + 0.5),
                  0.5 + 0.4 * np.cos(8.0 * z + 4.0 * x)], 1)
    if rs is not None and noise > 0:
        c = c + rs.normal(0, noise, c.shape)
    return np.clip(c, 0.0, 1.0)


def scene_points(rs, density, scale=1.0):
    """A 1.0 m x 0.8 m floor, 2 boxes and a sphere, all times `scale` (one independent surface sampling per call; the layout is fixed)."""
    k = int(0.8 * scale * scale * density)
    pts = [np.c_[rs.uniform(0, 1.0 * scale, k), rs.uniform(0, 0.8 * scale, k), np.zeros(k)]]
    pts.append(_box_surface(rs, scale * np.r_[0.15, 0.10, 0.0], scale * np.r_[0.40, 0.32, 0.22], density))
    pts.append(_box_surface(rs, scale * np.r_[0.55, 0.40, 0.0], scale * np.r_[0.82, 0.70, 0.15], density))
    pts.append(_sphere_surface(rs, scale * np.r_[0.50, 0.22, 0.12], scale * 0.12, density))
    return np.concatenate(pts)


def planted_pair(seed, density=10000.0, noise=0.001, max_deg=40.0, max_shift=0.3, scale=1.0):
    """-> (pc_src, pc_tgt, col_src, col_tgt, T [4,4]) with T p_src = p_tgt: crops x < 0.72 and x > 0.28 (times `scale`) of two samplings
    of the scene.  scale 1 keeps the numpy model quick; the feature-based initialisers need a larger scene (their FPFH radius is 0.25 m)."""
    rs = np.random.RandomState(seed)
    a, b = scene_points(rs, density, scale), scene_points(rs, density, scale)
    a, b = a[a[:, 0] < 0.72 * scale], b[b[:, 0] > 0.28 * scale]
    ca, cb = scene_color(a, rs), scene_color(b, rs)
    src = a + rs.normal(0, noise, a.shape) + OFFSET
    tgt = b + rs.normal(0, noise, b.shape) + OFFSET
    R = rotation(rs.normal(size=3), rs.uniform(-max_deg, max_deg))
    t = rs.uniform(-max_shift, max_shift, 3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src, tgt @ R.T + t, ca, cb, T


def textured_plane(seed, shift=(0.012, -0.009), density=10000.0, noise=0.0005, side=0.5):
    """A flat side x side patch under the sensor, coloured by a texture of a few cm wavelength; the target is a second sampling moved by
    `shift` inside the plane -> (pc_src, pc_tgt, col_src, col_tgt, T).  Geometry cannot see the shift; colour can."""
    rs = np.random.RandomState(seed)
    k = int(side * side * density)
    a = np.c_[rs.uniform(0, side, k), rs.uniform(0, side, k), np.zeros(k)]
    b = np.c_[rs.uniform(0, side, k), rs.uniform(0, side, k), np.zeros(k)]
    ca, cb = scene_color(a, rs, freq=4.0), scene_color(b, rs, freq=4.0)
    off = np.r_[-side / 2, -side / 2, -1.0]
    src = a + np.c_[np.zeros((k, 2)), rs.normal(0, noise, k)] + off
    tgt = b + np.c_[np.zeros((k, 2)), rs.normal(0, noise, k)] + off
    T = np.eye(4)
    T[:2, 3] = shift
    return src, tgt + T[:3, 3], ca, cb, T


def perturbed(T, seed, deg=3.0, shift=0.02):
    """T composed with a small random motion about the scene: the start a local refinement is given."""
    rs = np.random.RandomState(1000 + seed)
    D = np.eye(4)
    D[:3, :3] = rotation(rs.normal(size=3), deg)
    c = OFFSET + np.r_[0.5, 0.4, 0.0]                    # rotate about the scene's centre, not the far origin
    d = rs.normal(size=3)
    D[:3, 3] = c - D[:3, :3] @ c + shift * d / np.linalg.norm(d)
    return T @ D
