"""Shared inputs of the visibility tests (test infrastructure): multi-view scenes of all three panorama conventions, their observed clouds
through the oracle, the directed queries under the ground-truth poses and under stated wrong poses, and the numpy model's results, computed
once per process.  The model's integer results are pinned as constants, the way overlap_scenes.NO_HIT is."""
import functools

import numpy as np

import overlap_model as OM
import overlap_scenes as OS
import visibility_model as VM
from relativepose_amd import synth

# The scenes that satisfy both conditions under the model alone (test_visibility_cpu.py checks them): at most 1 % of the classified points
# contradicted under the ground-truth poses, more than 10 % under the wrong ones.  The observed cloud of a scannet view is geometrically
# right only at h = 160 (relpose_depth2pc keeps the reference's fixed / 160 rescaling of the kinect crop), hence that scene's size.
SCENES = (("suncg", 32), ("matterport", 32), ("scannet", 160), ("suncg", 16))
# Dropped from the conditions, kept for the bitwise comparisons: the 192-point scannet crop at h = 32 (a partial last wave).  Its cloud is
# scaled by 32 / 160 against its panorama, so 43 % of its classified points are contradicted under the ground-truth poses.
BITWISE_ONLY = (("scannet", 32),)
SCENE_SEED, SCENE_VIEWS = 7, 4
WRONG_SEED, WRONG_ANGLE, WRONG_SHIFT = 11, 0.6, 0.5      # the wrong pose of query k: random_rigid(RandomState(WRONG_SEED + k), 0.6, 0.5) T_gt
POINTS = {("suncg", 32): 1024, ("matterport", 32): 1024, ("scannet", 160): 5808, ("suncg", 16): 256, ("scannet", 32): 192}

# the model's counts summed over the scene's 12 directed queries, classes 0..5, default parameters (radius 1, tol 0.05 + 0.02 d), and the
# sum of margin_sum: {scene: (ground truth, wrong)}
PINNED = {
    ("suncg", 32): (((0, 3695, 0, 8585, 8, 0), 10481), ((0, 3836, 0, 3303, 3095, 2054), 47535942)),
    ("matterport", 32): (((99, 4014, 100, 8064, 11, 0), 11009), ((99, 3930, 97, 2852, 1901, 3409), 37697342)),
    ("scannet", 160): (((651, 21405, 525, 47115, 0, 0), 0), ((651, 22249, 493, 13469, 8822, 24012), 218326834)),
    ("suncg", 16): (((0, 937, 0, 2123, 12, 0), 54753), ((0, 971, 0, 1016, 622, 463), 8558860)),
    ("scannet", 32): (((12, 641, 5, 936, 450, 260), 5958635), ((12, 692, 0, 460, 452, 688), 7951477)),
}


def wrong_poses(T):
    """T [Q,4,4] ground-truth poses -> the stated wrong poses"""
    return np.stack([np.matmul(synth.random_rigid(np.random.RandomState(WRONG_SEED + k), WRONG_ANGLE, WRONG_SHIFT), T[k]) for k in range(len(T))])


@functools.lru_cache(maxsize=None)
def scene(ds, h):
    """-> dict: depth [M,h,4h], pc, valid (the observed clouds), the M (M - 1) directed queries (qc, rv, T ground truth, W wrong) (read-only)."""
    sc = synth.render_scene(SCENE_SEED, SCENE_VIEWS, ds, h)
    pc, valid = OS.observed_clouds(sc["depth"], ds)
    qc, rv, T = OM.matrix_queries(sc["R"])
    return {"depth": sc["depth"], "R": sc["R"], "pc": pc, "valid": valid, "qc": qc, "rv": rv, "T": T, "W": wrong_poses(T)}


@functools.lru_cache(maxsize=None)
def model(ds, h, radius=1, wrong=False, tol_abs=0.05, tol_rel=0.02):
    """the numpy model's result for the scene's queries (read-only)"""
    s = scene(ds, h)
    return VM.visibility(s["pc"], s["valid"], s["depth"], s["qc"], s["rv"], s["W" if wrong else "T"], ds, tol_abs, tol_rel, radius)


# ---------------------------------------------------------------------------------------------------------------- hand-built edge cases
EDGE_H, EDGE_P = 16, 1536
EDGE_DEPTH = np.float32(2.7)                              # view 0: this depth everywhere


def aim(ds, slot, row, col, d, h=EDGE_H):
    """the point that projects onto the centre of pixel (row, slot h + col) of a `ds` panorama at face depth d (exactly: the face rotation is
    a signed permutation)"""
    v = np.array([(col / h - 0.5) * 2 * d, (0.5 - row / h) * 2 * d, -d])
    return np.matmul(synth.face_rotation(ds, slot), v)


def face_point(ds, slot, x, y, z):
    """face coordinates -> panorama frame"""
    return np.matmul(synth.face_rotation(ds, slot), np.array([x, y, z], np.float64))


def bounds(tol_abs=0.05, tol_rel=0.02, depth=EDGE_DEPTH):
    """(lo, hi) of the contract for one reference depth, each operation rounded on its own"""
    dm = np.float64(depth)
    return dm - (np.float64(tol_abs) + np.float64(tol_rel) * dm), dm + (np.float64(tol_abs) + np.float64(tol_rel) * dm)


# cloud 0 of edge_case: (name, expected class under the identity pose against view 0 with the default parameters)
def special_points(ds):
    lo, hi = bounds()
    inf, nan = np.inf, np.nan
    P = [("on_lo", face_point(ds, 0, 0, 0, -lo), 3), ("below_lo", face_point(ds, 0, 0, 0, -np.nextafter(lo, -inf)), 4),
         ("above_lo", face_point(ds, 0, 0, 0, -np.nextafter(lo, inf)), 3), ("on_hi", face_point(ds, 0, 0, 0, -hi), 3),
         ("above_hi", face_point(ds, 0, 0, 0, -np.nextafter(hi, inf)), 5), ("below_hi", face_point(ds, 0, 0, 0, -np.nextafter(hi, -inf)), 3),
         ("xn_is_1", np.array([1.0, 0.0, -1.0]), 1), ("xn_is_minus_1", np.array([-2.0, 0.5, -2.0]), 1), ("yn_is_1", np.array([0.0, 3.0, -3.0]), 1),
         ("origin", np.zeros(3), 1), ("z_is_0", face_point(ds, 0, 2.7, 0.25, 0.0), 3),          # Z = 0 on face 0: the next face takes it, at d = 2.7
         ("above", np.array([0.1, 5.0, -0.1]), 1), ("below", np.array([0.1, -5.0, 0.1]), 1),     # the panorama has no top or bottom face
         ("just_inside_32768", face_point(ds, 2, 0, 0, -np.nextafter(32768.0, 0)), 5), ("at_32768", face_point(ds, 2, 0, 0, -32768.0), 1),
         ("nan_x", np.array([nan, 0.0, -1.0]), 1), ("inf_z", np.array([0.0, 0.0, inf]), 1), ("minus_inf_z", np.array([0.0, 0.0, -inf]), 1),
         ("inf_x", np.array([inf, 0.0, -1.0]), 1), ("huge", np.array([1e300, 1e300, -1e300]), 1)]
    # (xn + 1) * 0.5 * h = k + 0.5 exactly, k even and odd, in columns and rows and at two depths: the pixel is the even neighbour
    for k in (4, 5, 10, 11):
        for z in (1.0, 4.0):
            P.append((f"half_col_{k}_{z}", face_point(ds, 1, ((k + 0.5) / 8 - 1) * z, 0.1 * z, -z), 4 if z == 1.0 else 5))
            P.append((f"half_row_{k}_{z}", face_point(ds, 3, 0.1 * z, (1 - (k + 0.5) / 8) * z, -z), 4 if z == 1.0 else 5))
    return P


@functools.lru_cache(maxsize=None)
def edge_case(ds):
    """-> dict(pc [5,P,3], valid [5,P], depth [2,h,4h], qc, rv, pose, h): see the comments (read-only)."""
    h, P = EDGE_H, EDGE_P
    rs = np.random.RandomState(5)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    depth = np.zeros((2, h, 4 * h), np.float32)
    depth[0] = EDGE_DEPTH
    for f in range(4):                                                         # view 1: every face at its own depth, so a window that
        depth[1][:, f * h:(f + 1) * h] = 2.0 + 1.5 * f + rs.uniform(-0.3, 0.3, (h, h))      # crossed a seam would change the classes
    bad = [(0, 0, 0.0), (0, h - 2, -1.0), (0, h + 1, nan), (h - 1, h - 2, inf), (h - 1, h + 1, 0.0), (5, 5, -inf), (9, 2 * h - 1, nan), (9, 2 * h + 1, 0.0)]
    for r, c, v in bad:
        depth[1][r, c] = v
    for r in range(6, 11):                                                     # a pixel whose 24 neighbours are all invalid, each kind of "no data"
        for c in range(3 * h + 6, 3 * h + 11):
            if (r, c) != (8, 3 * h + 8):
                depth[1][r, c] = (0.0, -1.0, nan, inf)[(r + c) % 4]
    depth[1][3, 2 * h + 3] = 40000.0                                           # deeper than any classified point: always a violation
    depth[1][12, 2 * h + 12] = 1e6                                             # its margin saturates at 32768
    depth[1][13, 2 * h + 3] = np.float32(3.4e38)

    pc = np.zeros((5, P, 3))
    valid = np.zeros((5, P), np.uint8)
    sp = special_points(ds)
    for k, (_, p, _) in enumerate(sp):
        pc[0, k] = p
    valid[0, :len(sp)] = 1
    valid[0, len(sp) + 3:len(sp) + 70] = 1                                     # valid zeros: the origin, outside
    # cloud 1: one point through the centre of every pixel of view 1 (invalid ones at depth 2), in front of, on and behind the surface
    factor = (0.8, 1.0, 1.25, 0.97, 1.03, 1.0)
    k = 0
    for r in range(h):
        for c in range(4 * h):
            z = depth[1][r, c]
            d = float(z) if np.isfinite(z) and 0 < z < 100 else 2.0
            pc[1, k] = aim(ds, c // h, r, c % h, d * factor[k % 6])
            k += 1
    valid[1, :k] = 1
    for j, (r, c) in enumerate(((0, h - 1), (0, h), (h - 1, h - 1), (h - 1, h), (1, h - 1), (1, h), (8, 3 * h + 8), (3, 2 * h + 3), (12, 2 * h + 12),
                                (13, 2 * h + 3))):
        for i, d in enumerate((1.0, 2.1, 2.9, 3.4, 3.6, 4.4, 5.9, 6.4, 7.5, 30000.0)):       # the seams, the corners, the lone and the deep pixels
            pc[1, k] = aim(ds, c // h, r, c % h, d)
            valid[1, k] = 1
            k += 1
    assert k <= P
    pc[2] = aim(ds, 1, 7, 9, 2.7)                                              # cloud 2: every point the same: one pixel, one class
    valid[2] = 1
    pc[3] = rs.randn(P, 3)                                                     # cloud 3: no valid point
    pc[4] = rs.randn(P, 3) * 3                                                 # cloud 4: NaN and inf sprinkled over a random cloud, all valid (valid = 1)
    pc[4, ::7, 0] = np.nan
    pc[4, 3::11, 2] = np.inf
    pc[4, 5::13, 1] = -np.inf
    valid[4] = 1
    eye = np.eye(4)
    near = eye.copy()
    near[:3, 3] = -0.6 * aim(ds, 1, 7, 9, 2.7) / 2.7                           # pulls cloud 2 0.6 towards the camera: all violations
    small = np.matmul(synth.random_rigid(np.random.RandomState(3), 0.2, 0.3), eye)
    pn, pi = eye.copy(), eye.copy()
    pn[1, 2] = np.nan
    pi[0, 3] = np.inf
    queries = [(0, 0, eye), (1, 1, eye), (1, 1, small), (2, 0, eye), (2, 0, near), (3, 1, eye), (4, 0, eye), (4, 1, small), (1, 0, pn), (1, 1, pi),
               (0, 1, eye), (0, 1, small)]
    return {"pc": pc, "valid": valid, "depth": depth, "h": h, "qc": np.array([q[0] for q in queries], np.int32),
            "rv": np.array([q[1] for q in queries], np.int32), "pose": np.stack([q[2] for q in queries])}


def einval_calls():
    """(name, field overrides) of every RELPOSE_EINVAL condition of relpose_visibility, for a base call with 2 clouds of 8 points, 2 views
    of h = 4 and 2 queries; "bad_q" / "bad_r" stand for index arrays with an entry out of range"""
    import ctypes as C
    from relativepose_amd import _lib
    nan, inf = float("nan"), float("inf")
    calls = [("short struct", dict(struct_size=16)), ("stream cut off", dict(struct_size=C.sizeof(_lib.VisibilityArgs) - 8))]
    calls += [(f"NULL {n}", {n: None}) for n in ("pc", "depth", "query_cloud_host", "ref_view_host", "pose", "counts", "margin_sum", "workspace")]
    calls += [(f"dataset {v}", dict(dataset=v)) for v in (-1, 3)] + [(f"radius {v}", dict(radius=v)) for v in (-1, 3)]
    calls += [(f"tol_abs {v}", dict(tol_abs=v)) for v in (-0.01, nan, inf)] + [(f"tol_rel {v}", dict(tol_rel=v)) for v in (-0.01, nan, inf)]
    calls += [("h odd", dict(h=5)), ("h 0", dict(h=0)), ("h too large", dict(h=8194)), ("h < 2r+1", dict(h=2, radius=1)), ("h < 2r+1", dict(h=4, radius=2)),
              ("n_views 0", dict(n_views=0)), ("n_clouds 0", dict(n_clouds=0)), ("n_points 0", dict(n_points=0)), ("n_queries 0", dict(n_queries=0)),
              ("n_points > 2^24", dict(n_points=(1 << 24) + 1)), ("pixels >= 2^31", dict(n_views=8, h=8192)),
              ("blocks >= 2^31", dict(n_points=1 << 24, n_queries=1 << 15)),
              ("cloud index", dict(n_clouds=1)), ("view index", dict(n_views=1)), ("negative cloud", dict(query_cloud_host="bad_q")),
              ("negative view", dict(ref_view_host="bad_q")), ("view too large", dict(ref_view_host="bad_r")),
              ("workspace too small", dict(workspace_bytes=64)), ("workspace unaligned", dict(workspace_offset=8))]
    return calls


def totals(res):
    """-> (counts summed over the queries as a tuple of 6 ints, the sum of margin_sum as an int)"""
    return tuple(int(v) for v in res["counts"].sum(0)), int(res["margin_sum"].sum())


def contradicted(counts):
    """the share of the classified points (consistent + violation + occluded) that are violations or occluded"""
    c, v, o = (int(np.asarray(counts)[..., k].sum()) for k in (3, 4, 5))
    return (v + o) / (c + v + o)


def same(got, want, keys=("counts", "margin_sum", "cls")):
    """bitwise comparison of two result dicts; returns the list of keys that differ"""
    return [k for k in keys if not np.array_equal(np.asarray(got[k]).astype(np.asarray(want[k]).dtype), np.asarray(want[k]))]
