"""The pinned inputs of the alignment tests (CPU and GPU): a closed room seen by 3 views at h = 16 and 4 at h = 32, the pinned rooms of
tests/tsdf_scenes.py, leave-one-out volumes fused by the model under the true poses, the perturbed starts, a three-scene batch and the
hand-built edge cases.  Every model result is computed once per process and must be left unchanged."""
import ctypes as C
import functools

import numpy as np

import align_model as AM
import tsdf_model as TM
import tsdf_scenes as TS
from relativepose_amd import synth

CLOSED_HALF = np.array([2.0, 1.25, 2.5])
CLOSED = ((16, 3, 0.25), (32, 4, 0.125))                  # h, views, voxel: volumes 22 x 16 x 26 and 38 x 26 x 46 (the box reaches 3 voxels beyond the walls)
STARTS = ((0.0, 0.0), (0.1, 0.15), (0.2, 0.3))            # random_rigid(RandomState(1), angle, shift) applied to the true pose
ITERS = 12
EIG_MIN = 0.0043                                          # relpose_tsdf_align's default; test_align_cpu.py checks where it lies
OUT_KEYS = ("pose", "eig", "held", "sums", "rms")
TRACE_KEYS = ("trace_pose", "trace_sums")


@functools.lru_cache(maxsize=None)
def closed_room(h):
    """render_scene's draw with the half-extents fixed: rs = RandomState(11), M poses random_rigid(rs, pi, 1.0) clipped to +-0.6 half"""
    M, voxel = next((c[1], c[2]) for c in CLOSED if c[0] == h)
    rs = np.random.RandomState(11)
    half = CLOSED_HALF
    poses = []
    for _ in range(M):
        T = synth.random_rigid(rs, np.pi, 1.0)
        T[:3, 3] = np.clip(T[:3, 3], -0.6 * half, 0.6 * half)
        poses.append(T)
    dep = np.zeros((M, h, 4 * h), np.float32)
    rgb = np.zeros((M, 3, h, 4 * h), np.float32)
    for v in range(0, M, 2):
        r, _, d, _ = synth.render_room(rs, "suncg", 0.0, h, poses=[poses[v], poses[min(v + 1, M - 1)]], half=half)
        k = min(2, M - v)
        dep[v:v + k], rgb[v:v + k] = d[:k], r[:k]
    dims = tuple(int(np.ceil(2 * (half[a] + 3 * voxel) / voxel)) for a in range(3))
    return {"depth": dep, "rgb": rgb, "R": np.stack([np.linalg.inv(T) for T in poses]), "half": half, "origin": -(half + 3 * voxel)[None],
            "dims": dims, "voxel": voxel, "trunc": 4 * voxel, "view_begin": np.array([0, M], np.int32), "ds": "suncg", "h": h}


def scene(name):
    """"closed16", "closed32", or a pinned room "suncg16", "suncg32", "scannet16" """
    if name.startswith("closed"):
        return closed_room(int(name[6:]))
    ds = name.rstrip("0123456789")
    return TS.room(ds, int(name[len(ds):]))


@functools.lru_cache(maxsize=None)
def leave_one_out(name, v):
    """the model's volume of every view but v, fused under the true poses (no colours)"""
    c = scene(name)
    return TS.fuse_model(c, order=[u for u in range(len(c["depth"])) if u != v], rgb=False)


def start_pose(c, v, k):
    """view v's true pose perturbed by STARTS[k]"""
    a, t = STARTS[k]
    if a == 0.0 and t == 0.0:
        return c["R"][v].copy()
    return np.matmul(synth.random_rigid(np.random.RandomState(1), a, t), c["R"][v])


@functools.lru_cache(maxsize=None)
def solo(name, v, k=2, eig_min=EIG_MIN, iters=ITERS, stride=1):
    """the model's alignment of view v of a scene to its leave-one-out volume from start k"""
    c = scene(name)
    st = leave_one_out(name, v)
    return AM.align(st, c["origin"], c["voxel"], c["depth"][v:v + 1], start_pose(c, v, k)[None], c["ds"], None, iters, eig_min, stride)


def displacement(c, v, T):
    """rms distance, in voxels, between view v's points moved by inv(T) and by the inverse of the true pose"""
    p, _ = AM.unproject(c["depth"][v], c["ds"])
    a, b = np.linalg.inv(T), np.linalg.inv(c["R"][v])
    d = (p @ a[:3, :3].T + a[:3, 3]) - (p @ b[:3, :3].T + b[:3, 3])
    return float(np.sqrt((d * d).sum(1).mean())) / c["voxel"]


def rotation_error_deg(c, v, T):
    R = T[:3, :3] @ c["R"][v][:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


# ---------------------------------------------------------------------------------------------- the batch
@functools.lru_cache(maxsize=None)
def batch():
    """Three volumes of the closed h = 16 room's shape: (0) all but view 0, (1) all but view 1, (2) all three views; scene 1 gets no view.
    Views: 0 -> scene 0 from start 2; 1 -> scene 2 from start 1; 2: view 2's depth under a pose 100 m away (every point outside) -> scene 0;
    3: a view with 5 pixels of data only (fewer than 6 used points) -> scene 2; 4: view 0 again -> scene 2 (two views share a volume)."""
    c = closed_room(16)
    sts = [leave_one_out("closed16", 0), leave_one_out("closed16", 1), TS.fuse_model(c, rgb=False)]
    state = {k: np.concatenate([s[k] for s in sts]) for k in ("tsdf_sum", "weight")}
    far = c["R"][2].copy()
    far[0, 3] += 100.0
    few = np.zeros_like(c["depth"][1])
    few.reshape(-1)[[5, 130, 300, 555, 900]] = c["depth"][1].reshape(-1)[[5, 130, 300, 555, 900]]
    depth = np.stack([c["depth"][0], c["depth"][1], c["depth"][2], few, c["depth"][0]])
    pose = np.stack([start_pose(c, 0, 2), start_pose(c, 1, 1), far, c["R"][1], start_pose(c, 0, 1)])
    return {"state": state, "origin": np.concatenate([c["origin"]] * 3), "dims": c["dims"], "voxel": c["voxel"], "ds": "suncg", "depth": depth,
            "pose": pose, "scene_of_view": np.array([0, 2, 0, 2, 2], np.int32), "h": 16}


def batch_member(v):
    """view v of batch() with its own volume as a one-scene case"""
    b = batch()
    s = int(b["scene_of_view"][v])
    m = dict(b)
    m["state"] = {k: b["state"][k][s:s + 1] for k in ("tsdf_sum", "weight")}
    m["origin"], m["depth"], m["pose"], m["scene_of_view"] = b["origin"][s:s + 1], b["depth"][v:v + 1], b["pose"][v:v + 1], np.zeros(1, np.int32)
    return m


def model_of(case, iters=ITERS, eig_min=EIG_MIN, stride=1, min_weight=1, loops=False):
    return AM.align(case["state"], case["origin"], case["voxel"], case["depth"], case["pose"], case["ds"], case["scene_of_view"], iters, eig_min,
                    stride, min_weight, loops)


# ---------------------------------------------------------------------------------------------- hand-built edge cases
@functools.lru_cache(maxsize=None)
def edge_case(ds="suncg", h=4):
    """A 4 x 3 x 5 volume written by hand, min_weight 2, voxel 0.5, origin (-1.25, -0.75, -1.75): voxel centres at multiples of 0.5 plus
    (-1, -0.5, -1.5).  The identity pose at the world origin; the depths are set so that points land where the rule has its edges:
    u exactly integer, u = -0.0, i0 = n - 2 and n - 1, and no-data depths (NaN, inf, 0, negative).  One corner has |t| exactly 1 (saturated),
    one weight = min_weight - 1 (unknown).  View 1 has a NaN in its pose, view 2 an inf: every point outside."""
    nx, ny, nz = 4, 3, 5
    rs = np.random.RandomState(3)
    w = np.full((nz, ny, nx), 3, np.int32)
    t = (rs.randint(-30000, 30000, (nz, ny, nx)) * 3).astype(np.int32)
    t[1, 1, 1] = 32768 * 3                              # |t| = 1 exactly
    t[3, 0, 2] = -32768 * 3
    w[2, 1, 3] = 1                                      # min_weight - 1
    origin = np.array([[-1.25, -0.75, -1.75]])
    rs = np.random.RandomState(4)
    depth = rs.uniform(0.2, 1.4, (3, h, 4 * h)).astype(np.float32)
    depth[0, 0, :4] = [np.nan, np.inf, 0.0, -1.0]
    # slot 0 looks along -z (suncg): pixel (py, px) has xn = 2 px / h - 1, yn = 1 - 2 py / h; at px = h / 2, py = h / 2 the ray is the axis and
    # depth D puts the point at (0, 0, -D): u_z = (-D + 1.75) / 0.5 - 0.5 -> D = 1.5: u_z = 0 exactly; D = 1.0: u_z = 1 (integer)
    depth[0, h // 2, h // 2] = 1.5
    depth[0, h // 2, h // 2 + 1] = 1.0
    for s in (1, 2, 3):                                  # the other faces' axes, (+-0.5, 0, 0) and (0, 0, 0.5): u_x = 3 = nx - 1 and u_z = 4 = nz - 1
        depth[0, h // 2, s * h + h // 2] = 0.5           # are outside, u_x = 1 is the integer start of a cell
    depth[:, 1, 1] = 3.0e38                              # data, far outside
    pose = np.stack([np.eye(4)] * 3)
    pose[1][1, 2] = np.nan
    pose[2][0, 0] = np.inf
    state = {"tsdf_sum": t[None].copy(), "weight": w[None].copy()}
    return {"state": state, "origin": origin, "dims": (nx, ny, nz), "voxel": 0.5, "ds": ds, "depth": depth, "pose": pose,
            "scene_of_view": np.zeros(3, np.int32), "h": h, "min_weight": 2}


def boundary_points():
    """camera = world points for accumulate(): on a 4 x 3 x 5 volume with origin 0 and voxel 1, u = q - 0.5.  -> (p [N,3], expected class)"""
    p = [((0.5, 0.5, 0.5), AM.USED),                    # u = (0, 0, 0): the first cell, f = 0
         ((-0.0 + 0.5, 1.0, 2.0), AM.USED),
         ((0.5 - 2.0 ** -52, 1.0, 1.0), AM.OUTSIDE),    # u just below 0
         ((2.5, 1.0, 1.0), AM.USED),                    # u_x = 2 = nx - 2: the last cell
         ((3.5 - 2.0 ** -50, 1.0, 1.0), AM.USED),       # still inside it
         ((3.5, 1.0, 1.0), AM.OUTSIDE),                 # u_x = 3 = nx - 1
         ((1.0, 2.5, 1.0), AM.OUTSIDE),                 # u_y = 2 = ny - 1
         ((1.0, 1.0, 4.5), AM.OUTSIDE),
         ((1.0, 1.0, 3.5), AM.USED),                    # u_z = 3 = nz - 2
         ((float("nan"), 1.0, 1.0), AM.OUTSIDE), ((1.0, float("inf"), 1.0), AM.OUTSIDE), ((1e300, 1.0, 1.0), AM.OUTSIDE)]
    return np.array([q for q, _ in p]), [k for _, k in p]


# ---------------------------------------------------------------------------------------------- invalid calls
def einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, 3 views at h = 4, a 3 x 2 x 2 volume, scene_of_view 0 1 1, 2 iterations)
    that must each return RELPOSE_EINVAL.  A str value names an alternative host array."""
    return [("no_tsdf", {"tsdf_sum": 0}), ("no_weight", {"weight": 0}), ("no_depth", {"depth": 0}), ("no_pose", {"pose": 0}),
            ("no_origin", {"origin_host": 0}), ("no_scene_of_view", {"scene_of_view_host": 0}), ("no_pose_out", {"pose_out": 0}),
            ("no_eig", {"eig": 0}), ("no_held", {"held": 0}), ("no_sums", {"sums": 0}), ("no_rms", {"rms": 0}), ("no_workspace", {"workspace": 0}),
            ("trace_pose_alone", {"trace_sums": 0}), ("trace_sums_alone", {"trace_pose": 0}),
            ("dataset_low", {"dataset": -1}), ("dataset_high", {"dataset": 3}), ("reserved", {"reserved0": 1}),
            ("voxel_0", {"voxel": 0.0}), ("voxel_neg", {"voxel": -0.5}), ("voxel_nan", {"voxel": float("nan")}), ("voxel_inf", {"voxel": float("inf")}),
            ("eig_min_neg", {"eig_min": -1e-9}), ("eig_min_nan", {"eig_min": float("nan")}), ("eig_min_inf", {"eig_min": float("inf")}),
            ("iters_neg", {"iters": -1}), ("iters_65", {"iters": 65}), ("stride_0", {"stride": 0}), ("stride_neg", {"stride": -2}),
            ("min_weight_0", {"min_weight": 0}), ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("views_0", {"n_views": 0}),
            ("views_neg", {"n_views": -2}), ("h_0", {"h": 0}), ("h_odd", {"h": 5}), ("h_big", {"h": 8194}), ("pixels_2_31", {"h": 8192, "n_views": 8}),
            ("points_2_22", {"h": 1026}), ("nx_0", {"nx": 0}), ("ny_neg", {"ny": -1}), ("nz_0", {"nz": 0}), ("nx_2049", {"nx": 2049}),
            ("voxels_2_31", {"nx": 2048, "ny": 1024, "nz": 1024}), ("scene_low", {"scene_of_view_host": "sov_low"}),
            ("scene_high", {"scene_of_view_host": "sov_high"}), ("origin_nan", {"origin_host": "org_nan"}), ("origin_inf", {"origin_host": "org_inf"}),
            ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


HOST = {"sov": [0, 1, 1], "sov_low": [0, -1, 1], "sov_high": [0, 2, 1], "org": TS.FUSE_HOST["org"], "org_nan": TS.FUSE_HOST["org_nan"],
        "org_inf": TS.FUSE_HOST["org_inf"]}


def host_arrays():
    return {k: ((C.c_int32 if k.startswith("sov") else C.c_double) * len(v))(*v) for k, v in HOST.items()}


POINTERS = ("tsdf_sum", "weight", "depth", "pose", "pose_out", "eig", "held", "sums", "rms", "trace_pose", "trace_sums")


def align_args(_lib, p, host, kw, ws=256 * 1024, ws_bytes=1 << 40, ptrs=None):
    """the valid base call of einval_calls with the changes kw; p: the address every device pointer gets (ptrs overrides)"""
    a = _lib.TsdfAlignArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz, a.min_weight, a.iters, a.stride = 2, 3, 4, 0, 3, 2, 2, 1, 2, 1
    a.voxel, a.eig_min = 0.5, 0.0043
    for k in POINTERS:
        setattr(a, k, p if ptrs is None else ptrs[k])
    a.origin_host, a.scene_of_view_host = C.addressof(host["org"]), C.addressof(host["sov"])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        else:
            setattr(a, k, C.addressof(host[v]) if isinstance(v, str) else v)
    return a
