"""The pinned inputs of the TSDF tests (CPU and GPU): three synthetic rooms, two tiny volumes, a three-scene batch, a hand-built fuse edge
case and a hand-built state for the surface rule.  Every model result is computed once per process and must be left unchanged."""
import ctypes as C
import functools

import numpy as np

import tsdf_model as TM
import visibility_model as VM
from relativepose_amd import synth

ROOMS = (("suncg", 16, 3, 0.25), ("suncg", 32, 4, 0.125), ("scannet", 16, 3, 0.25))     # dataset, h, views, voxel
ROOM_KEYS = tuple(r[:2] for r in ROOMS)
STATE_KEYS = ("tsdf_sum", "weight", "color_sum")
SURF_KEYS = ("points", "normals", "colors", "valid", "n_points")
FILL = {"points": -7.5, "normals": 9.25, "colors": -3.0}                               # what the surface outputs are pre-filled with
SEED = 7


def bits_equal(a, b):
    """bit for bit, NaN payloads included"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differ(got, want, keys):
    return [k for k in keys if not bits_equal(got[k], want[k])]


@functools.lru_cache(maxsize=None)
def room(ds, h):
    """{"depth", "rgb", "R", "half", "origin" [1,3], "dims", "voxel", "trunc", "view_begin"}: the box reaches 3 voxels beyond the walls"""
    M, voxel = next((r[2], r[3]) for r in ROOMS if r[:2] == (ds, h))
    sc = synth.render_scene(SEED, M, ds, h)
    half = sc["half"]
    dims = tuple(int(np.ceil(2 * (half[a] + 3 * voxel) / voxel)) for a in range(3))
    return {"depth": sc["depth"].astype(np.float32), "rgb": sc["rgb"].astype(np.float32), "R": sc["R"], "half": half,
            "origin": -(half + 3 * voxel)[None], "dims": dims, "voxel": voxel, "trunc": 4 * voxel, "view_begin": np.array([0, M], np.int32),
            "ds": ds, "h": h}


def fuse_model(c, R=None, order=None, rgb=True):
    """the model's state of a case; `order` (single-scene cases only) picks and orders the views"""
    R = c["R"] if R is None else R
    o = list(range(len(c["depth"]))) if order is None else list(order)
    vb = c["view_begin"] if order is None else np.array([0, len(o)], np.int32)
    return TM.fuse(c["depth"][o], c["rgb"][o] if rgb else None, R[o], vb, c["origin"], c["dims"], c["voxel"], c["ds"], c["trunc"])


@functools.lru_cache(maxsize=None)
def room_state(ds, h):
    return fuse_model(room(ds, h))


def surface_cap(state, origin, voxel, min_weight=1):
    return max(int(TM.surface(state["tsdf_sum"][s], state["weight"][s], None, origin[s], voxel, min_weight)["n"]) for s in range(len(origin)))


@functools.lru_cache(maxsize=None)
def room_surface(ds, h):
    """(cap, surface_outputs): cap = the number of crossings + 5, so rows beyond n stay pre-filled"""
    c, st = room(ds, h), room_state(ds, h)
    cap = surface_cap(st, c["origin"], c["voxel"]) + 5
    return cap, TM.surface_outputs(st, c["origin"], c["voxel"], 1, cap, FILL)


def wall_error(points, half, voxel):
    """distance of every point to the nearest wall plane |x_a| = half_a, in voxels"""
    return np.abs(np.abs(points) - np.asarray(half)[None]).min(1) / voxel


def wall_stats(points, half, voxel):
    e = wall_error(points, half, voxel)
    return float(np.median(e)), float(np.percentile(e, 90)), float(e.max())


def perturbed(c):
    """the poses with view 0's replaced by random_rigid(RandomState(1), 0.2, 0.3) applied in its camera frame"""
    R = c["R"].copy()
    R[0] = np.matmul(synth.random_rigid(np.random.RandomState(1), 0.2, 0.3), R[0])
    return R


def surface_points(state, c, s=0):
    return TM.surface(state["tsdf_sum"][s], state["weight"][s], None, c["origin"][s], c["voxel"])["points"]


# ---------------------------------------------------------------------------------------------- small volumes and the batch
@functools.lru_cache(maxsize=None)
def tiny(which):
    """the suncg h = 16 room seen through a 1 x 1 x 2 box across its +z wall, or a 5 x 3 x 2 box across its +x wall"""
    c = dict(room("suncg", 16))
    hf = c["half"]
    if which == "1x1x2":
        c["dims"], c["origin"] = (1, 1, 2), np.array([[0.05, -0.1, hf[2] - 0.25]])
    else:
        c["dims"], c["origin"] = (5, 3, 2), np.array([[hf[0] - 0.6, -0.4, -0.3]])
    return c


@functools.lru_cache(maxsize=None)
def batch():
    """three scenes sharing dims: the suncg h = 16 room's 3 views, no view, and 2 views of another room in a shifted box"""
    a = room("suncg", 16)
    b = synth.render_scene(SEED + 1, 2, "suncg", 16)
    c = dict(a)
    c["depth"] = np.concatenate([a["depth"], b["depth"].astype(np.float32)])
    c["rgb"] = np.concatenate([a["rgb"], b["rgb"].astype(np.float32)])
    c["R"] = np.concatenate([a["R"], b["R"]])
    c["view_begin"] = np.array([0, 3, 3, 5], np.int32)
    c["origin"] = np.concatenate([a["origin"], a["origin"] + 1.0, a["origin"] + 0.1])
    return c


def batch_member(k):
    """scene k of batch() as a case of its own"""
    c = dict(batch())
    v0, v1 = c["view_begin"][k], c["view_begin"][k + 1]
    if v1 == v0:
        return None
    c["depth"], c["rgb"], c["R"] = c["depth"][v0:v1], c["rgb"][v0:v1], c["R"][v0:v1]
    c["view_begin"], c["origin"] = np.array([0, v1 - v0], np.int32), c["origin"][k:k + 1]
    return c


# ---------------------------------------------------------------------------------------------- the hand-built fuse edge case
EDGE_H, EDGE_DIMS, EDGE_VOXEL, EDGE_TRUNC = 8, (16, 8, 3), 0.25, 1.0
EDGE_ORIGIN = np.array([[-2.125, -1.125, -2.125]])   # centres x -2 .. 1.75, y -1 .. 0.75, z -2, -1.75, -1.5: all exact
F32 = np.float32
SPECIAL_DEPTHS = (F32(1.0), np.nextafter(F32(1.0), F32(0)), np.nextafter(F32(1.0), F32(2)), F32(0), F32(-1), F32(np.nan), F32(np.inf),
                  F32(3.0e38), F32(2.0), F32(1.5), F32(2.5), F32(-np.inf))


@functools.lru_cache(maxsize=None)
def edge_case(ds):
    """View 0 looks from the world origin with the identity pose at a box of exact voxel centres: in the z = -2 layer |x / z| = 1 exactly at
    x = -2, and every other x / z (an odd multiple of 1 / 8) lands on a half pixel at h = 8.  The pixels that layer's voxels hit carry SPECIAL_DEPTHS in turn: with
    trunc = 1 and d = 2, depth 1 gives sdf = -trunc exactly, its float32 neighbours one ulp either side, then 0, -1, NaN, inf, huge and -inf.
    View 1 is translated so that the z = -2 layer has d = 32768 exactly and the other two layers d just below.  View 2's pose holds a NaN,
    view 3's an inf.  View 4 is rotated about y and looks at the box obliquely.  rgb runs from -0.5 to 1.5 and holds NaN."""
    h = EDGE_H
    rs = np.random.RandomState(11)
    V = 5
    depth = (2.0 + rs.uniform(-0.6, 0.6, (V, h, 4 * h))).astype(np.float32)
    rgb = rs.uniform(-0.5, 1.5, (V, 3, h, 4 * h)).astype(np.float32)
    rgb[:, :, 0, ::5] = np.nan
    rgb[0, 1, 1, :] = 0.5
    pose = np.stack([np.eye(4)] * V)
    pose[1][2, 3] = -32766.0
    depth[1] = 40000.0
    depth[1, 4, :] = 32767.0                         # the row all of view 1's voxels land in
    pose[2][0, 3] = np.nan
    pose[3][1, 1] = np.inf
    a = 0.7
    pose[4][:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    pose[4][:3, 3] = [0.25, -0.125, 0.5]
    c = TM.centres(EDGE_ORIGIN[0], EDGE_DIMS, EDGE_VOXEL)
    pix, d = VM.project(VM.move(c, pose[0]), h, ds)
    layer = np.nonzero((c[:, 2] == -2.0) & (pix >= 0))[0]
    first = list(dict.fromkeys(pix[layer].tolist()))                                       # several voxels share a pixel: stamp each once
    for n, px in enumerate(first):
        depth[0].reshape(-1)[px] = SPECIAL_DEPTHS[n % len(SPECIAL_DEPTHS)]
    return {"depth": depth, "rgb": rgb, "R": pose, "origin": EDGE_ORIGIN, "dims": EDGE_DIMS, "voxel": EDGE_VOXEL, "trunc": EDGE_TRUNC,
            "view_begin": np.array([0, V], np.int32), "ds": ds, "h": h}


# ---------------------------------------------------------------------------------------------- the hand-built state of the surface rule
@functools.lru_cache(maxsize=None)
def edge_state():
    """A 6 x 4 x 3 state written by hand: values of exactly 0 next to a negative one (a crossing at s = 0), next to another 0 (none) and
    behind a negative one (s = 1 seen from the other side); an isolated known voxel; weights below min_weight = 2; a checkerboard corner
    that crosses on every edge (more crossings than the small cap)."""
    nx, ny, nz = 6, 4, 3
    rs = np.random.RandomState(5)
    w = np.full((nz, ny, nx), 3, np.int32)
    t = (rs.randint(-32768, 32768, (nz, ny, nx)) * 3).astype(np.int32)
    t[0, 0, 0:4] = [0, -3000, 0, 0]                  # ta = 0 | tb < 0: crossing at s = 0; -3000 | 0: crossing at s = 1; 0 | 0: none
    w[1, 1, 1] = 1                                   # below min_weight: unknown
    w[:, 2:, 4:] = 0                                 # an unknown corner block ...
    w[1, 3, 5] = 4                                   # ... around one known voxel: its six neighbours are unknown or outside
    t[1, 3, 5] = 5000
    col = rs.randint(0, 256 * 3, (3, nz, ny, nx)).astype(np.uint32)
    return {"tsdf_sum": t[None].copy(), "weight": w[None].copy(), "color_sum": col[None].copy(), "origin": np.array([[0.3, -1.7, 2.9]]),
            "voxel": 0.3, "min_weight": 2, "dims": (nx, ny, nz)}


# ---------------------------------------------------------------------------------------------- invalid calls
def fuse_einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, 3 views at h = 4, a 3 x 2 x 2 volume, view_begin 0 2 3) that must each
    return RELPOSE_EINVAL.  A str value names an alternative host array; "null:<field>" is written as 0."""
    big = 1 << 30
    return [("no_depth", {"depth": 0}), ("no_pose", {"pose": 0}), ("no_view_begin", {"view_begin_host": 0}), ("no_origin", {"origin_host": 0}),
            ("no_tsdf", {"tsdf_sum": 0}), ("no_weight", {"weight": 0}), ("no_workspace", {"workspace": 0}),
            ("rgb_without_color", {"color_sum": 0}), ("color_without_rgb", {"rgb": 0}),
            ("dataset_low", {"dataset": -1}), ("dataset_high", {"dataset": 3}), ("accumulate_2", {"accumulate": 2}), ("accumulate_neg", {"accumulate": -1}),
            ("reserved", {"reserved0": 1}), ("voxel_0", {"voxel": 0.0}), ("voxel_neg", {"voxel": -0.5}), ("voxel_nan", {"voxel": float("nan")}),
            ("voxel_inf", {"voxel": float("inf")}), ("trunc_0", {"trunc": 0.0}), ("trunc_neg", {"trunc": -1.0}), ("trunc_nan", {"trunc": float("nan")}),
            ("trunc_inf", {"trunc": float("inf")}), ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("views_0", {"n_views": 0}),
            ("views_neg", {"n_views": -2}), ("h_0", {"h": 0}), ("h_odd", {"h": 5}), ("h_big", {"h": 8194}), ("pixels_2_31", {"h": 8192, "n_views": 8}),
            ("nx_0", {"nx": 0}), ("ny_0", {"ny": 0}), ("nz_0", {"nz": 0}), ("nx_neg", {"nx": -3}), ("voxels_2_31", {"nx": big, "ny": 2, "nz": 1}),
            ("voxels_2_31_all", {"nx": 2048, "ny": 1024, "nz": 1024}), ("scene_voxels_2_31", {"nx": 1 << 15, "ny": 1 << 15, "nz": 1}),
            ("begin_not_0", {"view_begin_host": "vb_start"}), ("begin_descending", {"view_begin_host": "vb_desc"}),
            ("begin_end", {"view_begin_host": "vb_end"}), ("begin_past", {"view_begin_host": "vb_past"}),
            ("too_many_views", {"view_begin_host": "vb_4097", "n_views": 4097}), ("origin_nan", {"origin_host": "org_nan"}),
            ("origin_inf", {"origin_host": "org_inf"}), ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}),
            ("struct_small", {"struct_size": 16})]


FUSE_HOST = {"vb": [0, 2, 3], "vb_start": [1, 2, 3], "vb_desc": [0, 3, 2], "vb_end": [0, 2, 2], "vb_past": [0, 2, 4], "vb_4097": [0, 4097, 4097],
             "org": [0.0, 0.5, 1.0, -1.0, 2.0, 0.25], "org_nan": [0.0, float("nan"), 1.0, -1.0, 2.0, 0.25],
             "org_inf": [0.0, 0.5, 1.0, -1.0, float("inf"), 0.25]}


def surface_einval_calls():
    """the same for relpose_tsdf_surface (2 scenes, a 3 x 2 x 2 volume, cap 8, min_weight 1)"""
    return [("no_tsdf", {"tsdf_sum": 0}), ("no_weight", {"weight": 0}), ("no_origin", {"origin_host": 0}), ("no_points", {"points": 0}),
            ("no_normals", {"normals": 0}), ("no_valid", {"valid": 0}), ("no_n_points", {"n_points": 0}), ("no_workspace", {"workspace": 0}),
            ("colors_without_color_sum", {"color_sum": 0}), ("min_weight_0", {"min_weight": 0}), ("min_weight_neg", {"min_weight": -1}),
            ("cap_0", {"cap": 0}), ("cap_neg", {"cap": -5}), ("cap_big", {"cap": 1 << 28}), ("reserved", {"reserved0": 2}),
            ("voxel_0", {"voxel": 0.0}), ("voxel_neg", {"voxel": -0.1}), ("voxel_nan", {"voxel": float("nan")}), ("voxel_inf", {"voxel": float("inf")}),
            ("scenes_0", {"n_scenes": 0}), ("nx_0", {"nx": 0}), ("ny_neg", {"ny": -1}), ("nz_0", {"nz": 0}),
            ("voxels_2_31", {"nx": 2048, "ny": 1024, "nz": 1024}), ("crossings_2_31", {"nx": 1024, "ny": 1024, "nz": 700, "n_scenes": 1}),
            ("origin_nan", {"origin_host": "org_nan"}), ("origin_inf", {"origin_host": "org_inf"}), ("workspace_small", {"workspace_bytes": 255}),
            ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


def host_arrays():
    return {k: _host(k) for k in FUSE_HOST}


def _host(name):
    v = FUSE_HOST[name]
    return (C.c_int32 * len(v))(*v) if name.startswith("vb") else (C.c_double * len(v))(*v)


def fuse_args(_lib, p, host, kw, ws=256 * 1024, ws_bytes=1 << 40, ptrs=None):
    """the valid base call of tsdf_scenes.fuse_einval_calls with the changes kw; p: the address every device pointer gets (ptrs overrides)"""
    a = _lib.TsdfFuseArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz, a.accumulate = 2, 3, 4, 0, 3, 2, 2, 0
    a.voxel, a.trunc = 0.5, 2.0
    for k in ("depth", "rgb", "pose", "tsdf_sum", "weight", "color_sum"):
        setattr(a, k, p if ptrs is None else ptrs[k])
    a.view_begin_host, a.origin_host = C.addressof(host["vb"]), C.addressof(host["org"])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        else:
            setattr(a, k, C.addressof(host[v]) if isinstance(v, str) else v)
    return a


def surface_args(_lib, p, host, kw, ws=256 * 1024, ws_bytes=1 << 40, ptrs=None):
    a = _lib.TsdfSurfaceArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap = 2, 3, 2, 2, 1, 8
    a.voxel = 0.5
    for k in ("tsdf_sum", "weight", "color_sum", "points", "normals", "colors", "valid", "n_points"):
        setattr(a, k, p if ptrs is None else ptrs[k])
    a.origin_host = C.addressof(host["org"])
    a.workspace, a.workspace_bytes = ws, ws_bytes
    for k, v in kw.items():
        if k == "workspace_offset":
            a.workspace = ws + v
        else:
            setattr(a, k, C.addressof(host[v]) if isinstance(v, str) else v)
    return a
