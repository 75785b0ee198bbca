"""The pinned inputs of the rendering tests (CPU and GPU): the closed rooms of tests/align_scenes.py and a pinned scannet room of
tests/tsdf_scenes.py fused by the model under the true poses (all views, and leave-one-out), a three-scene batch, the hand-built edge
volume and the invalid calls.  Every model result is computed once per process and must be left unchanged."""
import ctypes as C
import functools

import numpy as np

import align_scenes as AS
import render_model as RM
import tsdf_scenes as TS

STATE_KEYS = ("tsdf_sum", "weight", "color_sum")
FILL = {"depth": -7.5, "cls": 77, "normal": 9.25, "color": -3.0, "n_evaluated": -9}      # what the outputs are pre-filled with


@functools.lru_cache(maxsize=None)
def full_state(name):
    """the model's volume of every view of a scene under the true poses, with colours"""
    return TS.fuse_model(AS.scene(name))


@functools.lru_cache(maxsize=None)
def loo_state(name, v):
    """... of every view but v"""
    c = AS.scene(name)
    return TS.fuse_model(c, order=[u for u in range(len(c["depth"])) if u != v])


def case(name, views=None, state=None):
    """a scene's views (all, or the listed ones) against one volume (default: the fusion of all views) as a render case"""
    c = AS.scene(name)
    vs = list(range(len(c["R"]))) if views is None else list(views)
    step, n_steps = RM.steps_for(c["dims"], c["voxel"])
    return {"state": full_state(name) if state is None else state, "origin": c["origin"], "dims": c["dims"], "voxel": c["voxel"], "ds": c["ds"],
            "h": c["h"], "pose": c["R"][vs], "scene_of_view": np.zeros(len(vs), np.int32), "d_min": 0.0, "step": step, "n_steps": n_steps,
            "min_weight": 1}


def model_of(cs, skip=True, clip=True, color=True, **kw):
    p = {k: cs[k] for k in ("d_min", "step", "n_steps", "min_weight")}
    p.update(kw)
    return RM.render(cs["state"], cs["origin"], cs["voxel"], cs["pose"], cs["ds"], cs["h"], cs["scene_of_view"], skip=skip, clip=clip, color=color, **p)


@functools.lru_cache(maxsize=None)
def room_model(name, skip=True):
    """every view of a scene against the fusion of all views"""
    return model_of(case(name), skip=skip)


@functools.lru_cache(maxsize=None)
def loo_model(name, v):
    """view v against its leave-one-out volume"""
    return model_of(case(name, [v], loo_state(name, v)))


# ---------------------------------------------------------------------------------------------- accuracy against the analytic room
def analytic_normals(c, v):
    """the camera-frame inward normal of the wall each pixel of view v sees, from its analytic depth: [3,h,4h]"""
    h = c["h"]
    d = c["depth"][v].reshape(-1).astype(np.float64)
    p = RM.rays(h, c["ds"]) * d[:, None]
    Wm = np.linalg.inv(c["R"][v])
    q = p @ Wm[:3, :3].T + Wm[:3, 3]
    a = np.abs(np.abs(q) - c["half"][None]).argmin(1)
    n = np.zeros_like(q)
    n[np.arange(len(q)), a] = -np.sign(q[np.arange(len(q)), a])
    return (n @ c["R"][v][:3, :3].T).T.reshape(3, h, 4 * h)


def accuracy(name, out, views):
    """rendered views `views` of a closed room against their own analytic inputs -> (median, p90 of |rendered - analytic| in voxels over
    pixels where both have data, coverage = hits / pixels with analytic data, median angle in degrees between the normals)"""
    c = AS.scene(name)
    err, ang, hits, meas = [], [], 0, 0
    for n, v in enumerate(views):
        ref = c["depth"][v]
        have = np.isfinite(ref) & (ref > 0)
        hit = out["cls"][n] == RM.HIT
        both = hit & have
        err.append(np.abs(out["depth"][n][both].astype(np.float64) - ref[both].astype(np.float64)) / c["voxel"])
        cosine = (out["normal"][n].astype(np.float64) * analytic_normals(c, v)).sum(0)[both]
        ang.append(np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0))))
        hits, meas = hits + int(hit.sum()), meas + int(have.sum())
    err, ang = np.concatenate(err), np.concatenate(ang)
    return float(np.median(err)), float(np.percentile(err, 90)), hits / meas, float(np.median(ang))


# ---------------------------------------------------------------------------------------------- the batch
@functools.lru_cache(maxsize=None)
def batch():
    """Three volumes of the closed h = 16 room's shape: (0) all three views, (1) all but view 1, (2) all but view 0; scene 1 gets no view.
    Views: 0 -> scene 0; 1 -> scene 2; 2: view 2's pose moved 100 m away (every sample outside) -> scene 0; 3: view 0 again -> scene 2 (two
    views share a volume)."""
    c = AS.closed_room(16)
    sts = [full_state("closed16"), loo_state("closed16", 1), loo_state("closed16", 0)]
    b = case("closed16")
    b["state"] = {k: np.concatenate([s[k] for s in sts]) for k in STATE_KEYS}
    far = c["R"][2].copy()
    far[0, 3] += 100.0
    b["origin"] = np.concatenate([c["origin"]] * 3)
    b["pose"] = np.stack([c["R"][0], c["R"][1], far, c["R"][0]])
    b["scene_of_view"] = np.array([0, 2, 0, 2], np.int32)
    return b


def batch_member(v):
    """view v of batch() with its own volume as a one-scene case"""
    b = batch()
    s = int(b["scene_of_view"][v])
    m = dict(b)
    m["state"] = {k: b["state"][k][s:s + 1] for k in STATE_KEYS}
    m["origin"], m["pose"], m["scene_of_view"] = b["origin"][s:s + 1], b["pose"][v:v + 1], np.zeros(1, np.int32)
    return m


# ---------------------------------------------------------------------------------------------- the hand-built edge volume
EDGE_AXIS = {"hit_s0": (0, 2, 2), "last_cell": (0, 2, 10), "no_bridge": (1, 2, 2), "back_face": (2, 2, 10)}      # view, row, column at h = 4


@functools.lru_cache(maxsize=None)
def edge_case(ds="suncg", h=4):
    """A 4 x 3 x 5 volume written by hand, min_weight 2, voxel 0.5, origin (-1.25, -0.75, -1.75): voxel centres at multiples of 0.5 plus
    (-1, -0.5, -1.5); step 0.25, so every second sample of an axis ray has an integer u.  t = tsdf_sum / 3 / 32768 with weight 3.  The
    voxel column (x = 2, y = 1) holds t = -0.7, -0.5, 0, 0.5, 0.8 from z = 0 to 4; the column (x = 1, y = 1) holds -0.5, -0.3, an unknown
    voxel (weight = min_weight - 1), 0.4, 0.6.  All poses have the identity rotation, so the centre rays of the faces run along the axes (two
    zero direction components in the clip).  At h = 4 and suncg (EDGE_AXIS names the pixels):
      view 0  camera at the world origin, the centre of voxel (2, 1, 3), inside the box.  Looking along -z: u_z = 3 - k / 2: 0.5, 0.25, then
              t_2 = 0 exactly (no crossing at the pair (1, 2)), then -0.25: a hit at the pair (2, 3) with s = 0, depth 0.5 exactly.  Looking
              along +z: u_z = 3 and 3.5 lie in the last cell, u_z = 4 = nz - 1 is one past it: two evaluations, a miss.
      view 1  camera at (-0.5, 0, 1.5), outside the box, looking along -z down the column (1, 1): 0.5 and 0.4 in the cell above the unknown
              voxel, four invalid samples in the two cells that touch it, -0.4 and -0.5 below: no pair of valid samples changes sign, a miss.
      view 2  camera at (0, 0, -1.5), the centre of voxel (2, 1, 0), inside the solid; looking along +z: -0.7, -0.6, -0.5, -0.25, 0: the first
              valid sample is negative and the pair (3, 4) leaves the solid: a back face.
      view 3  a NaN in the pose, view 4 an inf: every sample is out of range, all misses and zero outputs."""
    nx, ny, nz = 4, 3, 5
    rs = np.random.RandomState(3)
    w = np.full((nz, ny, nx), 3, np.int32)
    t = (rs.randint(-30000, 30000, (nz, ny, nx)) * 3).astype(np.int32)
    t[:, 1, 2] = np.array([-22938, -16384, 0, 16384, 26214]) * 3
    t[:, 1, 1] = np.array([-16384, -9830, 777, 13107, 19661]) * 3
    w[2, 1, 1] = 1                                      # min_weight - 1
    col = rs.randint(0, 256 * 3, (3, nz, ny, nx)).astype(np.uint32)
    pose = np.stack([np.eye(4)] * 5)
    pose[1][:3, 3] = [0.5, 0.0, -1.5]
    pose[2][:3, 3] = [0.0, 0.0, 1.5]
    pose[3][1, 2] = np.nan
    pose[4][0, 0] = np.inf
    state = {"tsdf_sum": t[None].copy(), "weight": w[None].copy(), "color_sum": col[None].copy()}
    return {"state": state, "origin": np.array([[-1.25, -0.75, -1.75]]), "dims": (nx, ny, nz), "voxel": 0.5, "ds": ds, "h": h, "pose": pose,
            "scene_of_view": np.zeros(5, np.int32), "d_min": 0.0, "step": 0.25, "n_steps": 15, "min_weight": 2}


@functools.lru_cache(maxsize=None)
def flat_case():
    """the edge case with its y = 1 layer alone: a volume with a dimension of 1 has no cells"""
    e = dict(edge_case())
    e["state"] = {k: np.ascontiguousarray(v[..., 1:2, :]) for k, v in e["state"].items()}
    e["dims"] = (4, 1, 5)
    return e


# ---------------------------------------------------------------------------------------------- invalid calls
def einval_calls():
    """(name, {field: value}) changes of a valid base call (2 scenes, 3 views at h = 4, a 3 x 2 x 2 volume, scene_of_view 0 1 1, 6 steps of 0.25,
    skip 1, every output) that must each return RELPOSE_EINVAL.  A str value names an alternative host array."""
    return [("no_tsdf", {"tsdf_sum": 0}), ("no_weight", {"weight": 0}), ("no_pose", {"pose": 0}), ("no_origin", {"origin_host": 0}),
            ("no_scene_of_view", {"scene_of_view_host": 0}), ("no_depth", {"depth": 0}), ("no_cls", {"cls": 0}), ("no_workspace", {"workspace": 0}),
            ("color_without_color_sum", {"color_sum": 0}), ("dataset_low", {"dataset": -1}), ("dataset_high", {"dataset": 3}),
            ("reserved", {"reserved0": 1}), ("voxel_0", {"voxel": 0.0}), ("voxel_neg", {"voxel": -0.5}), ("voxel_nan", {"voxel": float("nan")}),
            ("voxel_inf", {"voxel": float("inf")}), ("d_min_neg", {"d_min": -1e-9}), ("d_min_nan", {"d_min": float("nan")}),
            ("d_min_inf", {"d_min": float("inf")}), ("step_0", {"step": 0.0}), ("step_neg", {"step": -0.25}), ("step_nan", {"step": float("nan")}),
            ("step_inf", {"step": float("inf")}), ("steps_0", {"n_steps": 0}), ("steps_neg", {"n_steps": -4}), ("steps_65537", {"n_steps": 65537}),
            ("skip_2", {"skip": 2}), ("skip_neg", {"skip": -1}), ("min_weight_0", {"min_weight": 0}), ("min_weight_neg", {"min_weight": -1}),
            ("scenes_0", {"n_scenes": 0}), ("scenes_neg", {"n_scenes": -1}), ("views_0", {"n_views": 0}), ("views_neg", {"n_views": -2}),
            ("h_0", {"h": 0}), ("h_odd", {"h": 5}), ("h_big", {"h": 8194}), ("pixels_2_31", {"h": 8192, "n_views": 8}), ("nx_0", {"nx": 0}),
            ("ny_neg", {"ny": -1}), ("nz_0", {"nz": 0}), ("voxels_2_31", {"nx": 2048, "ny": 1024, "nz": 1024}),
            ("colours_2_31", {"nx": 1024, "ny": 1024, "nz": 700, "n_scenes": 1}), ("scene_low", {"scene_of_view_host": "sov_low"}),
            ("scene_high", {"scene_of_view_host": "sov_high"}), ("origin_nan", {"origin_host": "org_nan"}), ("origin_inf", {"origin_host": "org_inf"}),
            ("workspace_small", {"workspace_bytes": 255}), ("workspace_unaligned", {"workspace_offset": 8}), ("struct_small", {"struct_size": 16})]


POINTERS = ("tsdf_sum", "weight", "color_sum", "pose", "depth", "cls", "normal", "color", "n_evaluated")


def render_args(_lib, p, host, kw, ws=256 * 1024, ws_bytes=1 << 40, ptrs=None):
    """the valid base call of einval_calls with the changes kw; p: the address every device pointer gets (ptrs overrides)"""
    a = _lib.TsdfRenderArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz, a.min_weight, a.n_steps, a.skip = 2, 3, 4, 0, 3, 2, 2, 1, 6, 1
    a.voxel, a.d_min, a.step = 0.5, 0.0, 0.25
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
