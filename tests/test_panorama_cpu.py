"""CPU: the contract of relpose_frames_to_pano as tests/panorama_model.py states it -- anchored to the reference's
depth2pc and reproj_helper through the oracle, its support against the kinect window, the occlusion rule on exact values, the analytic
rooms of synth.render_frames, batch independence -- and the argument checks of the C ABI, which need no device."""
import ctypes as C

import numpy as np
import pytest

import panorama_model as M
from relativepose_amd import synth, util

H = 160


def _u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# ---- anchor to the reference ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scannet_frame():
    depth, rgb = synth.make_full_res_pair(31)                       # [1,2,480,640] with 15 % holes, uint8 [1,2,3,480,640]
    return depth[0, :1], np.ascontiguousarray(np.moveaxis(rgb[0, :1], 1, -1))


@pytest.fixture(scope="module")
def scannet_model(scannet_frame):
    dep, col = scannet_frame
    return M.frames_to_pano(dep[None], col[None], util.SCANNET_FRAME_SCALE, None, "scannet", H, None)


def test_scale_constants_are_the_reference_s():
    from oracle import geom_oracle as G
    assert util.SCANNET_FRAME_SCALE == (G.KINECT_FX, G.KINECT_FY)
    assert synth.SCANNET_FRAME_SCALE is util.SCANNET_FRAME_SCALE
    # a 640x480 camera with fx = fy = 570.94 px
    assert util.frame_scale(570.94, 570.94, 640, 480) == (2 * 570.94 / 640, 2 * 570.94 / 480)
    assert np.allclose(util.frame_scale(570.94, 570.94, 640, 480), util.SCANNET_FRAME_SCALE, rtol=2e-4)


def test_occupancy_is_the_reference_s(scannet_frame, scannet_model):
    from oracle import geom_oracle as G
    dep, _ = scannet_frame
    assert 0.1 < (dep == 0).mean() < 0.2
    ref = G._reproject(G.depth2pc(dep[0], "scannet")[0].T, None, H, "depth", "scannet")
    assert np.array_equal(scannet_model["valid"][0] != 0, ref != 0)
    assert (ref != 0).sum() > 5808                                  # the full frame reaches past the 66x88 kinect window


def test_reference_depth_lies_between_the_nearest_and_farthest_point_of_its_pixel(scannet_frame, scannet_model):
    from oracle import geom_oracle as G
    dep, col = scannet_frame
    ref = G._reproject(G.depth2pc(dep[0], "scannet")[0].T, None, H, "depth", "scannet").reshape(-1)
    pix, d, _ = M.view_points(dep, col, [util.SCANNET_FRAME_SCALE], None, "scannet", H, None)
    zmax = np.zeros(H * 4 * H, np.float32)
    np.maximum.at(zmax, pix, d)
    occ = ref != 0
    zmin = scannet_model["zmin"].reshape(-1).view(np.float32)
    assert (ref[occ] >= zmin[occ].astype(np.float64)).all() and (ref[occ] <= zmax[occ].astype(np.float64)).all()
    # and the fused depth is a gated mean: between the nearest point and (1 + gate) times it, one f32 rounding each
    fd = scannet_model["depth"].reshape(-1)
    assert (fd[occ] >= zmin[occ]).all() and (fd[occ] <= (zmin[occ] + zmin[occ] * np.float32(0.05)) * np.float32(1 + 2.0 ** -23)).all()


# ---- support ----------------------------------------------------------------------------------------------------------------------
def test_support_is_the_kinect_window():
    dep = np.full((1, 1, 480, 640), 2.5, np.float32)
    col = _u8((1, 1, 480, 640, 3), 3)
    y0, y1, x0, x1 = synth.observed_box("kinect", H)
    mask = np.zeros((H, 4 * H), bool)
    mask[y0:y1, x0:x1] = True
    boxed = M.frames_to_pano(dep, col, util.SCANNET_FRAME_SCALE, None, "scannet", H, (y0, y1, x0, x1))
    assert np.array_equal(boxed["valid"][0] != 0, mask)
    free = M.frames_to_pano(dep, col, util.SCANNET_FRAME_SCALE, None, "scannet", H, None)
    v = free["valid"][0] != 0
    assert v[mask].all() and v.sum() > mask.sum()
    ys, xs = np.nonzero(v & ~mask)                                  # the border: about one pixel further on each side
    assert ys.min() >= y0 - 2 and ys.max() <= y1 + 1 and xs.min() >= x0 - 2 and xs.max() <= x1 + 1
    # inside the window the box changes nothing
    for k in ("zmin", "count", "sum_z", "depth"):
        assert np.array_equal(boxed[k][0][mask], free[k][0][mask]), k


# ---- occlusion and gate: exact values ---------------------------------------------------------------------------------------------
def _two_frames(z2):
    dep = np.stack([np.full((48, 64), 2.0, np.float32), np.full((48, 64), z2, np.float32)])[None]
    col = np.stack([np.full((48, 64, 3), 40, np.uint8), np.full((48, 64, 3), 201, np.uint8)])[None]
    col[0, 0, :, :, 1] = 80
    m = M.frames_to_pano(dep, col, util.SCANNET_FRAME_SCALE, None, "scannet", H, None)
    one = M.frames_to_pano(dep[:, :1], col[:, :1], util.SCANNET_FRAME_SCALE, None, "scannet", H, None)
    v = m["valid"][0] != 0
    assert v.sum() > 1000 and np.array_equal(m["valid"], one["valid"])
    return m, one, v


def test_a_far_frame_is_occluded_by_a_near_one():
    m, one, v = _two_frames(3.0)
    assert (m["depth"][0][v] == np.float32(2.0)).all()
    assert np.array_equal(m["count"], one["count"]) and np.array_equal(m["sum_rgb"], one["sum_rgb"])
    assert (m["rgb"][0][:, v] == np.array([40, 80, 40], np.float32)[:, None] / np.float32(255)).all()


def test_a_frame_inside_the_gate_is_averaged_in():
    m, one, v = _two_frames(2.09)
    assert np.array_equal(m["count"][0][v], 2 * one["count"][0][v])
    q = int(np.rint(float(np.float32(2.0)) * 65536)) + int(np.rint(float(np.float32(2.09)) * 65536))
    assert (m["sum_z"][0][v] == one["count"][0][v].astype(np.uint64) * np.uint64(q)).all()
    assert (m["depth"][0][v] == np.float32(q / 2 / 65536.0)).all() and abs(float(m["depth"][0][v][0]) - 2.045) < 1e-5
    # (40 + 201) / 2 = 120.5 rounds up to 121, (80 + 201) / 2 = 140.5 to 141
    assert (m["rgb"][0][:, v] == np.array([121, 141, 121], np.float32)[:, None] / np.float32(255)).all()


def test_a_frame_outside_the_gate_is_not():
    m, one, v = _two_frames(2.11)
    for k in ("count", "sum_z", "sum_rgb", "depth", "rgb", "zmin"):
        assert np.array_equal(m[k], one[k]), k


# ---- analytic rooms ---------------------------------------------------------------------------------------------------------------
def _yaw(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = t
    return T


FRAME_POSES = [_yaw(-40.0, [0.05, -0.02, 0.03]), _yaw(0.0, [0.0, 0.0, 0.0]), _yaw(40.0, [-0.04, 0.03, 0.02])]
K_SUB = 5                      # samples per axis of a pixel's footprint
EPS_PX = 1e-3                  # the footprint is widened by this: a point's position carries the f32 rounding of its frame depth, moved
                               # through a frame translation of <= 0.07 m at >= 0.5 m: h/2 * 0.14 * 2^-24 < 1e-6 pixels, far inside


def _axis_depths(T, half, dataset, slot, u, v, h):
    """Per room axis the face depth at which the panorama ray through sub-pixel face coordinates (u, v) of `slot` meets the wall it is
    heading for (inf when it runs parallel), and the ray's direction sign along that axis."""
    d_face = np.stack([(u / h - 0.5) * 2, (0.5 - v / h) * 2, -np.ones_like(u)], -1)
    d_w = (d_face @ synth.face_rotation(dataset, slot).T) @ T[:3, :3].T
    tw = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(d_w > 0, (half - tw) / d_w, (-half - tw) / d_w)
    s[~np.isfinite(s)] = np.inf
    return s, np.sign(d_w)


def _depth_bounds(T, half, dataset, ys, xs, h):
    """[lo, hi] that hold the analytic panorama depth over the footprint of every pixel (ys, xs): the sub-pixel positions that round to
    it -- [c - 1/2, c + 1/2], the last column / row also takes what is clipped to it -- sampled on a K_SUB x K_SUB grid.  The depth is
    the minimum over the three axes of s_a = const / (affine in (u, v)), and a linear-fractional function takes its extremes over a
    rectangle at the corners.  So the minimum over the samples IS the infimum; and over every sub-cell on which an axis' direction keeps
    its sign the maximum of s_a is at the cell's corners, the depth is <= s_a, hence sup <= max over sub-cells of min over such axes of
    the corner maximum: no slack for the sampling is needed on either side."""
    slot = xs // h
    cx, cy = (xs - slot * h).astype(np.float64), ys.astype(np.float64)
    lo_u, hi_u = cx - 0.5 - EPS_PX, np.where(cx == h - 1, h + EPS_PX, cx + 0.5 + EPS_PX)
    lo_v, hi_v = cy - 0.5 - EPS_PX, np.where(cy == h - 1, h + EPS_PX, cy + 0.5 + EPS_PX)
    f = np.linspace(0, 1, K_SUB)
    u = (lo_u[:, None, None] + (hi_u - lo_u)[:, None, None] * f[None, None, :]) + 0 * f[None, :, None]
    v = (lo_v[:, None, None] + (hi_v - lo_v)[:, None, None] * f[None, :, None]) + 0 * f[None, None, :]
    lo, hi = np.zeros(len(ys)), np.zeros(len(ys))
    for sl in range(4):
        k = slot == sl
        if not k.any():
            continue
        s, sg = _axis_depths(T, half, dataset, sl, u[k], v[k], h)              # [m, K, K, 3]
        lo[k] = s.min(-1).min((1, 2))
        corners = [(slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None)), (slice(1, None), slice(None, -1)), (slice(1, None), slice(1, None))]
        cmax = np.max([s[:, a, b] for a, b in corners], 0)                     # [m, K-1, K-1, 3]
        same = np.all([sg[:, a, b] == sg[:, :-1, :-1] for a, b in corners], 0) & (sg[:, :-1, :-1] != 0)
        hi[k] = np.where(same, cmax, np.inf).min(-1).max((1, 2))
    return lo, hi


@pytest.mark.parametrize("dataset,F", [("scannet", 1), ("suncg", 1), ("scannet", 3), ("suncg", 3)])
def test_fused_depth_lies_inside_the_analytic_depth_of_its_footprint(dataset, F):
    rs = np.random.RandomState(77)
    half = np.array([2.6, 1.9, 3.1])
    T = synth.random_rigid(rs, np.pi, 0.4)
    fp = [FRAME_POSES[1:2] if F == 1 else FRAME_POSES]
    Hf, Wf = (480, 640) if (dataset, F) == ("scannet", 1) else (240, 320)
    dep, col = synth.render_frames(rs, [T], half, Hf, Wf, frame_poses=fp)
    assert dep.shape == (1, F, Hf, Wf) and col.shape == (1, F, Hf, Wf, 3) and col.dtype == np.uint8 and (dep > 0.5).all()
    m = M.frames_to_pano(dep, col, util.SCANNET_FRAME_SCALE, np.stack(fp), dataset, H, None)
    ys, xs = np.nonzero(m["valid"][0])
    slots = set((xs // H).tolist())
    assert len(ys) > 5000 and (len(slots) >= 2 if F == 3 else len(slots) == 1)   # three yawed frames cross a face seam
    lo, hi = _depth_bounds(T, half, dataset, ys, xs, H)
    got = m["depth"][0][ys, xs].astype(np.float64)
    # slack: half a step of the 2^-16 quantisation of every summed depth; the f32 roundings of the rendered frame depth, of the face
    # depth d and of the output (3 x 2^-24 relative, taken as 2^-22); 1e-9 for the float64 geometry
    slack = 2.0 ** -17 + got * 2.0 ** -22 + 1e-9
    assert (got >= lo - slack).all(), float((lo - got).max())
    assert (got <= hi + slack).all(), float((got - hi).max())
    assert np.isfinite(hi).all() and np.median(hi - lo) < 0.1                    # the bounds bind
    # the colours are the texture's, up to its variation over the footprint and the quantisation
    assert m["rgb"].min() >= 0 and m["rgb"].max() <= 1


# ---- batch independence -----------------------------------------------------------------------------------------------------------
def test_a_view_does_not_depend_on_its_batch():
    rs = np.random.RandomState(9)
    dep = rs.uniform(0.5, 4.0, (3, 2, 30, 40)).astype(np.float32)
    dep[rs.rand(*dep.shape) < 0.2] = 0
    dep[0, 0, 0, :4] = [np.nan, np.inf, -1.0, -np.inf]              # no data either
    col = _u8((3, 2, 30, 40, 3), 10)
    pose = np.stack([np.stack([synth.random_rigid(rs, np.pi, 0.3) for _ in range(2)]) for _ in range(3)])
    sc = rs.uniform(0.8, 2.5, (3, 2, 2))
    full = M.frames_to_pano(dep, col, sc, pose, "matterport", 16, None)
    assert full["count"].sum() > 500 and len(set((np.nonzero(full["valid"])[2] // 16).tolist())) == 4
    for v in range(3):
        alone = M.frames_to_pano(dep[v:v + 1], col[v:v + 1], sc[v:v + 1], pose[v:v + 1], "matterport", 16, None)
        for k in full:
            assert np.array_equal(alone[k][0], full[k][v]), (v, k)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_abi_rejects_invalid_arguments_without_a_device():
    from relativepose_amd import _lib
    L = _lib.lib()
    assert L.relpose_frames_to_pano(None) == -1
    assert L.relpose_frames_to_pano_workspace_bytes(2, 160) >= 2 * 160 * 640 * 28
    assert L.relpose_frames_to_pano_workspace_bytes(2, 161) == 0 and L.relpose_frames_to_pano_workspace_bytes(0, 160) == 0

    def call(**kw):
        a = _lib.FramesToPanoArgs()
        a.struct_size = C.sizeof(a)
        a.n_views, a.n_frames, a.frame_h, a.frame_w, a.h, a.dataset, a.gate = 1, 1, 48, 64, 160, 2, 0.05
        a.box[:] = (-1, -1, -1, -1)
        for k in ("depth", "rgb", "scale", "out_depth", "out_rgb", "out_valid", "workspace"):
            setattr(a, k, 4096)                                     # never dereferenced on the host
        a.workspace_bytes = L.relpose_frames_to_pano_workspace_bytes(1, 160)
        for k, val in kw.items():
            if k == "box":
                a.box[:] = val
            else:
                setattr(a, k, val)
        return L.relpose_frames_to_pano(C.byref(a))
    assert call(n_frames=0) == -1 and call(h=161) == -1 and call(gate=-0.01) == -1 and call(gate=float("nan")) == -1
    assert call(depth=None) == -1 and call(out_valid=None) == -1 and call(workspace=None) == -1 and call(scale=None) == -1
    assert call(box=(0, 161, 0, 640)) == -1 and call(box=(0, 160, 0, 641)) == -1 and call(box=(-1, 160, 0, 640)) == -1
    assert call(box=(10, 5, 0, 640)) == -1 and call(dataset=3) == -1 and call(workspace_bytes=16) == -1
    assert call(struct_size=8) == -1 and call(n_frames=4096, frame_h=480, frame_w=640) == -1
    assert call(workspace=4100) == -1                               # sum_z (u64) lies at the workspace's base
    # a launch of 2^32 threads or more: 65520 frames of 1024x1024 (2^24 pixels per view are still allowed); 65535 views at h = 8192
    big = 1 << 50
    assert call(n_views=4095, n_frames=16, frame_h=1024, frame_w=1024, workspace_bytes=big) == -1
    assert call(n_views=65535, h=8192, workspace_bytes=big) == -1


def test_cli_takes_from_frames_for_scannet_ours_only():
    from relativepose_amd import evaluation
    args = evaluation._cli_parser_completion().parse_args(["--from-frames", "--dataset", "scannet"])
    assert args.from_frames and not evaluation._cli_parser_completion().parse_args([]).from_frames
    for argv in (["--from-frames", "--dataset", "suncg"], ["--from-frames", "--dataset", "scannet", "--method", "gs"],
                 ["--from-frames", "--dataset", "scannet", "--gpus", "2"], ["--from-frames", "--dataset", "scannet", "--keypoint-mode", "reference"]):
        with pytest.raises(SystemExit):
            evaluation.main(argv)
