"""CPU: the TSDF contract's numpy model (tests/tsdf_model.py) agrees with its own plain-loop statement, the integer volume does not depend
on the order of the views or on how they are split over accumulating calls, the surface of the pinned rooms lies on the analytic walls
within the pinned distances and moves away under a perturbed pose, the hand-built edge cases get what the contract gives them, save_ply
round-trips, and the host layers around relpose_tsdf_fuse / relpose_tsdf_surface -- operator registration, workspace queries, argument
validation -- work without a GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import tsdf_model as TM
import tsdf_scenes as TS

# Measured with the model on the pinned rooms (median, p90, max of the surface's distance to the nearest wall plane, in voxels; DESIGN.md
# §4.16 holds the same numbers).  The pins are the measured values x 1.25.
MEASURED = {("suncg", 16): (0.05134, 0.28742, 0.97712), ("suncg", 32): (0.06374, 0.38322, 1.30325), ("scannet", 16): (0.05227, 0.28918, 0.97712)}


def args_of(c):
    return c["depth"], c["rgb"], c["R"], c["view_begin"], c["origin"], c["dims"], c["voxel"], c["ds"], c["trunc"]


@pytest.mark.parametrize("case", ["1x1x2", "5x3x2", "edge_suncg", "edge_matterport", "edge_scannet", "batch_crop"])
def test_fuse_loops_equal_the_vectorised_form(case):
    if case.startswith("edge_"):
        c = TS.edge_case(case[5:])
    elif case == "batch_crop":
        c = dict(TS.batch())
        c["dims"] = (5, 4, 3)                                                  # three scenes (3, 0 and 2 views) around the -x wall
        c["origin"] = c["origin"] + np.array([[2 * 0.25, 10 * 0.25, 9 * 0.25]])
    else:
        c = TS.tiny(case)
    a, b = TM.fuse(*args_of(c)), TM.fuse_loops(*args_of(c))
    assert TS.differ(a, b, TS.STATE_KEYS) == []
    assert a["weight"].max() > 0 and a["weight"].max() <= len(c["depth"])
    assert (np.abs(a["tsdf_sum"].astype(np.int64)) <= 32768 * a["weight"].astype(np.int64)).all()
    assert (a["color_sum"] <= 255 * a["weight"][:, None].astype(np.uint32)).all()
    if case == "batch_crop":
        assert (a["weight"][1] == 0).all() and (a["tsdf_sum"][1] == 0).all()   # the scene without a view


@pytest.mark.parametrize("case", ["1x1x2", "5x3x2", "edge_suncg", "edge_state", "room_crop"])
def test_surface_loops_equal_the_vectorised_form(case):
    mw = 1
    if case == "edge_state":
        e = TS.edge_state()
        ts, wt, cs, origin, voxel, mw = e["tsdf_sum"][0], e["weight"][0], e["color_sum"][0], e["origin"][0], e["voxel"], e["min_weight"]
    elif case == "room_crop":
        c, st = TS.room("suncg", 16), TS.room_state("suncg", 16)
        ts, wt, cs = (st[k][0][..., 8:20, 0:9, 0:8] for k in TS.STATE_KEYS)
        origin, voxel = c["origin"][0], c["voxel"]
    else:
        c = TS.edge_case("suncg") if case == "edge_suncg" else TS.tiny(case)
        st = TS.fuse_model(c)
        ts, wt, cs, origin, voxel = st["tsdf_sum"][0], st["weight"][0], st["color_sum"][0], c["origin"][0], c["voxel"]
    a, b = TM.surface(ts, wt, cs, origin, voxel, mw), TM.surface_loops(ts, wt, cs, origin, voxel, mw)
    assert a["n"] == b["n"] >= 1
    assert TS.differ(a, b, ("points", "normals", "colors", "edge")) == []
    lin = a["edge"][:, 0] * 3 + a["edge"][:, 1]
    assert (np.diff(lin) > 0).all()                                            # ascending voxel, then axis
    nn = np.linalg.norm(a["normals"], axis=1)
    assert (np.abs(nn[nn > 0] - 1) < 1e-12).all()
    assert np.isfinite(a["points"]).all() and np.isfinite(a["colors"]).all()
    no_col = TM.surface(ts, wt, None, origin, voxel, mw)
    assert no_col["colors"] is None and TS.differ(no_col, a, ("points", "normals", "edge")) == []


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS)
def test_volume_is_independent_of_view_order_and_of_the_split(ds, h):
    c, want = TS.room(ds, h), TS.room_state(ds, h)
    M = len(c["depth"])
    orders = list(itertools.permutations(range(M))) if M <= 3 else [tuple(range(M))[::-1], (2, 0, 3, 1), (1, 3, 0, 2)]
    for order in orders:
        assert TS.differ(TS.fuse_model(c, order=order), want, TS.STATE_KEYS) == [], order
    for cut in range(0, M + 1):                                                # one call, or accumulate over a split (an empty part included)
        st = None
        for part in (range(0, cut), range(cut, M)):
            o = list(part)
            st = TM.fuse(c["depth"][o], c["rgb"][o], c["R"][o], np.array([0, len(o)]), c["origin"], c["dims"], c["voxel"], ds, c["trunc"], state=st)
        assert TS.differ(st, want, TS.STATE_KEYS) == [], cut


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS)
def test_surface_lies_on_the_analytic_walls(ds, h):
    c, st = TS.room(ds, h), TS.room_state(ds, h)
    assert c["dims"] == tuple(int(np.ceil(2 * (c["half"][a] + 3 * c["voxel"]) / c["voxel"])) for a in range(3))
    assert any(d % 64 for d in c["dims"]) and np.prod(c["dims"]) % 256 != 0    # no multiple of the workgroup shape
    cap, out = TS.room_surface(ds, h)
    n = int(out["n_points"][0])
    assert n == cap - 5 and n > 2000
    got = TS.wall_stats(out["points"][0, :n], c["half"], c["voxel"])
    print("wall error (median, p90, max) in voxels", ds, h, got)
    for g, m in zip(got, MEASURED[(ds, h)]):
        assert g <= 1.25 * m
        assert g >= 0.75 * m                                                   # and the table in DESIGN.md is still what the model gives
    # the normals point into the room: away from the wall the point lies on
    p, nrm = out["points"][0, :n], out["normals"][0, :n]
    a = np.abs(np.abs(p) - c["half"][None]).argmin(1)
    inward = -np.sign(p[np.arange(n), a]) * nrm[np.arange(n), a]
    assert (inward > 0).mean() > 0.97 and np.median(inward) > 0.9
    assert (out["colors"][0, :n] >= 0).all() and (out["colors"][0, :n] <= 1).all()


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS)
def test_a_perturbed_pose_moves_the_surface_off_the_walls(ds, h):
    c = TS.room(ds, h)
    true = TS.wall_stats(TS.surface_points(TS.room_state(ds, h), c), c["half"], c["voxel"])[0]
    bad = TS.wall_stats(TS.surface_points(TS.fuse_model(c, R=TS.perturbed(c)), c), c["half"], c["voxel"])[0]
    print("median wall error, true and perturbed pose", ds, h, true, bad)
    assert bad > true


@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
def test_fuse_edge_case_gets_what_the_contract_gives(ds):
    c = TS.edge_case(ds)
    h, (nx, ny, nz) = c["h"], c["dims"]
    ctr = TM.centres(c["origin"][0], c["dims"], c["voxel"])
    assert np.array_equal(np.unique(ctr[:, 0]), np.arange(-2, 2, 0.25)) and np.array_equal(np.unique(ctr[:, 2]), [-2.0, -1.75, -1.5])
    import visibility_model as VM
    per_view = [TM.fuse_view(ctr, c["depth"][v], c["rgb"][v], c["R"][v], ds, c["trunc"]) for v in range(len(c["depth"]))]
    # view 0: the z = -2 layer
    pix, d = VM.project(VM.move(ctr, c["R"][0]), h, ds)
    layer = np.nonzero((ctr[:, 2] == -2.0) & (pix >= 0))[0]
    assert pix[(ctr[:, 2] == -2.0) & (ctr[:, 0] == -2.0)].max() == -1         # |x / z| = 1 exactly: no face takes the voxel
    xn = ctr[layer, 0] / 2.0
    assert ((np.abs((xn + 1) * 0.5 * h % 1 - 0.5) == 0).sum()) >= 32          # exact half pixels
    assert (d[layer] == 2.0).all() and len(set(pix[layer].tolist())) >= len(TS.SPECIAL_DEPTHS)
    dt, dw, _ = per_view[0]
    seen = {}
    for e in layer:
        z = c["depth"][0].reshape(-1)[pix[e]]
        seen[np.float32(z).tobytes()] = (int(dt[e]), int(dw[e]))
    key = lambda v: np.float32(v).tobytes()
    assert seen[key(1.0)] == (-32768, 1)                                       # sdf = -trunc exactly: integrated, t = -1
    assert seen[key(TS.SPECIAL_DEPTHS[1])] == (0, 0)                           # one float32 ulp nearer: sdf < -trunc, skipped
    assert seen[key(TS.SPECIAL_DEPTHS[2])] == (-32768, 1)                      # one ulp farther: integrated; t = -1 + 2^-23 rounds to -32768
    for z in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert seen[key(z)] == (0, 0), z
    assert seen[key(3.0e38)] == (32768, 1) and seen[key(2.0)] == (0, 1) and seen[key(2.5)] == (16384, 1) and seen[key(1.5)] == (-16384, 1)
    # view 1: d = 32768 is outside, 32767.5 inside
    dt, dw, _ = per_view[1]
    assert (dw[ctr[:, 2] == -2.0] == 0).all() and (dw[ctr[:, 2] == -1.75] == 1).all() and (dw[ctr[:, 2] == -1.5] == 1).all()
    assert set(dt[ctr[:, 2] == -1.75].tolist()) == {llr(32767.0 - 32767.75)} and set(dt[ctr[:, 2] == -1.5].tolist()) == {llr(32767.0 - 32767.5)}
    # views 2 and 3: NaN / inf in the pose
    assert per_view[2][1].sum() == 0
    assert per_view[3][1].sum() < per_view[0][1].sum()
    assert per_view[4][1].sum() > 10
    # colours: clamped, NaN counts 0
    assert TM.quantise_rgb(np.array([-0.5, 0.0, 0.5, 1.0, 1.5, np.nan], np.float32)).tolist() == [0, 0, 128, 255, 255, 0]
    st = TS.fuse_model(c)
    assert st["color_sum"].max() <= 255 * st["weight"].max() and st["color_sum"].max() > 255


def llr(t):
    return int(np.rint(max(min(t, 1.0), -1.0) * 32768.0))


def test_surface_edge_state_gets_what_the_contract_gives():
    e = TS.edge_state()
    r = TM.surface(e["tsdf_sum"][0], e["weight"][0], e["color_sum"][0], e["origin"][0], e["voxel"], e["min_weight"])
    edges = [tuple(x) for x in r["edge"].tolist()]
    assert (0, 0) in edges and (1, 0) in edges and (2, 0) not in edges         # 0 | -3000, -3000 | 0, 0 | 0
    k0, k1 = edges.index((0, 0)), edges.index((1, 0))
    o, vx = e["origin"][0], e["voxel"]
    assert r["points"][k0, 0] == o[0] + ((0.0 + 0.5) + 0.0) * vx and r["points"][k1, 0] == o[0] + ((1.0 + 0.5) + 1.0) * vx
    nx, ny, nz = e["dims"]
    lonely = (1 * ny + 3) * nx + 5
    assert all(a != lonely for a, _ in edges)                                  # no known neighbour: no crossing ...
    known, t = TM.values(e["tsdf_sum"][0], e["weight"][0], e["min_weight"])
    g = TM.gradient(known, t)
    assert known[1, 3, 5] and all(g[c][1, 3, 5] == 0 for c in range(3))        # ... and a zero gradient
    unknown = (1 * ny + 1) * nx + 1
    assert all(a != unknown and not (a + (1, nx, nx * ny)[c] == unknown) for a, c in edges)      # weight 1 < min_weight 2
    assert len(TM.surface(e["tsdf_sum"][0], e["weight"][0], None, o, vx, 1)["edge"]) != len(edges)
    cap = 10
    assert r["n"] > cap
    st = {k: e[k] for k in TS.STATE_KEYS}
    out = TM.surface_outputs(st, e["origin"], vx, e["min_weight"], cap, TS.FILL)
    assert out["n_points"][0] == r["n"] and out["valid"].all() and TS.bits_equal(out["points"][0], r["points"][:cap])
    out = TM.surface_outputs(st, e["origin"], vx, e["min_weight"], r["n"] + 3, TS.FILL)
    assert out["valid"][0].tolist() == [1] * r["n"] + [0] * 3 and (out["points"][0, r["n"]:] == TS.FILL["points"]).all()
    # a zero normal where the interpolated gradient vanishes
    ts = np.zeros((1, 1, 2), np.int32)
    ts[0, 0] = [100, -100]
    z = TM.surface(ts, np.ones((1, 1, 2), np.int32), None, [0, 0, 0], 1.0)
    assert z["n"] == 1 and z["points"][0].tolist() == [1.0, 0.5, 0.5] and z["normals"][0, 0] == -1.0 and (z["normals"][0, 1:] == 0).all()


def test_save_ply_round_trip(tmp_path):
    from relativepose_amd import util
    rs = np.random.RandomState(3)
    N = 37
    p, n, c = rs.randn(N, 3), rs.randn(N, 3), rs.uniform(-0.2, 1.2, (N, 3)).astype(np.float32)
    for name, kw, fields in (("all.ply", dict(normals=n, colors=c), 9), ("points.ply", {}, 3), ("colors.ply", dict(colors=c), 6)):
        path = tmp_path / name
        assert util.save_ply(str(path), p, **kw) == N
        raw = path.read_bytes()
        head, payload = raw.split(b"end_header\n", 1)
        lines = head.decode("ascii").split("\n")
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == f"element vertex {N}"
        props = [ln.split() for ln in lines[3:] if ln]
        assert all(pr[0] == "property" for pr in props) and len(props) == fields
        dt = np.dtype([(pr[2], {"float": "<f4", "uchar": "u1"}[pr[1]]) for pr in props])
        assert len(payload) == N * dt.itemsize
        rec = np.frombuffer(payload, dt)
        assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), p.astype(np.float32))
        if "normals" in kw:
            assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), n.astype(np.float32))
        if "colors" in kw:
            assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        util.save_ply(str(tmp_path / "bad.ply"), p, normals=n[:5])
    assert util.save_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3))) == 0


def test_operators_are_registered_with_meta_kernels():
    import torch
    from relativepose_amd import ops
    assert "tsdf_fuse" in ops.OPS and "tsdf_surface" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    depth, rgb, pose = m(5, 16, 64, dt=torch.float32), m(5, 3, 16, 64, dt=torch.float32), m(5, 4, 4, dt=torch.float64)
    ts, wt, cs = torch.ops.relpose.tsdf_fuse(depth, rgb, pose, m(4, dt=torch.int32), m(3, 3, dt=torch.float64), [20, 34, 27], 0.25, 0)
    assert ts.shape == wt.shape == (3, 27, 34, 20) and ts.dtype == wt.dtype == cs.dtype == torch.int32 and cs.shape == (3, 3, 27, 34, 20)
    ts, wt, cs0 = torch.ops.relpose.tsdf_fuse(depth, None, pose, m(4, dt=torch.int32), m(3, 3, dt=torch.float64), [20, 34, 27], 0.25, 2, 1.0)
    assert cs0.numel() == 0
    p, n, c, v, k = torch.ops.relpose.tsdf_surface(ts, wt, cs, m(3, 3, dt=torch.float64), 0.25, 1, 500)
    assert p.shape == n.shape == c.shape == (3, 500, 3) and p.dtype == n.dtype == torch.float64 and c.dtype == torch.float32
    assert v.shape == (3, 500) and v.dtype == torch.uint8 and k.shape == (3,) and k.dtype == torch.int32
    assert torch.ops.relpose.tsdf_surface(ts, wt, None, m(3, 3, dt=torch.float64), 0.25)[2].numel() == 0
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.tsdf_fuse(torch.ones(2, 4, 16), None, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1), torch.tensor([0, 2]),
                                    torch.zeros(1, 3, dtype=torch.float64), [2, 2, 2], 0.5, 0)


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_tsdf_fuse(None) == EINVAL and lib.relpose_tsdf_surface(None) == EINVAL
    buf = (C.c_double * 64)()                      # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)
    host = TS.host_arrays()
    calls = TS.fuse_einval_calls()
    assert len(calls) > 40 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        assert lib.relpose_tsdf_fuse(C.byref(TS.fuse_args(_lib, p, host, kw))) == EINVAL, name
    calls = TS.surface_einval_calls()
    assert len(calls) >= 30 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        assert lib.relpose_tsdf_surface(C.byref(TS.surface_args(_lib, p, host, kw))) == EINVAL, name
    assert buf[:] == [0.0] * 64
    W = lib.relpose_tsdf_fuse_workspace_bytes
    assert W(2, 3, 4, 3, 2, 2) >= 2 * 3 * 8 + 3 * 4 and W(2, 3, 4, 3, 2, 2) % 256 == 0
    for a in ((0, 3, 4, 3, 2, 2), (2, 0, 4, 3, 2, 2), (2, 3, 5, 3, 2, 2), (2, 3, 0, 3, 2, 2), (2, 3, 8194, 3, 2, 2), (2, 8, 8192, 3, 2, 2),
              (2, 3, 4, 0, 2, 2), (2, 3, 4, 3, -1, 2), (2, 3, 4, 3, 2, 0), (2, 3, 4, 2048, 1024, 512), (1, 3, 4, 1 << 30, 2, 1), (-1, 3, 4, 3, 2, 2)):
        assert W(*a) == 0, a
    assert W(1, 1, 4, 2047, 1024, 1024) > 0                                    # 2^31 - 2^20 voxels: inside the limit
    Ws = lib.relpose_tsdf_surface_workspace_bytes
    nblk = lambda n: (n + 255) // 256
    assert Ws(2, 3, 2, 2) >= 2 * 3 * 8 + 2 * nblk(12) * 4 and Ws(2, 3, 2, 2) % 256 == 0
    assert Ws(1, 256, 256, 128) - Ws(1, 256, 256, 64) == nblk(256 * 256 * 64) * 4      # one int per workgroup of 256 voxels
    for a in ((0, 3, 2, 2), (2, 0, 2, 2), (2, 3, -2, 2), (2, 3, 2, 0), (2, 2048, 1024, 512), (1, 1024, 1024, 700), (-1, 3, 2, 2)):
        assert Ws(*a) == 0, a
    assert Ws(1, 1024, 1024, 600) > 0


def test_cli_flag_and_its_default():
    from relativepose_amd import evaluation as E
    assert E._cli_parser_completion().parse_args([]).fuse is None
    assert E._cli_parser_completion().parse_args(["--mine-pairs", "--fuse", "0.0625"]).fuse == 0.0625
    assert E._cli_parser_completion().parse_args(["--method", "fgs", "--fuse", "0.125"]).fuse == 0.125
    for argv in (["--fuse", "0"], ["--fuse", "-1"], ["--descriptor-eval", "--fuse", "0.1"], ["--completion-eval", "--fuse", "0.1"],
                 ["--gpus", "2", "--fuse", "0.1"], ["--keypoint-mode", "reference", "--fuse", "0.1"]):
        with pytest.raises(SystemExit):
            E.main(argv)
    e = E.wall_error(np.array([[1.0, 0.2, 0.3], [0.0, 1.9, 0.0]]), [1.5, 2.0, 2.5], 0.25)
    assert np.allclose(e, [2.0, 0.4])
    s = E.fuse_summary([{'fuse_accuracy': 0.9, 'fuse_completeness': 0.8, 'fuse_points': 10, 'err_ad': 1.0},
                        {'fuse_accuracy': 0.5, 'fuse_completeness': 0.6, 'fuse_points': 30, 'err_ad': 9.0},
                        {'fuse_accuracy': float("nan"), 'fuse_completeness': float("nan"), 'fuse_points': 0, 'err_ad': 50.0}])
    assert s["fuse_accuracy_median"] == 0.7 and s["fuse_completeness_median"] == 0.7 and s["fuse_spearman_rot"] == pytest.approx(-1.0)
