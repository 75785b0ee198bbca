"""GPU: relpose_tsdf_fuse and relpose_tsdf_surface (TSDF fusion of posed depth panoramas) against the numpy model bit for
bit on the pinned rooms, the tiny volumes, the three-scene batch and the hand-built edge cases; batch invariance, repeatability and
accumulation; the overflow of `cap`; the operators and the shims against the C ABI; every RELPOSE_EINVAL path with pre-filled outputs; and
the evaluation drivers built on it.  Every test runs under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler
from types import SimpleNamespace

import numpy as np
import pytest

import tsdf_model as TM
import tsdf_scenes as TS
from gpu_util import log
from relativepose_amd import synth, weights

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; the slowest (the pipeline fixture) takes a few


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    import torch
    return torch.device("cuda:0")


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


def host_state(st):
    return {"tsdf_sum": st["tsdf_sum"].cpu().numpy(), "weight": st["weight"].cpu().numpy(),
            "color_sum": None if st["color_sum"] is None else st["color_sum"].cpu().numpy().view(np.uint32)}


def fuse(c, rgb=True, views=None, state=None, R=None):
    """util.tsdf_fuse_dev on a case of tsdf_scenes (views: a slice of a single-scene case) -> the device state"""
    from relativepose_amd import util
    v = slice(None) if views is None else views
    depth, col, pose = c["depth"][v], c["rgb"][v], (c["R"] if R is None else R)[v]
    vb = c["view_begin"] if views is None else np.array([0, len(depth)], np.int32)
    return util.tsdf_fuse_dev(up(depth, np.float32), up(col, np.float32) if rgb else None, pose, vb, c["origin"], c["dims"], c["voxel"], c["ds"],
                              c["trunc"], state=state)


def surface_raw(st, origin, voxel, min_weight, cap, colours=True):
    """relpose_tsdf_surface through the C ABI into outputs pre-filled with TS.FILL -> the model's output dict"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    ts, wt, cs = st["tsdf_sum"], st["weight"], st["color_sum"]
    S, nz, ny, nx = ts.shape
    nbytes = L.relpose_tsdf_surface_workspace_bytes(S, nx, ny, nz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    out = {"points": torch.full((S, cap, 3), TS.FILL["points"], dtype=torch.float64, device=dev()),
           "normals": torch.full((S, cap, 3), TS.FILL["normals"], dtype=torch.float64, device=dev()),
           "colors": torch.full((S, cap, 3), TS.FILL["colors"], dtype=torch.float32, device=dev()) if colours and cs is not None else None,
           "valid": torch.full((S, cap), 77, dtype=torch.uint8, device=dev()), "n_points": torch.full((S,), -7, dtype=torch.int32, device=dev())}
    org = np.ascontiguousarray(origin, dtype=np.float64).reshape(S, 3)
    a = _lib.TsdfSurfaceArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.nx, a.ny, a.nz, a.min_weight, a.cap = S, nx, ny, nz, min_weight, cap
    a.tsdf_sum, a.weight, a.color_sum = ts.data_ptr(), wt.data_ptr(), (0 if cs is None else cs.data_ptr())
    a.origin_host, a.voxel = org.ctypes.data, voxel
    a.points, a.normals, a.valid, a.n_points = (out[k].data_ptr() for k in ("points", "normals", "valid", "n_points"))
    a.colors = 0 if out["colors"] is None else out["colors"].data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_surface(C.byref(a)) == 0
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def check_state(name, got, want):
    bad = TS.differ(got, want, TS.STATE_KEYS)
    log("tsdf_fuse_" + name, differ=bad, weight=int(got["weight"].sum()), want_weight=int(want["weight"].sum()),
        tsdf=int(got["tsdf_sum"].astype(np.int64).sum()), want_tsdf=int(want["tsdf_sum"].astype(np.int64).sum()))
    assert bad == [], (name, bad)


def check_surface(name, got, want):
    bad = TS.differ(got, want, TS.SURF_KEYS)
    log("tsdf_surface_" + name, differ=bad, n=got["n_points"].tolist(), want_n=want["n_points"].tolist())
    assert bad == [], (name, bad, got["n_points"].tolist(), want["n_points"].tolist())


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS)
def test_rooms_match_the_model_bitwise(ds, h):
    c = TS.room(ds, h)
    st = fuse(c)
    check_state(f"room_{ds}_{h}", host_state(st), TS.room_state(ds, h))
    cap, want = TS.room_surface(ds, h)
    got = surface_raw(st, c["origin"], c["voxel"], 1, cap)
    check_surface(f"room_{ds}_{h}", got, want)
    n = int(got["n_points"][0])
    med, p90, mx = TS.wall_stats(got["points"][0, :n], c["half"], c["voxel"])
    log(f"tsdf_wall_{ds}_{h}", points=n, median=med, p90=p90, max=mx)
    assert n == cap - 5 and (got["valid"][0, n:] == 0).all() and (got["points"][0, n:] == TS.FILL["points"]).all()
    # without colours: the same volume and cloud
    st0 = fuse(c, rgb=False)
    h0 = host_state(st0)
    assert h0["color_sum"] is None and TS.differ(h0, TS.room_state(ds, h), ("tsdf_sum", "weight")) == []
    got0 = surface_raw(st0, c["origin"], c["voxel"], 1, cap)
    assert got0["colors"] is None and TS.differ(got0, want, ("points", "normals", "valid", "n_points")) == []


@pytest.mark.parametrize("which", ["1x1x2", "5x3x2"])
def test_tiny_volumes_match_the_model_bitwise(which):
    c = TS.tiny(which)
    want = TS.fuse_model(c)
    st = fuse(c)
    check_state(which, host_state(st), want)
    for cap in (1, 40):
        check_surface(f"{which}_{cap}", surface_raw(st, c["origin"], c["voxel"], 1, cap), TM.surface_outputs(want, c["origin"], c["voxel"], 1, cap, TS.FILL))


@pytest.mark.parametrize("trunc", [1.0, 0.3])
@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
def test_fuse_edge_case_matches_the_model_bitwise(ds, trunc):
    """tsdf_scenes.edge_case: voxel centres exactly on |xn| = 1 and on half pixels, d at and just below 32768, sdf exactly -trunc and one
    float32 ulp either side, depths 0 / -1 / NaN / +-inf / huge, NaN and inf in a pose, rgb below 0, above 1 and NaN."""
    c = dict(TS.edge_case(ds))
    c["trunc"] = trunc
    want = TS.fuse_model(c)
    st = fuse(c)
    check_state(f"edge_{ds}_{trunc}", host_state(st), want)
    n = TS.surface_cap(want, c["origin"], c["voxel"])
    for cap in (max(1, n // 2), n + 4):
        check_surface(f"edge_{ds}_{trunc}_{cap}", surface_raw(st, c["origin"], c["voxel"], 1, cap),
                      TM.surface_outputs(want, c["origin"], c["voxel"], 1, cap, TS.FILL))


@pytest.mark.parametrize("min_weight", [1, 2, 4])
def test_surface_edge_state_matches_the_model_bitwise(min_weight):
    """tsdf_scenes.edge_state: ta exactly 0, a known voxel without a known neighbour, weights below min_weight, more crossings than cap"""
    e = TS.edge_state()
    want_state = {k: e[k] for k in TS.STATE_KEYS}
    st = {"tsdf_sum": up(e["tsdf_sum"], np.int32), "weight": up(e["weight"], np.int32), "color_sum": up(e["color_sum"].view(np.int32), np.int32)}
    n = TS.surface_cap(want_state, e["origin"], e["voxel"], min_weight)
    assert n > 10 or min_weight == 4
    for cap in (1, 10, n + 3):
        got = surface_raw(st, e["origin"], e["voxel"], min_weight, cap)
        check_surface(f"edge_state_{min_weight}_{cap}", got, TM.surface_outputs(want_state, e["origin"], e["voxel"], min_weight, cap, TS.FILL))
        assert got["n_points"][0] == n                                         # the full count, whatever cap is
        assert got["valid"][0].tolist() == [1] * min(n, cap) + [0] * max(0, cap - n)
        assert (got["points"][0, min(n, cap):] == TS.FILL["points"]).all() and (got["normals"][0, min(n, cap):] == TS.FILL["normals"]).all()


def test_batch_equals_its_scenes_alone_and_repeats_bitwise():
    c = TS.batch()
    want = TS.fuse_model(c)
    st = fuse(c)
    got = host_state(st)
    check_state("batch", got, want)
    assert (got["weight"][1] == 0).all() and (got["tsdf_sum"][1] == 0).all() and (got["color_sum"][1] == 0).all()      # the scene without a view
    assert TS.differ(host_state(fuse(c)), got, TS.STATE_KEYS) == []            # a second run
    cap = TS.surface_cap(want, c["origin"], c["voxel"]) + 3
    surf = surface_raw(st, c["origin"], c["voxel"], 1, cap)
    check_surface("batch", surf, TM.surface_outputs(want, c["origin"], c["voxel"], 1, cap, TS.FILL))
    assert TS.differ(surface_raw(st, c["origin"], c["voxel"], 1, cap), surf, TS.SURF_KEYS) == []
    assert surf["n_points"][1] == 0 and (surf["valid"][1] == 0).all() and surf["n_points"][0] != surf["n_points"][2]
    for k in (0, 2):                                                           # a scene does not depend on the batch around it
        m = TS.batch_member(k)
        one = fuse(m)
        h1 = host_state(one)
        assert all(TS.bits_equal(h1[key][0], got[key][k]) for key in TS.STATE_KEYS), k
        s1 = surface_raw(one, m["origin"], m["voxel"], 1, cap)
        assert all(TS.bits_equal(s1[key][0], surf[key][k]) for key in TS.SURF_KEYS), k
    assert TS.bits_equal(got["tsdf_sum"][0], TS.room_state("suncg", 16)["tsdf_sum"][0])


@pytest.mark.parametrize("ds,h", TS.ROOM_KEYS[:2])
def test_accumulate_over_a_split_and_any_view_order_equal_one_call(ds, h):
    c, want = TS.room(ds, h), TS.room_state(ds, h)
    M = len(c["depth"])
    for cut in (1, M - 1):
        st = fuse(c, views=slice(0, cut))
        st2 = fuse(c, views=slice(cut, M), state=st)
        assert st2 is st
        check_state(f"split_{ds}_{h}_{cut}", host_state(st), want)
    rev = dict(c)
    rev["depth"], rev["rgb"], rev["R"] = c["depth"][::-1], c["rgb"][::-1], c["R"][::-1]
    check_state(f"reversed_{ds}_{h}", host_state(fuse(rev)), want)
    from relativepose_amd import util
    with pytest.raises(ValueError):                                            # a state of another geometry is not added to
        util.tsdf_fuse_dev(up(c["depth"], np.float32), up(c["rgb"], np.float32), c["R"], c["view_begin"], c["origin"] + 0.5, c["dims"], c["voxel"], ds,
                           c["trunc"], state=st)


def test_operators_and_shims_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import _lib, ops, util  # noqa: F401
    c = TS.batch()
    want = TS.fuse_model(c)
    S, (nx, ny, nz), V, h = 3, c["dims"], len(c["depth"]), c["h"]
    depth, rgb, pose = up(c["depth"], np.float32), up(c["rgb"], np.float32), up(c["R"], np.float64)
    # the C ABI, driven by hand, into pre-filled state (accumulate = 0 stores)
    L = _lib.lib()
    nbytes = L.relpose_tsdf_fuse_workspace_bytes(S, V, h, nx, ny, nz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    ts = torch.full((S, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    wt = torch.full((S, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    cs = torch.full((S, 3, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    vb, org = np.ascontiguousarray(c["view_begin"], np.int32), np.ascontiguousarray(c["origin"], np.float64)
    a = _lib.TsdfFuseArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz, a.accumulate = S, V, h, util.DATASETS[c["ds"]], nx, ny, nz, 0
    a.depth, a.rgb, a.pose = depth.data_ptr(), rgb.data_ptr(), pose.data_ptr()
    a.view_begin_host, a.origin_host, a.voxel, a.trunc = vb.ctypes.data, org.ctypes.data, c["voxel"], c["trunc"]
    a.tsdf_sum, a.weight, a.color_sum = ts.data_ptr(), wt.data_ptr(), cs.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_fuse(C.byref(a)) == 0
    abi = host_state({"tsdf_sum": ts, "weight": wt, "color_sum": cs})
    check_state("c_abi", abi, want)
    a.accumulate = 1                                                           # and once more on top: everything doubles
    assert L.relpose_tsdf_fuse(C.byref(a)) == 0
    twice = host_state({"tsdf_sum": ts, "weight": wt, "color_sum": cs})
    assert all(np.array_equal(twice[k], 2 * want[k]) for k in TS.STATE_KEYS)
    # the operator (pose as a tensor, trunc 0 = 4 voxel) and the shim
    ds_id = util.DATASETS[c["ds"]]
    o_ts, o_wt, o_cs = torch.ops.relpose.tsdf_fuse(depth, rgb, pose, torch.from_numpy(vb).to(dev()), torch.from_numpy(org), list(c["dims"]),
                                                   c["voxel"], ds_id, 0.0)
    assert c["trunc"] == 4 * c["voxel"]
    assert TS.differ(host_state({"tsdf_sum": o_ts, "weight": o_wt, "color_sum": o_cs}), abi, TS.STATE_KEYS) == []
    n_ts, n_wt, n_cs = torch.ops.relpose.tsdf_fuse(depth, None, pose, torch.from_numpy(vb), torch.from_numpy(org), list(c["dims"]), c["voxel"], ds_id)
    assert n_cs.numel() == 0 and torch.equal(n_ts, o_ts) and torch.equal(n_wt, o_wt)
    cap = TS.surface_cap(want, c["origin"], c["voxel"]) + 3
    st = fuse(c)
    raw = surface_raw(st, c["origin"], c["voxel"], 1, cap)
    op = torch.ops.relpose.tsdf_surface(o_ts, o_wt, o_cs, torch.from_numpy(org), c["voxel"], 1, cap)
    shim = util.tsdf_surface_dev(st, 1, cap)
    auto = util.tsdf_surface_dev(st)                                           # max_points=None: cap = the largest scene's count
    assert auto[0].shape[1] == int(raw["n_points"].max()) == cap - 3
    zero = TM.surface_outputs(want, c["origin"], c["voxel"], 1, cap, {"points": 0.0, "normals": 0.0, "colors": 0.0})      # the shims pre-fill with zeros
    for got in (op, shim):
        g = {k: v.cpu().numpy() for k, v in zip(TS.SURF_KEYS, got)}
        assert TS.differ(g, zero, TS.SURF_KEYS) == []
    for k, v in zip(TS.SURF_KEYS, auto):
        assert TS.bits_equal(v.cpu().numpy(), zero[k][:, :cap - 3] if k != "n_points" else zero[k]), k
    assert torch.ops.relpose.tsdf_surface(n_ts, n_wt, None, torch.from_numpy(org), c["voxel"], 1, cap)[2].numel() == 0
    # the Meta shapes
    m = torch.ops.relpose.tsdf_fuse(depth.to("meta"), rgb.to("meta"), pose.to("meta"), torch.from_numpy(vb).to("meta"), torch.from_numpy(org).to("meta"),
                                    list(c["dims"]), c["voxel"], ds_id)
    for got, ref in zip(m, (o_ts, o_wt, o_cs)):
        assert got.shape == ref.shape and got.dtype == ref.dtype
    m = torch.ops.relpose.tsdf_surface(o_ts.to("meta"), o_wt.to("meta"), o_cs.to("meta"), torch.from_numpy(org).to("meta"), c["voxel"], 1, cap)
    for got, ref in zip(m, op):
        assert got.shape == ref.shape and got.dtype == ref.dtype
    # no view at all: a stored state is zero, an accumulated one unchanged
    e = util.tsdf_fuse_dev(depth[:0], rgb[:0], c["R"][:0], [0, 0, 0, 0], c["origin"], c["dims"], c["voxel"], c["ds"])
    assert all((e[k] == 0).all() for k in TS.STATE_KEYS)
    util.tsdf_fuse_dev(depth[:0], rgb[:0], c["R"][:0], [0, 0, 0, 0], c["origin"], c["dims"], c["voxel"], c["ds"], c["trunc"], state=st)
    check_state("no_views", host_state(st), want)
    for bad in (dict(view_begin=[0, 3, 2, 5]), dict(view_begin=[0, 3, 3, 4]), dict(voxel=0.0), dict(trunc=-1.0)):
        kw = dict(view_begin=c["view_begin"], voxel=c["voxel"], trunc=c["trunc"])
        kw.update(bad)
        with pytest.raises(ValueError):
            util.tsdf_fuse_dev(depth, rgb, c["R"], kw["view_begin"], c["origin"], c["dims"], kw["voxel"], c["ds"], kw["trunc"])


def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, V, h, nx, ny, nz, cap = 2, 3, 4, 3, 2, 2, 8
    host = TS.host_arrays()
    depth = torch.full((V, h, 4 * h), 2.0, dtype=torch.float32, device=dev())
    rgb = torch.full((V, 3, h, 4 * h), 0.5, dtype=torch.float32, device=dev())
    pose = torch.eye(4, dtype=torch.float64, device=dev()).repeat(V, 1, 1)
    ts = torch.full((S, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    wt = torch.full((S, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    cs = torch.full((S, 3, nz, ny, nx), -7, dtype=torch.int32, device=dev())
    ws = torch.empty(max(L.relpose_tsdf_fuse_workspace_bytes(S, V, h, nx, ny, nz), L.relpose_tsdf_surface_workspace_bytes(S, nx, ny, nz)) + 512,
                     dtype=torch.uint8, device=dev())
    ptrs = {"depth": depth.data_ptr(), "rgb": rgb.data_ptr(), "pose": pose.data_ptr(), "tsdf_sum": ts.data_ptr(), "weight": wt.data_ptr(),
            "color_sum": cs.data_ptr()}
    calls = TS.fuse_einval_calls()
    for name, kw in calls:
        a = TS.fuse_args(_lib, 0, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
        a.stream = _lib.stream_ptr()
        assert L.relpose_tsdf_fuse(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert (ts == -7).all() and (wt == -7).all() and (cs == -7).all()
    a = TS.fuse_args(_lib, 0, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
    a.stream = _lib.stream_ptr()
    assert L.relpose_tsdf_fuse(C.byref(a)) == 0                                # the base call itself is valid
    assert (wt >= 0).all() and (wt <= 2).all() and wt.sum() > 0 and (cs >= 0).all()
    pts = torch.full((S, cap, 3), -7.0, dtype=torch.float64, device=dev())
    nrm = torch.full((S, cap, 3), -7.0, dtype=torch.float64, device=dev())
    col = torch.full((S, cap, 3), -7.0, dtype=torch.float32, device=dev())
    val = torch.full((S, cap), 77, dtype=torch.uint8, device=dev())
    npt = torch.full((S,), -7, dtype=torch.int32, device=dev())
    ptrs = {"tsdf_sum": ts.data_ptr(), "weight": wt.data_ptr(), "color_sum": cs.data_ptr(), "points": pts.data_ptr(), "normals": nrm.data_ptr(),
            "colors": col.data_ptr(), "valid": val.data_ptr(), "n_points": npt.data_ptr()}
    for name, kw in TS.surface_einval_calls():
        a = TS.surface_args(_lib, 0, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
        a.stream = _lib.stream_ptr()
        assert L.relpose_tsdf_surface(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert (pts == -7).all() and (nrm == -7).all() and (col == -7).all() and (val == 77).all() and (npt == -7).all()
    a = TS.surface_args(_lib, 0, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
    a.stream = _lib.stream_ptr()
    assert L.relpose_tsdf_surface(C.byref(a)) == 0
    assert (npt >= 0).all() and (val <= 1).all()


def test_bounds_fuse_views_and_reconstruction_scores():
    from relativepose_amd import evaluation as E, util
    c = TS.room("suncg", 32)
    depth, rgb = up(c["depth"], np.float32), up(c["rgb"], np.float32)
    origin, dims = util.tsdf_bounds_dev(depth, c["R"], "suncg", c["voxel"])
    # the same box from the reference's unprojection on the host (the oracle's Pano2PointCloud), the validity from the fuse rule
    from oracle import geom_oracle as G
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for v in range(len(c["depth"])):
        pc = G.pano2pc(c["depth"][v], "suncg")                                  # [3, 4 h h], face after face
        ok = np.concatenate([c["depth"][v][:, f * 32:(f + 1) * 32].reshape(-1) for f in range(4)]) > 0
        inv = np.linalg.inv(c["R"][v])
        pw = (np.matmul(inv[:3, :3], pc) + inv[:3, 3:4])[:, ok]
        lo, hi = np.minimum(lo, pw.min(1)), np.maximum(hi, pw.max(1))
    assert np.allclose(origin[0], lo - 3 * c["voxel"], atol=1e-9) and all(abs(dims[a] - (int(np.ceil((hi[a] - lo[a]) / c["voxel"])) + 7)) <= 1 for a in range(3))
    assert (origin[0] + 3 * c["voxel"] <= lo + 1e-9).all() and (origin[0] + (np.array(dims) - 3) * c["voxel"] >= hi - 1e-9).all()
    assert (lo > -c["half"] - 1e-4).all() and (hi < c["half"] + 1e-4).all()    # the points lie in the room
    o2, d2 = util.tsdf_bounds_dev(torch_cat(depth, depth[:2]), np.concatenate([c["R"], c["R"][:2]]), "suncg", c["voxel"], view_begin=[0, 4, 4, 6])
    assert d2 == dims and np.array_equal(o2[0], origin[0]) and np.array_equal(o2[1], [-3 * c["voxel"]] * 3) and (o2[2] >= origin[0]).all()
    surf = E.fuse_views(depth, rgb, c["R"], "suncg", c["voxel"])
    n = int(surf["n_points"][0])
    assert surf["points"].shape == (1, n, 3) and surf["valid"].all() and surf["colors"].shape == (1, n, 3)
    want = TM.fuse(c["depth"], c["rgb"], c["R"], c["view_begin"], origin, dims, c["voxel"], "suncg")       # the model in the same box
    ws = TM.surface(want["tsdf_sum"][0], want["weight"][0], want["color_sum"][0], origin[0], c["voxel"])
    assert ws["n"] == n and TS.bits_equal(surf["points"][0].cpu().numpy(), ws["points"]) and TS.bits_equal(surf["colors"][0].cpu().numpy(), ws["colors"])
    med, p90, mx = TS.wall_stats(ws["points"], c["half"], c["voxel"])
    log("tsdf_fuse_views", points=n, median=med, p90=p90, max=mx)
    # the surface feeds overlap_dev unchanged: a surface against itself scores 1 / 1
    acc, comp = E.reconstruction_scores(surf, surf)
    assert acc.tolist() == [1.0] and comp.tolist() == [1.0]
    bad = E.fuse_views(depth, rgb, TS.perturbed(c), "suncg", c["voxel"])
    acc, comp = E.reconstruction_scores(bad, surf)
    log("tsdf_scores_perturbed", accuracy=float(acc[0]), completeness=float(comp[0]))
    assert 0.0 < acc[0] < 1.0 and 0.0 < comp[0] < 1.0
    empty = {"points": surf["points"][:, :5] * 0, "valid": surf["valid"][:, :5] * 0}
    acc, comp = E.reconstruction_scores(empty, surf)
    assert np.isnan(acc[0]) and comp[0] == 0.0


def torch_cat(a, b):
    import torch
    return torch.cat([a, b])


@pytest.fixture(scope="module")
def eval_runs():
    """Two suncg pairs at h = 32 through the pipeline with the synthetic weights: evaluate_pairs with fuse None and fuse 0.125"""
    from relativepose_amd import evaluation as E
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    ds, mm, S, h = "suncg", "second", 15, 32
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(7, S))
    pipe = RelativePosePipeline(net, ds, mm)
    batch = synth.make_pairs(2, 1000, ds, h)
    batch["pts"], batch["ptw"] = synth.make_keypoints(2, 60, 1000, mm, h)
    recs = {f: E.evaluate_pairs(pipe, [batch], dev(), fuse=f) for f in (None, 0.125)}
    faulthandler.cancel_dump_traceback_later()
    return pipe, batch, recs


OLD_KEYS = ('img_src', 'img_tgt', 'err_ad', 'err_t', 'err_blind', 'err_t_blind', 'overlap', 'pc_dist', 'cam_dist', 'pc_nearest', 'R_gt', 'R_pred_44')
NEW_KEYS = ('fuse_accuracy', 'fuse_completeness', 'fuse_points')


def _same_record(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        assert (x == y) if isinstance(x, str) else np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), k


def test_evaluate_pairs_without_fuse_gives_the_records_it_gave(eval_runs):
    from relativepose_amd import evaluation as E
    pipe, batch, recs = eval_runs
    st = pipe.prepare(batch["rgb"], batch["norm"], batch["depth"], batch["pts"], batch["ptw"], dev())
    pose = pipe.run(st)[0].cpu().numpy()
    old = E._default_record(pipe, batch, pose, dev(), None, [0, 1])
    assert len(recs[None]) == 2
    for a, b in zip(recs[None], old):
        assert tuple(a) == OLD_KEYS == tuple(b)
        _same_record(a, b, OLD_KEYS)


def test_evaluate_pairs_with_fuse_adds_the_three_fields(eval_runs):
    from relativepose_amd import evaluation as E
    pipe, batch, recs = eval_runs
    assert len(recs[0.125]) == 2
    for a, b in zip(recs[0.125], recs[None]):
        assert tuple(a) == OLD_KEYS + NEW_KEYS
        _same_record(a, b, OLD_KEYS)                                           # the new fields leave the old ones alone
        assert 0.0 <= a['fuse_accuracy'] <= 1.0 and 0.0 <= a['fuse_completeness'] <= 1.0 and isinstance(a['fuse_points'], int) and a['fuse_points'] > 0
    # under the ground truth itself the estimate's fusion is the reference's
    st = pipe.prepare(batch["rgb"], batch["norm"], batch["depth"], batch["pts"], batch["ptw"], dev())
    R_gts = [np.matmul(batch["R"][b, 1], np.linalg.inv(batch["R"][b, 0])) for b in range(2)]
    f = E._fuse_fields(E._verify_depth(pipe, st, "observed", None), R_gts, R_gts, pipe.dataset, 0.125)
    assert all(r['fuse_accuracy'] == 1.0 and r['fuse_completeness'] == 1.0 for r in f)
    s = E.fuse_summary(recs[0.125])
    assert set(s) == {"fuse_accuracy_median", "fuse_completeness_median", "fuse_points_median", "fuse_spearman_rot"}
    log("tsdf_eval", accuracy=[r['fuse_accuracy'] for r in recs[0.125]], completeness=[r['fuse_completeness'] for r in recs[0.125]],
        points=[r['fuse_points'] for r in recs[0.125]])
