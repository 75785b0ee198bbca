"""GPU: relpose_tsdf_render (panoramas rendered from TSDF volumes) against the numpy model, bit for bit: the closed rooms,
a pinned scannet room (the face order) and the hand-built edge volume, skip against no skip, batch independence and repeatability, h = 2,
the optional outputs, the operator and the shim against the C ABI, every RELPOSE_EINVAL path with pre-filled outputs, and one end-to-end
render of a fused scene.  Every test runs under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import align_scenes as AS
import render_model as RM
import render_scenes as RS
import tsdf_scenes as TS
from gpu_util import log

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few


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


def render_raw(cs, skip=True, normal=True, color=True, stages=True, with_color_sum=True, **kw):
    """relpose_tsdf_render through the C ABI into outputs pre-filled with RS.FILL -> the model's output dict (host arrays; None where the
    output was not asked for)"""
    import torch
    from relativepose_amd import _lib, util
    L = _lib.lib()
    p = {k: cs[k] for k in ("d_min", "step", "n_steps", "min_weight")}
    p.update(kw)
    st = cs["state"]
    ts, wt = up(st["tsdf_sum"], np.int32), up(st["weight"], np.int32)
    col = up(st["color_sum"].astype(np.int64), np.int32) if with_color_sum else None
    S, nz, ny, nx = ts.shape
    T = up(cs["pose"], np.float64)
    sov = np.ascontiguousarray(cs["scene_of_view"], dtype=np.int32)
    V, h = T.shape[0], cs["h"]
    nbytes = L.relpose_tsdf_render_workspace_bytes(S, V, h, nx, ny, nz)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    shapes = {"depth": ((V, h, 4 * h), torch.float32), "cls": ((V, h, 4 * h), torch.uint8), "normal": ((V, 3, h, 4 * h), torch.float32),
              "color": ((V, 3, h, 4 * h), torch.float32), "n_evaluated": ((V, h, 4 * h), torch.int32)}
    want = {"depth": True, "cls": True, "normal": normal, "color": color, "n_evaluated": stages}
    out = {k: torch.full(s, RS.FILL[k], dtype=dt, device=dev()) for k, (s, dt) in shapes.items() if want[k]}
    org = np.ascontiguousarray(cs["origin"], dtype=np.float64).reshape(S, 3)
    a = _lib.TsdfRenderArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz = S, V, h, util.DATASETS[cs["ds"]], nx, ny, nz
    a.min_weight, a.n_steps, a.skip = p["min_weight"], p["n_steps"], int(skip)
    a.tsdf_sum, a.weight, a.color_sum, a.pose = ts.data_ptr(), wt.data_ptr(), (0 if col is None else col.data_ptr()), T.data_ptr()
    a.origin_host, a.scene_of_view_host = org.ctypes.data, sov.ctypes.data
    a.voxel, a.d_min, a.step = cs["voxel"], p["d_min"], p["step"]
    for k in RM.KEYS:
        setattr(a, k, out[k].data_ptr() if k in out else 0)
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_render(C.byref(a)) == 0
    return {k: (out[k].cpu().numpy() if k in out else None) for k in RM.KEYS}


def check(name, got, want, keys=RM.KEYS):
    bad = TS.differ(got, want, keys)
    log("tsdf_render_" + name, differ=bad, cls=np.bincount(got["cls"].ravel(), minlength=3), want_cls=np.bincount(want["cls"].ravel(), minlength=3),
        evaluated=None if got["n_evaluated"] is None else int(got["n_evaluated"].sum()),
        depth_diff=float(np.abs(got["depth"].astype(np.float64) - want["depth"]).max()))
    assert bad == [], (name, bad)


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name,views", [("closed16", None), ("closed32", [1]), ("scannet16", [0])])
@pytest.mark.parametrize("skip", [True, False])
def test_rooms_match_the_model_bitwise(name, views, skip):
    cs = RS.case(name, views)
    check(f"{name}_skip{int(skip)}", render_raw(cs, skip=skip), RS.model_of(cs, skip=skip))


@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
@pytest.mark.parametrize("h", [2, 4])
def test_edge_volume_gets_what_the_contract_gives(ds, h):
    """the axis rays, t = 0 exactly, s = 0, an unknown voxel between a positive and a negative sample, the camera inside a solid and outside
    the box, the last cell and one past it, NaN and inf in a pose; n_steps = 1; a volume with a dimension of 1; h = 2 is 16 pixels, a
    quarter of a wave"""
    e = RS.edge_case(ds, h)
    for skip in (True, False):
        want = RS.model_of(e, skip=skip)
        got = render_raw(e, skip=skip)
        check(f"edge_{ds}_{h}_skip{int(skip)}", got, want)
        check(f"edge_{ds}_{h}_one_step", render_raw(e, skip=skip, n_steps=1), RS.model_of(e, skip=skip, n_steps=1))
    for v in (3, 4):
        assert (got["cls"][v] == 0).all() and not got["depth"][v].any() and not got["normal"][v].any() and not got["color"][v].any()
    if ds == "suncg" and h == 4:
        assert got["cls"][RS.EDGE_AXIS["hit_s0"]] == 1 and got["depth"][RS.EDGE_AXIS["hit_s0"]] == np.float32(0.5)
        assert got["cls"][RS.EDGE_AXIS["no_bridge"]] == 0 and got["cls"][RS.EDGE_AXIS["back_face"]] == 2
        flat = RS.flat_case()
        for skip in (True, False):
            g = render_raw(flat, skip=skip)
            check(f"flat_skip{int(skip)}", g, RS.model_of(flat, skip=skip))
            assert (g["cls"] == 0).all() and not g["n_evaluated"].any()


# ---------------------------------------------------------------------------------------------- 2. skip
def test_skip_changes_nothing_but_the_count():
    for cs in (RS.case("closed32"), RS.batch(), RS.edge_case()):
        a, b = render_raw(cs, skip=True), render_raw(cs, skip=False)
        assert TS.differ(a, b, RM.IMAGE_KEYS) == []
        assert (a["n_evaluated"] <= b["n_evaluated"]).all()
    a, b = render_raw(RS.case("closed32"), skip=True), render_raw(RS.case("closed32"), skip=False)
    log("tsdf_render_skip_closed32", evaluated_skip=int(a["n_evaluated"].sum()), evaluated_plain=int(b["n_evaluated"].sum()))
    assert int(a["n_evaluated"].sum()) < int(b["n_evaluated"].sum())


# ---------------------------------------------------------------------------------------------- 3. the batch
def test_batch_equals_its_members_and_repeats_bitwise():
    b = RS.batch()
    got = render_raw(b)
    check("batch", got, RS.model_of(b))
    assert (got["cls"][2] == 0).all() and not got["n_evaluated"][2].any() and not got["depth"][2].any()       # 100 m away
    assert not (b["scene_of_view"] == 1).any()                                                             # scene 1 has no view
    assert (b["scene_of_view"] == 2).sum() == 2                                                            # two views share a volume
    again = render_raw(b)
    assert TS.differ(again, got, RM.KEYS) == []
    for v in range(len(b["pose"])):
        one = render_raw(RS.batch_member(v))
        for k in RM.KEYS:
            assert TS.bits_equal(one[k][0], got[k][v]), (v, k)


# ---------------------------------------------------------------------------------------------- 4. the optional outputs
def test_optional_outputs_do_not_change_the_others():
    b = RS.batch()
    full = render_raw(b)
    for kw in (dict(normal=False), dict(color=False), dict(stages=False), dict(normal=False, color=False, stages=False),
               dict(color=False, with_color_sum=False)):
        got = render_raw(b, **kw)
        for k in RM.KEYS:
            off = (k == "normal" and not kw.get("normal", True)) or (k == "color" and not kw.get("color", True)) or \
                  (k == "n_evaluated" and not kw.get("stages", True))
            assert got[k] is None if off else TS.bits_equal(got[k], full[k]), (kw, k)


# ---------------------------------------------------------------------------------------------- 5. operator and shim
def test_operator_and_shim_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import ops, util
    assert "tsdf_render" in ops.OPS
    b = RS.batch()
    abi = render_raw(b)
    ts, wt = up(b["state"]["tsdf_sum"], np.int32), up(b["state"]["weight"], np.int32)
    col = up(b["state"]["color_sum"].astype(np.int64), np.int32)
    pose = up(b["pose"], np.float64)
    st = {"tsdf_sum": ts, "weight": wt, "color_sum": col, "origin": b["origin"], "dims": b["dims"], "voxel": b["voxel"], "dataset": b["ds"]}
    shim = util.tsdf_render_dev(st, b["pose"], b["ds"], b["h"], b["scene_of_view"], stages=True)          # the defaults are the case's step and n_steps
    for k, t in zip(("depth", "normal", "color", "cls", "n_evaluated"), shim):
        assert TS.bits_equal(t.cpu().numpy(), abi[k]), k
    plain = util.tsdf_render_dev(st, pose, b["ds"], b["h"], b["scene_of_view"], skip=False)
    assert len(plain) == 4 and TS.bits_equal(plain[0].cpu().numpy(), abi["depth"]) and TS.bits_equal(plain[3].cpu().numpy(), abi["cls"])
    bare = util.tsdf_render_dev(dict(st, color_sum=None), pose, b["ds"], b["h"], b["scene_of_view"])
    assert bare[2] is None and TS.bits_equal(bare[1].cpu().numpy(), abi["normal"])
    near = util.tsdf_render_dev(st, pose, b["ds"], b["h"], b["scene_of_view"], d_min=0.5, d_max=3.0, step=0.1, stages=True)
    step, n_steps = util.tsdf_render_steps(b["dims"], b["voxel"], 0.5, 3.0, 0.1)
    want = RS.model_of(b, d_min=0.5, step=step, n_steps=n_steps)
    for k, t in zip(("depth", "normal", "color", "cls", "n_evaluated"), near):
        assert TS.bits_equal(t.cpu().numpy(), want[k]), k
    args = (ts, wt, col, torch.from_numpy(b["origin"]), b["voxel"], pose, torch.from_numpy(b["scene_of_view"]), util.DATASETS[b["ds"]], b["h"])
    op = torch.ops.relpose.tsdf_render(*args, 0.0, 0.0, 0.0, 1, True, True)
    for k, t in zip(("depth", "normal", "color", "cls", "n_evaluated"), op):
        assert TS.bits_equal(t.cpu().numpy(), abi[k]), k
    short = torch.ops.relpose.tsdf_render(ts, wt, None, *args[3:])
    assert short[2].numel() == 0 and short[4].numel() == 0 and torch.equal(short[0], op[0])
    meta = torch.ops.relpose.tsdf_render(*(t.to("meta") if hasattr(t, "to") else t for t in args), 0.0, 0.0, 0.0, 1, True, True)
    for got, ref in zip(meta, op):
        assert got.shape == ref.shape and got.dtype == ref.dtype
    for bad in (dict(scene_of_view=[0, 3, 0, 2]), dict(min_weight=0), dict(d_min=-1.0), dict(step=0.0), dict(step=float("nan"))):
        kw = dict(scene_of_view=b["scene_of_view"])
        kw.update(bad)
        with pytest.raises(ValueError):
            util.tsdf_render_dev(st, pose, b["ds"], b["h"], **kw)
    with pytest.raises(ValueError):
        util.tsdf_render_dev(st, pose, b["ds"], 5, b["scene_of_view"])


# ---------------------------------------------------------------------------------------------- 6. invalid arguments
def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, V, h, nx, ny, nz = 2, 3, 4, 3, 2, 2
    host = AS.host_arrays()
    pose = torch.eye(4, dtype=torch.float64, device=dev()).repeat(V, 1, 1)
    ts = torch.full((S, nz, ny, nx), 1000, dtype=torch.int32, device=dev())
    wt = torch.full((S, nz, ny, nx), 1, dtype=torch.int32, device=dev())
    col = torch.full((S, 3, nz, ny, nx), 100, dtype=torch.int32, device=dev())
    outs = {"depth": torch.full((V, h, 4 * h), -7.0, dtype=torch.float32, device=dev()), "cls": torch.full((V, h, 4 * h), 77, dtype=torch.uint8, device=dev()),
            "normal": torch.full((V, 3, h, 4 * h), -7.0, dtype=torch.float32, device=dev()),
            "color": torch.full((V, 3, h, 4 * h), -7.0, dtype=torch.float32, device=dev()),
            "n_evaluated": torch.full((V, h, 4 * h), -7, dtype=torch.int32, device=dev())}
    ws = torch.empty(L.relpose_tsdf_render_workspace_bytes(S, V, h, nx, ny, nz) + 512, dtype=torch.uint8, device=dev())
    ptrs = {"tsdf_sum": ts.data_ptr(), "weight": wt.data_ptr(), "color_sum": col.data_ptr(), "pose": pose.data_ptr()}
    ptrs.update({k: v.data_ptr() for k, v in outs.items()})
    for name, kw in RS.einval_calls():
        a = RS.render_args(_lib, 0, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
        a.stream = _lib.stream_ptr()
        assert L.relpose_tsdf_render(C.byref(a)) == -1, name
    for args in ((0, V, h, nx, ny, nz), (S, 0, h, nx, ny, nz), (S, V, 5, nx, ny, nz), (S, V, h, 0, ny, nz), (S, 8, 8192, nx, ny, nz),
                 (1, V, h, 1024, 1024, 700)):
        assert L.relpose_tsdf_render_workspace_bytes(*args) == 0, args
    torch.cuda.synchronize()
    assert all(bool((v == (77 if k == "cls" else -7)).all()) for k, v in outs.items())
    a = RS.render_args(_lib, 0, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
    a.stream = _lib.stream_ptr()
    assert L.relpose_tsdf_render(C.byref(a)) == 0                                          # the base call itself is valid
    assert bool((outs["cls"] == 0).all()) and bool((outs["depth"] == 0).all()) and bool((outs["n_evaluated"] >= 0).all())      # t > 0 everywhere: misses


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_render_views_of_a_fused_scene_match_its_scans():
    import torch
    from relativepose_amd import evaluation as E, util
    c = AS.scene("closed32")
    depth, rgb = up(c["depth"], np.float32), up(c["rgb"], np.float32)
    # the scene's own box: the state is the model's (tests/test_gpu_tsdf.py), so the scores are the ones tests/test_render_cpu.py measured
    state = util.tsdf_fuse_dev(depth, rgb, c["R"], c["view_begin"], c["origin"], c["dims"], c["voxel"], "suncg")
    rv = E.render_views(state, c["R"], h=c["h"])
    m = RS.room_model("closed32")
    for k in ("depth", "normal", "color", "cls"):
        assert TS.bits_equal(rv[k].cpu().numpy(), m[k]), k
    (med, p90), cov = E.render_scores(rv["depth"], rv["cls"], depth, c["voxel"])
    want = RS.accuracy("closed32", m, range(len(c["R"])))
    log("tsdf_render_end_to_end", median=med, p90=p90, coverage=cov, want=want)
    assert abs(med - want[0]) < 1e-12 and abs(p90 - want[1]) < 1e-12 and abs(cov - want[2]) < 1e-12
    assert float(rv["color"].min()) >= 0.0 and float(rv["color"].max()) <= 1.0
    assert bool(((rv["depth"] > 0) == (rv["cls"] == 1)).all())
    # the path of the CLI: the box of util.tsdf_bounds_dev (3 voxels beyond the data, as the scene's is beyond the walls).  The pins are
    # tests/test_render_cpu.py's for closed32 against the fusion of all views (measured with the model, x 1.25)
    surf = E.fuse_views(depth, rgb, c["R"], "suncg", c["voxel"])
    rv = E.render_views(surf["state"], c["R"], h=c["h"])
    (med, p90), cov = E.render_scores(rv["depth"], rv["cls"], depth, c["voxel"])
    log("tsdf_render_fuse_views", median=med, p90=p90, coverage=cov, dims=surf["dims"], origin=surf["origin"])
    assert med <= 0.03139 * 1.25 and p90 <= 0.16614 * 1.25 and cov >= 0.97961 / 1.25
    solo = E.render_views(surf["state"], c["R"][:1], "suncg", c["h"], skip=False)
    assert torch.equal(solo["depth"][0], rv["depth"][0]) and torch.equal(solo["normal"][0], rv["normal"][0])
