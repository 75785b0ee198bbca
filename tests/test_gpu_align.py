"""GPU: relpose_tsdf_align (frame-to-model alignment against TSDF volumes) against the numpy model: teacher-forced bit for
bit at every iteration, free-running within the model's own sensitivity, batch independence and repeatability, stride and a one-wave view,
the hand-built edge cases, the operator and the shim against the C ABI, every RELPOSE_EINVAL path with pre-filled outputs, and one
end-to-end refinement of a perturbed view.  Every test runs under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import align_model as AM
import align_scenes as AS
import tsdf_scenes as TS
from gpu_util import log

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few
FILL = {"pose": -7.5, "eig": 9.25, "held": -7, "sums": -3, "rms": -2.5, "trace_pose": 4.5, "trace_sums": -9}
# Measured with the model alone: a one-ulp change of any entry of the start pose moves the refined pose of the pinned cases by at most
# 1.11e-16 (the iteration contracts).  x 4.
FREE_TOL = 4.5e-16
SOLO_CASES = (("closed16", 0, 2), ("closed32", 1, 2), ("suncg16", 0, 2), ("scannet16", 1, 1), ("suncg32", 0, 1))


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


def solo_case(name, v, k):
    c = AS.scene(name)
    return {"state": AS.leave_one_out(name, v), "origin": c["origin"], "dims": c["dims"], "voxel": c["voxel"], "ds": c["ds"],
            "depth": c["depth"][v:v + 1], "pose": AS.start_pose(c, v, k)[None], "scene_of_view": np.zeros(1, np.int32), "h": c["h"]}


def align_raw(case, iters=AS.ITERS, eig_min=AS.EIG_MIN, stride=1, min_weight=1, trace=True, pose=None, depth=None, scene_of_view=None):
    """relpose_tsdf_align through the C ABI into outputs pre-filled with FILL -> the model's output dict (host arrays)"""
    import torch
    from relativepose_amd import _lib, util
    L = _lib.lib()
    ts, wt = up(case["state"]["tsdf_sum"], np.int32), up(case["state"]["weight"], np.int32)
    S, nz, ny, nx = ts.shape
    dep = up(case["depth"] if depth is None else depth, np.float32)
    T = up(case["pose"] if pose is None else pose, np.float64)
    sov = np.ascontiguousarray(case["scene_of_view"] if scene_of_view is None else scene_of_view, dtype=np.int32)
    V, h = dep.shape[0], dep.shape[1]
    nbytes = L.relpose_tsdf_align_workspace_bytes(S, V, h, nx, ny, nz, stride)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    shapes = {"pose": ((V, 4, 4), torch.float64), "eig": ((V, 6), torch.float64), "held": ((V,), torch.int32), "sums": ((V, 32), torch.int64),
              "rms": ((V, 2), torch.float64), "trace_pose": ((V, iters + 1, 4, 4), torch.float64), "trace_sums": ((V, iters + 1, 32), torch.int64)}
    out = {k: torch.full(s, FILL[k], dtype=dt, device=dev()) for k, (s, dt) in shapes.items() if trace or not k.startswith("trace")}
    org = np.ascontiguousarray(case["origin"], dtype=np.float64).reshape(S, 3)
    a = _lib.TsdfAlignArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.n_views, a.h, a.dataset, a.nx, a.ny, a.nz = S, V, h, util.DATASETS[case["ds"]], nx, ny, nz
    a.min_weight, a.iters, a.stride = min_weight, iters, stride
    a.tsdf_sum, a.weight, a.depth, a.pose = ts.data_ptr(), wt.data_ptr(), dep.data_ptr(), T.data_ptr()
    a.origin_host, a.scene_of_view_host = org.ctypes.data, sov.ctypes.data
    a.voxel, a.eig_min = case["voxel"], eig_min
    a.pose_out, a.eig, a.held, a.sums, a.rms = (out[k].data_ptr() for k in ("pose", "eig", "held", "sums", "rms"))
    a.trace_pose, a.trace_sums = (out["trace_pose"].data_ptr(), out["trace_sums"].data_ptr()) if trace else (0, 0)
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_tsdf_align(C.byref(a)) == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(name, got, want, keys=AS.OUT_KEYS + AS.TRACE_KEYS):
    bad = TS.differ(got, want, keys)
    log("tsdf_align_" + name, differ=bad, classes=got["sums"][:, 28:], want_classes=want["sums"][:, 28:], held=got["held"], want_held=want["held"],
        pose_diff=float(np.nanmax(np.abs(got["pose"] - want["pose"]))) if np.isfinite(want["pose"]).all() else None)
    assert bad == [], (name, bad)


# ---------------------------------------------------------------------------------------------- 1. teacher-forced
@pytest.mark.parametrize("name,v,k", SOLO_CASES)
def test_teacher_forced_every_iteration_matches_the_model_bitwise(name, v, k):
    """One iters = 1 call per iteration, started from the MODEL's pose of that iteration (the iterations ride as the views of one batch):
    the sums of that evaluation, the stepped pose and the sums at the stepped pose are the model's, bit for bit."""
    c = solo_case(name, v, k)
    m = AS.solo(name, v, k)
    E = AS.ITERS
    got = align_raw(c, iters=1, pose=m["trace_pose"][0, :E], depth=np.repeat(c["depth"], E, 0), scene_of_view=np.zeros(E, np.int32))
    sums_ok = TS.bits_equal(got["trace_sums"][:, 0], m["trace_sums"][0, :E]) and TS.bits_equal(got["trace_sums"][:, 1], m["trace_sums"][0, 1:])
    pose_ok = TS.bits_equal(got["pose"], m["trace_pose"][0, 1:]) and TS.bits_equal(got["trace_pose"][:, 0], m["trace_pose"][0, :E])
    log(f"tsdf_align_teacher_{name}_{v}", sums_ok=sums_ok, pose_ok=pose_ok, used=got["trace_sums"][:, 0, AM.USED],
        pose_diff=float(np.abs(got["pose"] - m["trace_pose"][0, 1:]).max()),
        first_bad_sum=np.argwhere(got["trace_sums"][:, 0] != m["trace_sums"][0, :E])[:4])
    assert sums_ok and pose_ok
    for e in range(E):                                                          # held and eig at the stepped pose are the next evaluation's
        st = m["steps"][0][e + 1]
        assert got["held"][e] == st["held"] and TS.bits_equal(got["eig"][e], st["eig"])
        assert got["rms"][e, 0] == AM.rms(m["trace_sums"][0, e]) and got["rms"][e, 1] == AM.rms(m["trace_sums"][0, e + 1])


# ---------------------------------------------------------------------------------------------- 2. free-running
@pytest.mark.parametrize("name,v,k", SOLO_CASES)
def test_free_running_stays_with_the_model(name, v, k):
    m = AS.solo(name, v, k)
    got = align_raw(solo_case(name, v, k))
    diff = float(np.abs(got["pose"] - m["pose"]).max())
    log(f"tsdf_align_free_{name}_{v}", pose_diff=diff, bitwise=TS.differ(got, m, AS.OUT_KEYS + AS.TRACE_KEYS), held=got["held"], rms=got["rms"],
        displacement=AS.displacement(AS.scene(name), v, got["pose"][0]))
    assert diff <= FREE_TOL
    assert got["held"][0] == m["held"][0] and (got["sums"][0, 28:] == m["sums"][0, 28:]).all()
    # one flipped llrint changes one of ~10^3 rows by one part in 2^8 .. 2^16: the sums, and with them eig and rms, agree far inside 1e-6
    assert np.allclose(got["eig"], m["eig"], rtol=1e-6, atol=0) and np.allclose(got["rms"], m["rms"], rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- 3. the batch
def test_batch_equals_its_members_and_repeats_bitwise():
    b = AS.batch()
    want = AS.model_of(b)
    got = align_raw(b)
    check("batch", got, want)
    assert (got["sums"][2, 28:] == [1024, 0, 0, 0]).all() and got["held"][2] == 6        # every point outside
    assert got["sums"][3, AM.USED] == 5 and got["held"][3] == 6                           # fewer than 6 used points: nothing moves
    assert TS.bits_equal(got["pose"][2:4], b["pose"][2:4])
    assert not (b["scene_of_view"] == 1).any()                                            # scene 1 has no view
    again = align_raw(b)
    assert TS.differ(again, got, AS.OUT_KEYS + AS.TRACE_KEYS) == []
    for v in range(len(b["depth"])):
        one = align_raw(AS.batch_member(v))
        for k in AS.OUT_KEYS + AS.TRACE_KEYS:
            assert TS.bits_equal(one[k][0], got[k][v]), (v, k)
    no_trace = align_raw(b, trace=False)
    assert set(no_trace) == set(AS.OUT_KEYS) and TS.differ(no_trace, got, AS.OUT_KEYS) == []
    in_place = align_raw(b, iters=0)
    assert TS.bits_equal(in_place["pose"], b["pose"]) and TS.bits_equal(in_place["sums"], got["trace_sums"][:, 0])       # iters = 0 scores the poses
    assert TS.bits_equal(in_place["rms"][:, 0], in_place["rms"][:, 1])


# ---------------------------------------------------------------------------------------------- 4. / 5. stride, small h, the edge cases
@pytest.mark.parametrize("stride", [1, 3])
def test_stride_matches_the_model(stride):
    b = AS.batch()
    check(f"stride_{stride}", align_raw(b, iters=3, stride=stride), AS.model_of(b, iters=3, stride=stride))
    c = solo_case("closed32", 2, 1)                                                       # four workgroups per view, the last one partial at stride 3
    want = AM.align(c["state"], c["origin"], c["voxel"], c["depth"], c["pose"], c["ds"], None, 2, AS.EIG_MIN, stride)
    check(f"closed32_stride_{stride}", align_raw(c, iters=2, stride=stride), want)


@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
@pytest.mark.parametrize("h", [2, 4])
def test_edge_cases_get_what_the_contract_gives(ds, h):
    """NaN / inf / 0 / negative depths, a NaN and an inf in a pose, a corner with |t| = 1, a weight of min_weight - 1, u exactly integer, the
    last cell and one past it; h = 2 is one partial wave of 16 pixels."""
    e = AS.edge_case(ds, h)
    for stride in (1, 3):
        want = AS.model_of(e, iters=2, stride=stride, min_weight=2)
        got = align_raw(e, iters=2, stride=stride, min_weight=2)
        check(f"edge_{ds}_{h}_{stride}", got, want)
    assert (want["sums"][1:, AM.OUTSIDE] == want["sums"][1:, 28:].sum(1)).all()           # the non-finite poses: every point outside ...
    assert np.array_equal(np.isnan(got["pose"][1]), np.isnan(e["pose"][1])) and np.array_equal(np.isinf(got["pose"][2]), np.isinf(e["pose"][2]))


# ---------------------------------------------------------------------------------------------- 6. operator and shim
def test_operator_and_shim_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import ops, util
    assert "tsdf_align" in ops.OPS
    b = AS.batch()
    abi = align_raw(b, iters=4, stride=2)
    ts, wt = up(b["state"]["tsdf_sum"], np.int32), up(b["state"]["weight"], np.int32)
    depth, pose = up(b["depth"], np.float32), up(b["pose"], np.float64)
    st = {"tsdf_sum": ts, "weight": wt, "color_sum": None, "origin": b["origin"], "dims": b["dims"], "voxel": b["voxel"], "dataset": b["ds"]}
    shim = util.tsdf_align_dev(st, depth, b["pose"], b["scene_of_view"], iters=4, stride=2, trace=True)
    assert TS.differ({k: v.cpu().numpy() for k, v in shim.items()}, abi, AS.OUT_KEYS + AS.TRACE_KEYS) == []
    op = torch.ops.relpose.tsdf_align(ts, wt, torch.from_numpy(b["origin"]), b["voxel"], depth, pose, torch.from_numpy(b["scene_of_view"]),
                                      util.DATASETS[b["ds"]], 4, AS.EIG_MIN, 2, 1, True)
    for k, t in zip(AS.OUT_KEYS + AS.TRACE_KEYS, op):
        assert TS.bits_equal(t.cpu().numpy(), abi[k]), k
    plain = torch.ops.relpose.tsdf_align(ts, wt, torch.from_numpy(b["origin"]), b["voxel"], depth, pose, torch.from_numpy(b["scene_of_view"]).to(dev()),
                                         util.DATASETS[b["ds"]], 4, AS.EIG_MIN, 2)
    assert plain[5].numel() == 0 and plain[6].numel() == 0 and torch.equal(plain[0], op[0])
    meta = torch.ops.relpose.tsdf_align(ts.to("meta"), wt.to("meta"), torch.from_numpy(b["origin"]).to("meta"), b["voxel"], depth.to("meta"),
                                        pose.to("meta"), torch.from_numpy(b["scene_of_view"]).to("meta"), util.DATASETS[b["ds"]], 4, AS.EIG_MIN, 2, 1, True)
    for got, ref in zip(meta, op):
        assert got.shape == ref.shape and got.dtype == ref.dtype
    default = util.tsdf_align_dev(st, depth[:1], pose[:1])                                # scene 0, 12 iterations, the default floor
    assert TS.bits_equal(default["pose"].cpu().numpy()[0], AS.solo("closed16", 0, 2)["pose"][0])
    for bad in (dict(scene_of_view=[0, 3, 0, 2, 2]), dict(iters=65), dict(stride=0), dict(eig_min=-1.0), dict(min_weight=0)):
        kw = dict(scene_of_view=b["scene_of_view"])
        kw.update(bad)
        with pytest.raises(ValueError):
            util.tsdf_align_dev(st, depth, pose, **kw)


# ---------------------------------------------------------------------------------------------- 7. invalid arguments
def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, V, h, nx, ny, nz, iters = 2, 3, 4, 3, 2, 2, 2
    host = AS.host_arrays()
    depth = torch.full((V, h, 4 * h), 0.4, dtype=torch.float32, device=dev())
    pose = torch.eye(4, dtype=torch.float64, device=dev()).repeat(V, 1, 1)
    ts = torch.full((S, nz, ny, nx), 1000, dtype=torch.int32, device=dev())
    wt = torch.full((S, nz, ny, nx), 1, dtype=torch.int32, device=dev())
    outs = {"pose_out": torch.full((V, 4, 4), -7.0, dtype=torch.float64, device=dev()), "eig": torch.full((V, 6), -7.0, dtype=torch.float64, device=dev()),
            "held": torch.full((V,), -7, dtype=torch.int32, device=dev()), "sums": torch.full((V, 32), -7, dtype=torch.int64, device=dev()),
            "rms": torch.full((V, 2), -7.0, dtype=torch.float64, device=dev()),
            "trace_pose": torch.full((V, iters + 1, 4, 4), -7.0, dtype=torch.float64, device=dev()),
            "trace_sums": torch.full((V, iters + 1, 32), -7, dtype=torch.int64, device=dev())}
    ws = torch.empty(L.relpose_tsdf_align_workspace_bytes(S, V, h, nx, ny, nz, 1) + 512, dtype=torch.uint8, device=dev())
    ptrs = {"tsdf_sum": ts.data_ptr(), "weight": wt.data_ptr(), "depth": depth.data_ptr(), "pose": pose.data_ptr()}
    ptrs.update({k: v.data_ptr() for k, v in outs.items()})
    for name, kw in AS.einval_calls():
        a = AS.align_args(_lib, 0, host, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
        a.stream = _lib.stream_ptr()
        assert L.relpose_tsdf_align(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values())
    a = AS.align_args(_lib, 0, host, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, ptrs=ptrs)
    a.stream = _lib.stream_ptr()
    assert L.relpose_tsdf_align(C.byref(a)) == 0                                           # the base call itself is valid
    assert (outs["sums"][:, 28:].sum(1) == 4 * h * h).all() and (outs["held"] >= 0).all() and (outs["rms"] >= 0).all()


# ---------------------------------------------------------------------------------------------- 8. end to end
def test_refine_scene_pulls_a_perturbed_view_back():
    import torch
    from relativepose_amd import evaluation as E, util
    c = AS.scene("closed32")
    depth = up(c["depth"], np.float32)
    R = c["R"].copy()
    R[0] = AS.start_pose(c, 0, 2)
    before = AS.displacement(c, 0, R[0])
    # leave-one-out by subtraction is the direct fusion of the others, bit for bit, on the device too
    V = len(R)
    vb1 = np.arange(V + 1, dtype=np.int32)
    both = util.tsdf_fuse_dev(depth, None, R, [0, V], c["origin"], c["dims"], c["voxel"], "suncg")
    solo = util.tsdf_fuse_dev(depth, None, R, vb1, np.repeat(c["origin"], V, 0), c["dims"], c["voxel"], "suncg")
    loo = E.leave_one_out_state(both, solo)
    for v in range(V):
        o = [u for u in range(V) if u != v]
        direct = util.tsdf_fuse_dev(depth[o], None, R[o], [0, V - 1], c["origin"], c["dims"], c["voxel"], "suncg")
        assert torch.equal(direct["tsdf_sum"][0], loo["tsdf_sum"][v]) and torch.equal(direct["weight"][0], loo["weight"][v])
    out = E.refine_scene(depth, R, "suncg", c["voxel"], rounds=1)
    after = AS.displacement(c, 0, out["pose"][0])
    wall = []
    for P in (R, out["pose"]):
        sf = E.fuse_views(depth, None, P, "suncg", c["voxel"])
        wall.append(TS.wall_stats(sf["points"][0, :int(sf["n_points"][0])].cpu().numpy(), c["half"], c["voxel"])[0])
    others = [AS.displacement(c, v, out["pose"][v]) for v in range(1, V)]
    log("tsdf_align_refine_scene", before=before, after=after, wall=wall, others=others, held=out["held"], rms=out["rms"])
    assert wall[1] <= wall[0]
    assert after < before / 10                                                  # the CPU test's pinned improvement at h = 32
    assert (out["held"] == 0).all() and out["rms"][0, 1] < out["rms"][0, 0]
    scored = E.refine_scene(depth, R, "suncg", c["voxel"], rounds=0)
    assert TS.bits_equal(scored["pose"], R)
