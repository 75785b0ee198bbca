"""GPU: relpose_visibility (visibility consistency of relative poses) against the numpy model bit for bit on the pinned
scenes and the hand-built edge cases, its batch invariance and repeatability, the operator and the shims against the C ABI, every
RELPOSE_EINVAL path with pre-filled outputs, and the evaluation drivers built on it."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import visibility_model as VM
import visibility_scenes as VS
from gpu_util import log
from relativepose_amd import synth, weights

pytestmark = pytest.mark.gpu

ALL_SCENES = VS.SCENES + VS.BITWISE_ONLY
KEYS = ("counts", "margin_sum", "cls")


def dev():
    import torch
    return torch.device("cuda:0")


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


def as_dict(out):
    return {k: v.cpu().numpy() for k, v in zip(KEYS, out)}


def run(pc, valid, depth, qc, rv, pose, ds, tol_abs=0.05, tol_rel=0.02, radius=1):
    """util.visibility_dev on numpy inputs -> the model's result dict"""
    from relativepose_amd import util
    return as_dict(util.visibility_dev(up(pc, np.float64), None if valid is None else up(valid, np.uint8), up(depth, np.float32), qc, rv,
                                       up(pose, np.float64), ds, tol_abs, tol_rel, radius, want_class=True))


def check(name, want, got):
    bad = VS.same(got, want)
    log("visibility_" + name, differ=bad, counts=got["counts"].sum(0), want_counts=want["counts"].sum(0),
        margin=int(got["margin_sum"].sum()), want_margin=int(want["margin_sum"].sum()))
    assert bad == [], (name, bad, got["counts"].tolist(), want["counts"].tolist())


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("wrong", [False, True])
@pytest.mark.parametrize("ds,h", ALL_SCENES)
def test_scene_queries_match_the_model_bitwise(ds, h, wrong, radius):
    s = VS.scene(ds, h)
    want = VS.model(ds, h, radius, wrong)
    got = run(s["pc"], s["valid"], s["depth"], s["qc"], s["rv"], s["W" if wrong else "T"], ds, radius=radius)
    check(f"scene_{ds}_{h}_{int(wrong)}_{radius}", want, got)
    if radius == 1:
        assert VS.totals(got) == VS.PINNED[(ds, h)][int(wrong)]


@pytest.mark.parametrize("tol", [(0.05, 0.02), (0.0, 0.0), (0.0, 0.3), (1.5, 0.0)])
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("ds", ["suncg", "matterport", "scannet"])
def test_edge_cases_match_the_model_bitwise(ds, radius, tol):
    """visibility_scenes.edge_case: points on each bound and one ulp to either side, |xn| = 1, Z = 0, exact half pixels, d at and just
    below 32768, NaN / inf in cloud and pose, reference depths 0 / -1 / NaN / inf / huge, windows at the seam columns and the first and last
    row, a window with only its centre, 1536 points on one pixel in one class, an all-invalid cloud."""
    e = VS.edge_case(ds)
    want = VM.visibility(e["pc"], e["valid"], e["depth"], e["qc"], e["rv"], e["pose"], ds, tol[0], tol[1], radius)
    got = run(e["pc"], e["valid"], e["depth"], e["qc"], e["rv"], e["pose"], ds, tol[0], tol[1], radius)
    check(f"edge_{ds}_{radius}_{tol}", want, got)
    if tol == (0.05, 0.02) and radius == 1:
        sp = VS.special_points(ds)
        assert got["cls"][0][:len(sp)].tolist() == [w for _, _, w in sp]
        assert got["counts"][3].tolist() == [0, 0, 0, VS.EDGE_P, 0, 0] and got["counts"][4].tolist() == [0, 0, 0, 0, VS.EDGE_P, 0]
        assert got["counts"][5].tolist() == [VS.EDGE_P, 0, 0, 0, 0, 0]


def test_valid_null_means_all_valid():
    s = VS.scene("matterport", 32)
    want = VM.visibility(s["pc"], None, s["depth"], s["qc"], s["rv"], s["W"], "matterport")
    check("null_valid", want, run(s["pc"], None, s["depth"], s["qc"], s["rv"], s["W"], "matterport"))
    assert (want["counts"][:, 0] == 0).all()


def test_64_queries_sharing_one_view_equal_the_same_queries_one_per_call_and_repeat_bitwise():
    s = VS.scene("suncg", 32)
    rs = np.random.RandomState(2)
    qc = rs.randint(0, VS.SCENE_VIEWS, 64)
    rv = np.full(64, 2)
    pose = np.stack([np.matmul(synth.random_rigid(rs, 0.5, 0.5), np.matmul(s["R"][2], np.linalg.inv(s["R"][c]))) for c in qc])
    a = run(s["pc"], s["valid"], s["depth"], qc, rv, pose, "suncg")
    b = run(s["pc"], s["valid"], s["depth"], qc, rv, pose, "suncg")
    assert VS.same(a, b) == []                                                 # two runs of one call
    check("batch64", VM.visibility(s["pc"], s["valid"], s["depth"], qc, rv, pose, "suncg"), a)
    for k in range(64):                                                        # a query's row does not depend on the batch around it
        one = run(s["pc"], s["valid"], s["depth"], qc[k:k + 1], rv[k:k + 1], pose[k:k + 1], "suncg")
        assert all(np.array_equal(one[key][0], a[key][k]) for key in KEYS), k
    assert len({tuple(r) for r in a["counts"].tolist()}) > 32


def test_operator_and_shims_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import _lib, ops, util  # noqa: F401
    ds, h = "matterport", 32
    s = VS.scene(ds, h)
    pc, valid, depth, pose = up(s["pc"], np.float64), up(s["valid"], np.uint8), up(s["depth"], np.float32), up(s["W"], np.float64)
    Q, P = len(s["qc"]), s["pc"].shape[1]
    # the C ABI, driven by hand
    L = _lib.lib()
    nbytes = L.relpose_visibility_workspace_bytes(VS.SCENE_VIEWS, h, Q)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    counts = torch.full((Q, 6), -7, dtype=torch.int32, device=dev())
    margin = torch.full((Q,), -7, dtype=torch.int64, device=dev())
    cls = torch.full((Q, P), 99, dtype=torch.uint8, device=dev())
    a = _lib.VisibilityArgs()
    a.struct_size = C.sizeof(a)
    a.n_clouds, a.n_points, a.n_views, a.h, a.n_queries, a.dataset, a.radius = VS.SCENE_VIEWS, P, VS.SCENE_VIEWS, h, Q, util.DATASETS[ds], 1
    a.pc, a.valid, a.depth, a.pose = pc.data_ptr(), valid.data_ptr(), depth.data_ptr(), pose.data_ptr()
    a.query_cloud_host, a.ref_view_host = s["qc"].ctypes.data, s["rv"].ctypes.data
    a.tol_abs, a.tol_rel = 0.05, 0.02
    a.counts, a.margin_sum, a.cls = counts.data_ptr(), margin.data_ptr(), cls.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_visibility(C.byref(a)) == 0
    abi = as_dict((counts, margin, cls))
    check("c_abi", VS.model(ds, h, 1, True), abi)
    assert (abi["counts"].sum(1) == P).all()
    # the operator
    qc_t, rv_t = torch.from_numpy(s["qc"]).to(dev()), torch.from_numpy(s["rv"]).to(dev())         # read back on the host by the operator
    op = as_dict(torch.ops.relpose.visibility(pc, valid, depth, qc_t, rv_t, pose, util.DATASETS[ds], 0.05, 0.02, 1))
    assert VS.same(op, abi) == []
    op0 = as_dict(torch.ops.relpose.visibility(pc, valid, depth, qc_t, rv_t, pose, util.DATASETS[ds], 0.0, 0.0, 0))
    assert VS.same(op0, VS.model(ds, h, 0, True, 0.0, 0.0)) == []
    # the Meta shapes
    m = torch.ops.relpose.visibility(pc.to("meta"), valid.to("meta"), depth.to("meta"), qc_t.to("meta"), rv_t.to("meta"), pose.to("meta"),
                                     util.DATASETS[ds])
    for got, want in zip(m, (counts, margin, cls)):
        assert got.shape == want.shape and got.dtype == want.dtype
    # visibility_dev without the classes, and its scores against the model's
    c2, m2 = util.visibility_dev(pc, valid, depth, s["qc"], s["rv"], pose, ds)
    assert np.array_equal(c2.cpu().numpy(), abi["counts"]) and np.array_equal(m2.cpu().numpy(), abi["margin_sum"])
    sc, want = util.visibility_scores(c2, m2), VM.scores(abi["counts"], abi["margin_sum"])
    for k in want:
        assert np.array_equal(sc[k].cpu().numpy(), want[k], equal_nan=True), k


def test_empty_inputs_return_without_a_launch():
    import torch
    from relativepose_amd import util
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev())
    depth = z(2, 16, 64, dt=torch.float32)
    c, m, k = util.visibility_dev(z(2, 10, 3, dt=torch.float64), None, depth, [], [], z(0, 4, 4, dt=torch.float64), "suncg", want_class=True)
    assert c.shape == (0, 6) and m.shape == (0,) and k.shape == (0, 10)
    c, m = util.visibility_dev(z(2, 0, 3, dt=torch.float64), None, depth, [0, 1], [1, 0], z(2, 4, 4, dt=torch.float64), "suncg")
    assert c.shape == (2, 6) and (c == 0).all() and (m == 0).all()
    c, m = util.visibility_dev(z(0, 5, 3, dt=torch.float64), None, depth, [], [], z(0, 4, 4, dt=torch.float64), "suncg")
    assert c.shape == (0, 6)
    for bad in (dict(radius=3), dict(tol_abs=-1.0), dict(tol_rel=float("nan"))):
        with pytest.raises(ValueError):
            util.visibility_dev(z(2, 10, 3, dt=torch.float64), None, depth, [0], [1], z(1, 4, 4, dt=torch.float64), "suncg", **bad)
    with pytest.raises(ValueError):                                            # a view index out of range
        util.visibility_dev(z(2, 10, 3, dt=torch.float64), None, depth, [0], [2], z(1, 4, 4, dt=torch.float64), "suncg")
    with pytest.raises(ValueError):                                            # h odd
        util.visibility_dev(z(2, 10, 3, dt=torch.float64), None, z(2, 15, 60, dt=torch.float32), [0], [1], z(1, 4, 4, dt=torch.float64), "suncg")


def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    n, P, V, h, Q = 2, 8, 2, 4, 2
    pc = torch.randn(n, P, 3, dtype=torch.float64, device=dev())
    valid = torch.ones(n, P, dtype=torch.uint8, device=dev())
    depth = torch.full((V, h, 4 * h), 2.0, dtype=torch.float32, device=dev())
    pose = torch.eye(4, dtype=torch.float64, device=dev()).repeat(Q, 1, 1)
    ws = torch.empty(L.relpose_visibility_workspace_bytes(V, h, Q) + 512, dtype=torch.uint8, device=dev())
    counts = torch.full((Q, 6), -7, dtype=torch.int32, device=dev())
    margin = torch.full((Q,), -7, dtype=torch.int64, device=dev())
    cls = torch.full((Q, P), 99, dtype=torch.uint8, device=dev())
    qc, rv = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 0)
    idx = {"bad_q": (C.c_int32 * 2)(0, -1), "bad_r": (C.c_int32 * 2)(0, 2)}
    long_idx = (C.c_int32 * (1 << 15))()

    def args(**kw):
        a = _lib.VisibilityArgs()
        a.struct_size = C.sizeof(a)
        a.n_clouds, a.n_points, a.n_views, a.h, a.n_queries, a.dataset, a.radius = n, P, V, h, Q, 0, 1
        a.tol_abs, a.tol_rel = 0.05, 0.02
        a.pc, a.valid, a.depth, a.pose = pc.data_ptr(), valid.data_ptr(), depth.data_ptr(), pose.data_ptr()
        a.counts, a.margin_sum, a.cls = counts.data_ptr(), margin.data_ptr(), cls.data_ptr()
        a.query_cloud_host, a.ref_view_host = C.addressof(qc), C.addressof(rv)
        a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws.numel() - 256, _lib.stream_ptr()
        for k, v in kw.items():
            if k == "workspace_offset":
                a.workspace = ws.data_ptr() + v
            else:
                setattr(a, k, C.addressof(idx[v]) if isinstance(v, str) else v)
        if kw.get("n_queries", 0) > 2:
            a.query_cloud_host = a.ref_view_host = C.addressof(long_idx)
        return a

    calls = VS.einval_calls()
    assert len(calls) > 35
    for name, kw in calls:
        assert L.relpose_visibility(C.byref(args(**kw))) == -1, name
    torch.cuda.synchronize()
    assert (counts == -7).all() and (margin == -7).all() and (cls == 99).all()
    assert L.relpose_visibility(C.byref(args())) == 0                          # the base call itself is valid
    assert (counts.sum(1) == P).all() and (cls < 6).all() and (margin >= 0).all()


def test_pose_visibility_dev_against_separate_calls():
    from relativepose_amd import util
    ds, h = "suncg", 32
    s = VS.scene(ds, h)
    B, K = 2, 3
    pc, valid, depth = up(s["pc"], np.float64), up(s["valid"], np.uint8), up(s["depth"], np.float32)
    rs = np.random.RandomState(4)
    T = np.empty((B, K, 4, 4))
    for b in range(B):
        gt = np.matmul(s["R"][2 * b + 1], np.linalg.inv(s["R"][2 * b]))
        T[b] = [gt, np.matmul(synth.random_rigid(rs, 0.6, 0.5), gt), np.matmul(synth.random_rigid(rs, 0.1, 0.1), gt)]
    counts, margin, sc = util.pose_visibility_dev(pc, valid, depth, T, ds)
    assert counts.shape == (B, K, 2, 6) and margin.shape == (B, K, 2) and all(v.shape == (B, K) for v in sc.values())
    counts, margin = counts.cpu().numpy(), margin.cpu().numpy()
    for b in range(B):
        for k in range(K):
            for d, (q, r, pose) in enumerate(((2 * b, 2 * b + 1, T[b, k]), (2 * b + 1, 2 * b, np.linalg.inv(T[b, k])))):
                c1, m1 = util.visibility_dev(pc, valid, depth, [q], [r], up(pose[None], np.float64), ds)
                assert np.array_equal(c1.cpu().numpy()[0], counts[b, k, d]) and m1.cpu().numpy()[0] == margin[b, k, d], (b, k, d)
    want = VM.scores(counts.sum(2), margin.sum(2))
    for key in want:
        assert np.array_equal(sc[key].cpu().numpy(), want[key], equal_nan=True), key
    ag = sc["agreement"].cpu().numpy()
    assert (ag[:, 0] > 0.99).all() and (ag[:, 1] < 0.9).all()                  # the true pose agrees, the wrong one does not
    from relativepose_amd import evaluation as E
    assert E.select_pose(sc).tolist() == [int(np.argmax(ag[b])) for b in range(B)]


def test_visibility_matrix_dev_against_its_pairwise_calls():
    from relativepose_amd import util
    ds, h = "matterport", 32
    s = VS.scene(ds, h)
    M = VS.SCENE_VIEWS
    pc, valid, depth = up(s["pc"], np.float64), up(s["valid"], np.uint8), up(s["depth"], np.float32)
    counts, margin, sc = util.visibility_matrix_dev(pc, valid, depth, s["R"], ds)
    assert counts.shape == (M, M, 6) and margin.shape == (M, M) and sc["agreement"].shape == (M, M)
    want = VS.model(ds, h, 1, False)                                           # the same M (M - 1) queries, T_ij = R_j inv(R_i)
    counts, margin = counts.cpu().numpy(), margin.cpu().numpy()
    for k in range(len(s["qc"])):
        i, j = s["qc"][k], s["rv"][k]
        c1, m1 = util.visibility_dev(pc, valid, depth, [i], [j], up(s["T"][k:k + 1], np.float64), ds)
        assert np.array_equal(c1.cpu().numpy()[0], counts[i, j]) and m1.cpu().numpy()[0] == margin[i, j]
        assert np.array_equal(counts[i, j], want["counts"][k]) and margin[i, j] == want["margin_sum"][k]
    d = np.arange(M)
    assert (counts[d, d] == 0).all() and np.isnan(sc["agreement"].cpu().numpy()[d, d]).all()


@pytest.fixture(scope="module")
def eval_runs():
    """The smallest configuration the pipeline tests use (one batch of suncg pairs at 160 x 640, 60 keypoints, the synthetic weights):
    evaluate_pairs with verify None / "observed" / "completed", and the pieces the explicit calls need."""
    from relativepose_amd import evaluation as E
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline
    ds, mm, S = "suncg", "second", 15
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(7, S))
    pipe = RelativePosePipeline(net, ds, mm)
    batch = synth.make_pairs(2, 1000, ds)
    batch["pts"], batch["ptw"] = synth.make_keypoints(2, 60, 1000, mm)
    recs = {v: E.evaluate_pairs(pipe, [batch], dev(), verify=v) for v in (None, "observed", "completed")}
    return pipe, batch, recs


def _same_record(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        same = np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if not isinstance(x, str) else x == y
        assert same, k


OLD_KEYS = ('img_src', 'img_tgt', 'err_ad', 'err_t', 'err_blind', 'err_t_blind', 'overlap', 'pc_dist', 'cam_dist', 'pc_nearest', 'R_gt', 'R_pred_44')
NEW_KEYS = ('vis_agreement', 'vis_violation_rate', 'vis_observed', 'vis_counts', 'vis_level', 'R_pred_44_selected')


def test_evaluate_pairs_without_verify_gives_the_records_it_gave(eval_runs):
    """verify=None: the keys and values of the unchanged record builder (_default_record on the poses of an unchanged pipe.run)."""
    from relativepose_amd import evaluation as E
    pipe, batch, recs = eval_runs
    st = pipe.prepare(batch["rgb"], batch["norm"], batch["depth"], batch["pts"], batch["ptw"], dev())
    pose = pipe.run(st)[0].cpu().numpy()
    old = E._default_record(pipe, batch, pose, dev(), None, [0, 1])
    assert len(recs[None]) == 2
    for a, b in zip(recs[None], old):
        assert tuple(a) == OLD_KEYS == tuple(b)
        _same_record(a, b, OLD_KEYS)
    for v in ("observed", "completed"):                                        # and the new fields leave the old ones alone
        for a, b in zip(recs[v], recs[None]):
            assert tuple(a) == OLD_KEYS + NEW_KEYS
            _same_record(a, b, OLD_KEYS)


@pytest.mark.parametrize("verify", ["observed", "completed"])
def test_evaluate_pairs_verify_fields_equal_an_explicit_call(eval_runs, verify):
    import torch
    from relativepose_amd import evaluation as E, util
    pipe, batch, recs = eval_runs
    st = pipe.prepare(batch["rgb"], batch["norm"], batch["depth"], batch["pts"], batch["ptw"], dev())
    keep = []
    _, _, trace = pipe.run(st, keep=keep)
    h = st["h"]
    if verify == "observed":
        ref = util.build_view_dev(st["rgb"], st["norm"], st["depth"], pipe.mask_method)[:, 6].contiguous()
        assert (ref[:, :, :h] == 0).all() and (ref[:, :, 2 * h:] == 0).all() and torch.equal(ref[:, :, h:2 * h], st["depth"][:, :, h:2 * h])
    else:
        m = torch.zeros(h, 4 * h, device=dev())
        m[:, h:2 * h] = 1
        ref = ((1 - m) * keep[-1]["f"][:, 6] + m * st["depth"]).contiguous()
    pcs, valid = util.depth2pc_dev(st["depth"], pipe.dataset)
    levels = np.stack([t.cpu().numpy() for t in trace], 1)
    counts, margin, sc = util.pose_visibility_dev(pcs, valid, ref, levels, pipe.dataset)
    pick = E.select_pose(sc)
    counts = counts.sum(2).cpu().numpy()
    for b, rec in enumerate(recs[verify]):
        assert np.array_equal(rec['R_pred_44'][:3], levels[b, -1][:3])
        for key, name in (("agreement", "vis_agreement"), ("violation_rate", "vis_violation_rate"), ("observed", "vis_observed")):
            assert np.array_equal(np.float64(rec[name]), sc[key].cpu().numpy()[b, -1], equal_nan=True), name
        assert np.array_equal(rec['vis_counts'], counts[b, -1]) and rec['vis_counts'].sum() == 2 * pcs.shape[1]
        assert rec['vis_level'] == pick[b] and np.array_equal(rec['R_pred_44_selected'], levels[b, pick[b]])
    s = E.verify_summary(recs[verify])
    assert set(s) == {"vis_spearman_rot", "vis_spearman_trans", "vis_selected"}
    log("visibility_eval", verify=verify, agreement=[r['vis_agreement'] for r in recs[verify]], level=[r['vis_level'] for r in recs[verify]])


def test_mine_pairs_with_verify_adds_the_agreement():
    from relativepose_amd import evaluation as E
    sc = synth.render_scene(7, 4, "suncg", 32)
    plain = E.mine_pairs(sc["depth"], sc["R"], "suncg", "room", device=dev())
    ver = E.mine_pairs(sc["depth"], sc["R"], "suncg", "room", device=dev(), verify="observed")
    assert [{k: v for k, v in e.items() if k != 'vis_agreement'} for e in ver] == plain
    from relativepose_amd import util
    d = up(sc["depth"], np.float32)
    od = E.observed_depth(d, "suncg")
    want = sc["depth"].copy()
    want[:, :, :32] = 0
    want[:, :, 64:] = 0
    assert np.array_equal(od.cpu().numpy(), want)
    pc, valid = util.depth2pc_dev(d, "suncg")
    counts = util.visibility_matrix_dev(pc, valid, od, sc["R"], "suncg")[0].cpu().numpy()
    for e in ver:
        c = counts[e['id_src'], e['id_tgt']] + counts[e['id_tgt'], e['id_src']]
        seen = int(c[3:].sum())
        assert (np.isnan(e['vis_agreement']) and seen == 0) or e['vis_agreement'] == c[3] / seen
    assert sum(1 for e in ver if not np.isnan(e['vis_agreement'])) >= 3
