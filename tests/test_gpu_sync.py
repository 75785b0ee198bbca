"""GPU: relpose_pose_sync (robust synchronisation of pose graphs) against the numpy model -- the integer outputs bit for
bit, the float outputs within 1000 x the model's own sensitivity to one-ulp input noise (tests/sync_scenes.py SENS; the device's sin and
atan2 are not numpy's) -- on every pinned graph and a 64-view, 4096-edge scene; repeatability and batch independence bit for bit; ignored
edges; the operator and the shims against the C ABI; every RELPOSE_EINVAL path with pre-filled outputs; and the evaluation drivers built on
it.  Every test runs under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import sync_model as SM
import sync_scenes as SS
from gpu_util import log
from relativepose_amd import synth

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few at the most
INT_KEYS = ("component", "tree", "edge_state", "n_components")
FLOAT_KEYS = ("pose", "confidence", "res_rot", "res_trans", "cost", "last_step")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    import torch
    return torch.device("cuda:0")


def run(b, **kw):
    """util.pose_sync_dev on a batch of tests/sync_scenes.py -> host arrays"""
    from relativepose_amd import util
    out = util.pose_sync_dev(b["T"], b["src"], b["dst"], b["w0"], b["view_begin"], b["edge_begin"], device=dev(), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw(b, kw=None):
    """relpose_pose_sync through the C ABI into outputs pre-filled with SS.FILL -> (return code, host arrays)"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    V, E, S = int(b["view_begin"][-1]), int(b["edge_begin"][-1]), len(b["view_begin"]) - 1
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())
    ins = {"src": t(b["src"], np.int32), "dst": t(b["dst"], np.int32), "T": t(b["T"], np.float64), "w0": t(b["w0"], np.float64)}
    shapes = {"pose": (V, 4, 4), "confidence": (E,), "res_rot": (E,), "res_trans": (E,), "cost": (S,), "last_step": (S,), "component": (V,),
              "tree": (E,), "edge_state": (E,), "n_components": (S,)}
    out = {k: torch.full(shapes[k], SS.FILL["f"] if k in SS.OUT_F else SS.FILL["i"], dtype=torch.float64 if k in SS.OUT_F else torch.int32,
                         device=dev()) for k in shapes}
    nbytes = L.relpose_pose_sync_workspace(S, V, E)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev())
    ptrs = {k: v.data_ptr() for k, v in {**ins, **out}.items()}
    kw = dict(workspace=ws.data_ptr() + 8) if kw == "unaligned" else kw
    a = SS.sync_args(_lib, ptrs, b["view_begin"], b["edge_begin"], ws.data_ptr(), nbytes, kw)
    if a.stream is None:
        a.stream = _lib.stream_ptr()
    rc = L.relpose_pose_sync(C.byref(a))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def bitwise(a, b, keys=INT_KEYS + FLOAT_KEYS):
    return [k for k in keys if not SS.bits_equal(a[k], b[k])]


def check_against_model(name, got, want, bar):
    assert [k for k in ("component", "tree", "edge_state") if not SS.bits_equal(got[k], want[k])] == [], name
    diffs = {}
    for k in FLOAT_KEYS:
        g, w = np.asarray(got[k], np.float64).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, k)
        ok = ~np.isnan(w)
        diffs[k] = float(np.abs(g[ok] - w[ok]).max()) if ok.any() else 0.0
    log("pose_sync_" + name, bar=bar, **diffs)
    print(name, "largest difference to the model", diffs, "bar", bar)
    for k, d in diffs.items():
        assert d <= bar, (name, k, d, bar)


@pytest.mark.parametrize("name", SS.ALL)
def test_matches_the_model(name):
    got = run(SS.batch((name,)))
    want = SS.model(name)
    assert int(got["n_components"][0]) == want["n_components"]
    one = {k: (got[k][0] if k in ("cost", "last_step") else got[k]) for k in got}
    check_against_model(name, one, want, SS.bar(name))
    f = SS.fixture(name)
    rot, tr = SS.pose_errors(got["pose"], f["G"])
    log("pose_sync_gt_" + name, rot_deg=float(rot.max()), trans_m=float(tr.max()))
    if name in SS.OUTLIER:
        assert (got["confidence"][f["outlier"]] < 0.5).all() and (got["confidence"][~f["outlier"]] > 0.5).all()


def test_batch_with_a_scene_without_views_matches_the_model():
    names = ("k4", "empty", "chain5", "two_comp", "isolated", "m1", "m2")
    b = SS.batch(names)
    got = run(b)
    want = SM.sync(b["T"], b["src"], b["dst"], b["w0"], b["view_begin"], b["edge_begin"])
    assert got["n_components"].tolist() == want["n_components"].tolist() == [1, 0, 1, 2, 2, 1, 1]
    check_against_model("batch", got, want, max(SS.bar(n) for n in names if n != "empty"))


@pytest.mark.parametrize("name", ["k8_out_0", SS.BIG])
def test_repeatable_and_independent_of_the_batch(name):
    alone = run(SS.batch((name,)))
    assert bitwise(run(SS.batch((name,))), alone) == []
    f = SS.fixture(name)
    M, E = f["M"], len(f["src"])
    for names in ((name, "k4", "empty", "chain5", "k8_out_1"), ("k4", "empty", "chain5", "k8_out_1", name)):
        b = SS.batch(names)
        got = run(b)
        s = names.index(name)
        v0, e0 = int(b["view_begin"][s]), int(b["edge_begin"][s])
        part = {k: got[k][v0:v0 + M] if k in ("pose", "component") else (got[k][s:s + 1] if k in ("n_components", "cost", "last_step") else got[k][e0:e0 + E])
                for k in got}
        assert bitwise(part, alone) == [], names
        others = [n for n in names if n not in (name, "empty")]
        assert got["n_components"].tolist().count(0) == 1 and all(SS.model(n)["n_components"] == got["n_components"][names.index(n)] for n in others)


def test_ignored_edges_are_flagged_and_change_nothing_else():
    f = SS.fixture("k8_out_1")
    clean = run(SS.batch(("k8_out_1",)))
    E = len(f["src"])
    I = np.eye(4)
    nanT = I.copy()
    nanT[2, 3] = np.nan
    infT = I.copy()
    infT[0, 0] = np.inf
    bad = [(0, (8, 1, I, 1.0), SM.BAD_INDEX), (5, (2, -1, I, 1.0), SM.BAD_INDEX), (5, (3, 3, I, 1.0), SM.SELF_EDGE), (11, (1, 2, I, 0.0), SM.BAD_WEIGHT),
           (20, (1, 2, I, np.nan), SM.BAD_WEIGHT), (20, (4, 2, I, -1.0), SM.BAD_WEIGHT), (28, (0, 7, nanT, 1.0), SM.BAD_POSE),
           (28, (6, 7, infT, np.inf), SM.BAD_WEIGHT), (28, (9, 9, nanT, np.nan), SM.BAD_INDEX), (14, (5, 6, infT, 3.0), SM.BAD_POSE)]
    src, dst, T, w0, code, keep = [], [], [], [], [], []
    for e in range(E + 1):
        for at, (i, j, P, w), c in bad:
            if at == e:
                src.append(i); dst.append(j); T.append(P); w0.append(w); code.append(c); keep.append(False)
        if e < E:
            src.append(f["src"][e]); dst.append(f["dst"][e]); T.append(f["T"][e]); w0.append(f["w0"][e]); code.append(0); keep.append(True)
    keep, code = np.array(keep), np.array(code, np.int32)
    b = {"src": np.array(src, np.int32), "dst": np.array(dst, np.int32), "T": np.stack(T), "w0": np.array(w0), "view_begin": np.array([0, 8], np.int32),
         "edge_begin": np.array([0, len(src)], np.int32)}
    got = run(b)
    assert np.array_equal(got["edge_state"], code)
    assert (got["confidence"][~keep] == 0).all() and np.isnan(got["res_rot"][~keep]).all() and np.isnan(got["res_trans"][~keep]).all()
    assert (got["tree"][~keep] == 0).all()
    part = {k: (got[k][keep] if got[k].shape[0] == len(keep) else got[k]) for k in got}
    assert bitwise(part, clean) == []
    want = SM.sync_scene(8, b["src"], b["dst"], b["T"], b["w0"])
    assert np.array_equal(want["edge_state"], code) and np.array_equal(want["tree"], got["tree"]) and np.array_equal(want["component"], got["component"])
    # a graph of ignored edges alone: every view is its own component at the identity
    only = {k: (v[~keep] if k in ("src", "dst", "T", "w0") else v) for k, v in b.items()}
    only["edge_begin"] = np.array([0, int((~keep).sum())], np.int32)
    got = run(only)
    assert got["n_components"].tolist() == [8] and got["component"].tolist() == list(range(8)) and (got["pose"] == np.eye(4)).all()
    assert got["cost"].tolist() == [0.0] and np.array_equal(got["edge_state"], code[~keep])


def test_operator_and_shim_equal_the_c_abi():
    import torch
    from relativepose_amd import ops
    names = ("k8_out_2", "two_comp", "empty", "k4")
    b = SS.batch(names)
    rc, want = raw(b)
    assert rc == 0 and not any((want[k] == SS.FILL["f"]).any() for k in SS.OUT_F) and not any((want[k] == SS.FILL["i"]).any() for k in SS.OUT_I)
    assert bitwise(run(b), want) == []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    out = torch.ops.relpose.pose_sync(t(b["T"]), t(b["src"]), t(b["dst"]), t(b["w0"]), torch.from_numpy(b["view_begin"]), torch.from_numpy(b["edge_begin"]),
                                      int(b["view_begin"][-1]))
    assert bitwise({k: v.cpu().numpy() for k, v in zip(ops.POSE_SYNC_OUTPUTS, out)}, want) == []
    # the other schedule and the plain least squares, through both
    kw = dict(sigma_r=0.05, sigma_t=0.2, mu0=10.0, div=2.0, n_final=3)
    rc, want = raw(b, kw)
    assert rc == 0 and bitwise(run(b, **kw), want) == []
    rc, want = raw(b, dict(robust=0))
    assert rc == 0 and bitwise(run(b, robust=False), want) == [] and (want["confidence"] == 1.0).all()
    rc, none = raw(b, dict(mu0=1.0, n_final=0))                                 # no iteration: the spanning tree's poses
    assert rc == 0 and (none["last_step"] == 0).all() and (none["confidence"] == 1.0).all()
    assert bitwise(none, want, ("component", "tree", "edge_state", "n_components")) == []
    from relativepose_amd import evaluation as E
    f = SS.fixture("k8_out_2")
    sy = E.synchronize_scene(list(zip(f["src"].tolist(), f["dst"].tolist())), list(f["T"]), 8, device=dev())
    assert SS.bits_equal(sy["pose"], run(SS.batch(("k8_out_2",)))["pose"]) and (sy["pair_confidence"][f["outlier"]] < 0.5).all()


def test_invalid_arguments_leave_the_outputs_untouched():
    b, _ = SS.host_case()
    for name, kw in SS.einval_calls():
        rc, out = raw(b, "unaligned" if kw is None else kw)
        assert rc == -1 and SS.untouched(out), name
    import torch
    from relativepose_amd import _lib, util
    for kw in (dict(sigma_r=0.0), dict(div=1.0), dict(mu0=0.5), dict(n_final=-1)):
        with pytest.raises(ValueError):
            util.pose_sync_dev(b["T"], b["src"], b["dst"], b["w0"], b["view_begin"], b["edge_begin"], device=dev(), **kw)
    with pytest.raises(ValueError):
        util.pose_sync_dev(np.zeros((0, 4, 4)), [], [], [], [0, 65], [0, 0], device=dev())
    rc, out = raw(b)
    assert rc == 0 and not SS.untouched(out)


def test_synchronised_poses_rebuild_the_room():
    """synth.render_scene(7, 4, "suncg", 16): the six ground-truth relative poses with the first replaced by an outlier -> synchronize_scene ->
    fuse_views at voxel 0.25.  The surface's median distance to the walls stays within test_tsdf_cpu.py's pin for (suncg, 16) with the
    robust weights and leaves it without."""
    import torch
    from relativepose_amd import evaluation as E
    sc = synth.render_scene(7, 4, "suncg", 16)
    R = sc["R"]
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    T = [np.matmul(R[j], np.linalg.inv(R[i])) for i, j in pairs]
    T[0] = synth.random_rigid(np.random.RandomState(1))
    depth = torch.from_numpy(sc["depth"].astype(np.float32)).to(dev())
    pin = 0.05134 * 1.25
    med = {}
    for robust in (True, False):
        sy = E.synchronize_scene(pairs, T, 4, device=dev(), robust=robust)
        world = np.stack([np.matmul(sy["pose"][k], R[0]) for k in range(4)])      # the gauge is view 0's camera: back to the room's frame
        surf = E.fuse_views(depth, None, world, "suncg", 0.25)
        n = int(surf["n_points"][0])
        med[robust] = float(np.median(E.wall_error(surf["points"][0, :n].cpu().numpy(), sc["half"], 0.25)))
        rot, tr = E.absolute_pose_errors(sy["pose"], R, sy["component"])
        log("pose_sync_room", robust=robust, wall_median=med[robust], points=n, rot_deg=float(rot.max()), trans_m=float(tr.max()),
            confidence=sy["confidence"].tolist())
        print("robust", robust, "median wall error (voxels)", med[robust], "pin", pin, "pose errors", rot.max(), tr.max())
        if robust:
            assert sy["confidence"][0] < 0.5 and (sy["confidence"][1:] > 0.5).all()
    assert med[True] <= pin
    assert med[False] > pin


def test_evaluate_scenes_adds_its_fields_and_leaves_the_pair_records_alone():
    from relativepose_amd import evaluation as E
    sc = synth.render_scene(7, 4, "suncg", 16)
    recs = E.evaluate_scenes("fgs", [sc], dev(), dataset="suncg", fuse=0.25)
    assert len(recs) == 1
    r = recs[0]
    for k in ('scene', 'views', 'pairs', 'records', 'edges', 'n_components', 'component', 'pose', 'abs_err_rot', 'abs_err_t', 'abs_err_rot_median',
              'abs_err_rot_max', 'abs_err_t_median', 'abs_err_t_max', 'pair_confidence', 'downweighted_share', 'bad_share', 'bad_downweighted',
              'good_downweighted', 'cost', 'last_step', 'fuse_accuracy', 'fuse_completeness', 'fuse_points', 'fuse_views'):
        assert k in r, k
    assert r['views'] == 4 and r['pairs'] == 6 and r['pose'].shape == (4, 4, 4) and len(r['pair_confidence']) == len(r['records']) == r['edges']
    assert np.array_equal(r['pose'][0], np.eye(4)) and r['abs_err_rot'].shape == (4,) and 1 <= r['n_components'] <= 4
    # the pair records are evaluate_fgs' own on the same pairs
    ents = E.mine_pairs(sc["depth"], sc["R"], "suncg", "scene0", device=dev())
    ij = [(e['id_src'], e['id_tgt']) for e in ents]
    batch = {k: np.stack([sc[k][[i, j]] for i, j in ij]) for k in ("rgb", "norm", "depth", "R")}
    old = E.evaluate_fgs([batch], dev(), "suncg")
    assert len(old) == len(r['records'])
    for a, b in zip(r['records'], old):
        assert tuple(a) == tuple(b)
        for k in a:
            assert (a[k] == b[k]) if isinstance(a[k], str) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    s = E.scenes_summary(recs)
    assert s["pair_records"] == len(old) and "abs_err_rot_median" in s and "fuse_accuracy_median" in s
    log("pose_sync_scenes", records=len(old), rot=r['abs_err_rot'].tolist(), bad_share=r['bad_share'], downweighted=r['downweighted_share'],
        fuse_accuracy=r['fuse_accuracy'], fuse_completeness=r['fuse_completeness'])
