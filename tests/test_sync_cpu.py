"""CPU: the pose synchronisation contract's numpy model (tests/sync_model.py) agrees with its own plain-loop statement bit for bit, returns
ground truth on exact graphs, recovers every view of the pinned graphs with a quarter of their edges replaced by outliers (and does not
without the robust weights), its sensitivity to one-ulp changes of the input is what tests/sync_scenes.py pins, and the host layers
around relpose_pose_sync -- header, exports, operator registration, workspace query, argument validation, util.pose_graph -- work without
a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import sync_model as SM
import sync_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured with the model on k8_out_<seed> (8 views, 28 edges, 7 of them outliers; DESIGN.md 4.17 holds the same numbers): the largest
# rotation error in degrees and translation error in metres over the views.  The pins are the measured values x 1.25.
MEASURED = {"k8_out_0": (0.0003352, 6.431e-06), "k8_out_1": (0.0002365, 3.655e-06), "k8_out_2": (0.0001135, 5.633e-06)}


def same(a, b):
    return [k for k in SM.KEYS if not SS.bits_equal(np.asarray(a[k], dtype=np.asarray(b[k]).dtype), np.asarray(b[k]))]


@pytest.mark.parametrize("name", SS.EXACT + SS.OUTLIER[:1])
@pytest.mark.parametrize("robust", [True, False])
def test_loops_equal_the_vectorised_form(name, robust):
    f = SS.fixture(name)
    a = SS.model(name, robust)
    b = SM.sync_scene_loops(f["M"], f["src"], f["dst"], f["T"], f["w0"], robust=robust)
    assert same(a, b) == []


def test_loops_equal_the_vectorised_form_with_ignored_edges_and_another_schedule():
    f = SS.fixture("k8_out_1")
    src, dst, T, w0 = f["src"].copy(), f["dst"].copy(), f["T"].copy(), f["w0"].copy()
    src[3], dst[5], w0[7], w0[9], w0[11] = 8, dst[5] * 0 + src[5], 0.0, np.nan, -1.0
    T[13, 1, 2] = np.nan
    kw = dict(sigma_r=0.05, sigma_t=0.2, mu0=10.0, div=2.0, n_final=3)
    a, b = SM.sync_scene(8, src, dst, T, w0, **kw), SM.sync_scene_loops(8, src, dst, T, w0, **kw)
    assert same(a, b) == []
    assert a["edge_state"][[3, 5, 7, 9, 11, 13]].tolist() == [SM.BAD_INDEX, SM.SELF_EDGE, SM.BAD_WEIGHT, SM.BAD_WEIGHT, SM.BAD_WEIGHT, SM.BAD_POSE]
    assert SM.schedule(10.0, 2.0, 3) == [10.0, 5.0, 2.5, 1.25, 1.0, 1.0, 1.0] and len(SM.schedule()) == 13 + 10


@pytest.mark.parametrize("name", SS.EXACT)
def test_exact_graphs_return_ground_truth(name):
    f, m = SS.fixture(name), SS.model(name)
    assert np.array_equal(m["component"], f["component"]) and m["n_components"] == len(set(f["component"].tolist()))
    assert m["tree"].sum() == f["M"] - m["n_components"]
    rot, tr = SS.pose_errors(m["pose"], f["G"])
    print(name, "rotation error (deg), translation error (m)", rot.max(), tr.max())
    assert rot.max() < 1e-12 and tr.max() < 1e-13                      # a few ulps of poses whose translations are at most 2 m apart
    assert (m["confidence"] > 1 - 1e-12).all() and (m["res_rot"] < 1e-14).all() and (m["res_trans"] < 1e-14).all()
    assert m["cost"] < 1e-24 and m["last_step"] < 1e-15
    for v in np.nonzero(f["component"] == np.arange(f["M"]))[0]:
        assert np.array_equal(m["pose"][v], np.eye(4))                 # the gauge, the isolated view included


def test_scene_without_views_in_the_middle_of_a_batch():
    b = SS.batch(("k4", "empty", "chain5"))
    assert b["view_begin"].tolist() == [0, 4, 4, 9] and b["edge_begin"].tolist() == [0, 6, 6, 10]
    out = SM.sync(b["T"], b["src"], b["dst"], b["w0"], b["view_begin"], b["edge_begin"])
    assert out["n_components"].tolist() == [1, 0, 1] and out["cost"][1] == 0.0 and out["last_step"][1] == 0.0
    assert SS.bits_equal(out["pose"][:4], SS.model("k4")["pose"]) and SS.bits_equal(out["pose"][4:], SS.model("chain5")["pose"])
    rot, tr = SS.pose_errors(out["pose"], b["G"])
    assert rot.max() < 1e-12 and tr.max() < 1e-13


@pytest.mark.parametrize("name", SS.OUTLIER)
def test_outliers_are_rejected_and_every_view_recovered(name):
    f, m = SS.fixture(name), SS.model(name)
    assert f["M"] == 8 and len(f["src"]) == 28 and f["outlier"].sum() == 7
    rot, tr = SS.pose_errors(m["pose"], f["G"])
    print(name, "robust: rotation error (deg), translation error (m)", rot.max(), tr.max())
    assert rot.max() <= 1.25 * MEASURED[name][0] and tr.max() <= 1.25 * MEASURED[name][1]
    assert rot.max() >= 0.75 * MEASURED[name][0] and tr.max() >= 0.75 * MEASURED[name][1]      # the table is still what the model gives
    assert (m["confidence"][f["outlier"]] < 0.5).all() and (m["confidence"][~f["outlier"]] > 0.5).all()
    assert m["last_step"] < 1e-12 and m["n_components"] == 1
    plain = SS.model(name, False)
    prot, ptr = SS.pose_errors(plain["pose"], f["G"])
    print(name, "plain least squares: rotation error (deg), translation error (m)", prot.max(), ptr.max())
    assert prot.max() > 1.0 and (plain["confidence"] == 1.0).all()


@pytest.mark.parametrize("name", SS.ALL)
def test_sensitivity(name):
    got = SS.sensitivity(name)
    print(name, "largest change of a pose entry under one-ulp input noise", got, "pinned", SS.SENS[name])
    assert 0.5 * SS.SENS[name] <= got <= 2.0 * SS.SENS[name]
    assert SS.bar(name) == max(1000 * SS.SENS[name], 1e-12)


def test_big_graph_reaches_the_limits():
    f, m = SS.fixture(SS.BIG), SS.model(SS.BIG)
    assert f["M"] == SM.MAX_VIEWS and len(f["src"]) == SM.MAX_EDGES and m["tree"].sum() == 63 and m["n_components"] == 1
    assert len({(int(a), int(b)) for a, b in zip(f["src"], f["dst"])}) < 4096         # duplicates
    rot, tr = SS.pose_errors(m["pose"], f["G"])
    assert rot.max() < 1e-11 and tr.max() < 1e-12


# ------------------------------------------------------------------------------------------------------------- host layers
def test_header_declares_the_symbols_and_the_library_exports_them():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    for sym in ("relpose_pose_sync_workspace", "relpose_pose_sync", "RelposePoseSyncArgs", "RELPOSE_SYNC_MAX_VIEWS = 64", "RELPOSE_SYNC_MAX_EDGES = 4096",
                "RELPOSE_SYNC_BAD_INDEX = 1", "RELPOSE_SYNC_SELF_EDGE = 2", "RELPOSE_SYNC_BAD_WEIGHT = 3", "RELPOSE_SYNC_BAD_POSE = 4"):
        assert sym in h, sym
    from relativepose_amd import _lib, build
    assert "relpose_pose_sync" in _lib.SIGNATURES and "relpose_pose_sync_workspace" in _lib.SIGNATURES
    assert (_lib.SYNC_MAX_VIEWS, _lib.SYNC_MAX_EDGES) == (SM.MAX_VIEWS, SM.MAX_EDGES)
    assert any(s == "posesync.hip" and "-ffp-contract=off" in fl for s, fl in build.SOURCES)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    assert hasattr(lib, "relpose_pose_sync") and hasattr(lib, "relpose_pose_sync_workspace")


def test_struct_layout_matches_the_header(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    from relativepose_amd import _lib
    fields = [n for n, _ in _lib.PoseSyncArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu\\n", offsetof(RelposePoseSyncArgs, {n}));\n' for n in fields)
                   + '    printf("%zu\\n", sizeof(RelposePoseSyncArgs));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.PoseSyncArgs, n).offset for n in fields] + [C.sizeof(_lib.PoseSyncArgs)]


def test_operator_is_registered_with_its_meta_function():
    import torch
    from relativepose_amd import ops
    assert "pose_sync" in ops.OPS
    m = lambda *s, dt: torch.empty(*s, dtype=dt, device="meta")
    out = torch.ops.relpose.pose_sync(m(10, 4, 4, dt=torch.float64), m(10, dt=torch.int32), m(10, dt=torch.int32), m(10, dt=torch.float64),
                                      m(3, dt=torch.int32), m(3, dt=torch.int32), 9)
    assert len(out) == len(ops.POSE_SYNC_OUTPUTS) == 10
    shapes = {"pose": (9, 4, 4), "component": (9,), "tree": (10,), "edge_state": (10,), "confidence": (10,), "res_rot": (10,), "res_trans": (10,),
              "n_components": (2,), "cost": (2,), "last_step": (2,)}
    for k, t in zip(ops.POSE_SYNC_OUTPUTS, out):
        assert tuple(t.shape) == shapes[k], k
        assert t.dtype == (torch.int32 if k in ("component", "tree", "edge_state", "n_components") else torch.float64), k
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.pose_sync(torch.eye(4, dtype=torch.float64)[None], torch.tensor([0]), torch.tensor([1]), torch.ones(1, dtype=torch.float64),
                                    torch.tensor([0, 2]), torch.tensor([0, 1]), 2)


def test_invalid_arguments_are_rejected_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1
    assert lib.relpose_pose_sync(None) == EINVAL
    W = lib.relpose_pose_sync_workspace
    assert W(2, 9, 10) >= 2 * 3 * 4 + 10 * (8 + 24 + 8) and W(2, 9, 10) % 256 == 0
    assert W(1, 64, 4096) > 0 and W(3, 0, 0) > 0 and W(2, 128, 8192) > 0
    for a in ((0, 0, 0), (-1, 4, 4), (1, 65, 0), (1, 4, 4097), (2, 129, 0), (2, 0, 8193), (1, -1, 0), (1, 0, -1), (1 << 24, 0, 0)):
        assert W(*a) == 0, a
    b, out = SS.host_case()                          # host memory: a valid call would fault, an invalid one must not touch it
    ws = (C.c_double * 64)()
    wsp = (C.addressof(ws) + 255) & ~255
    ptrs = {k: b[k].ctypes.data for k in ("src", "dst", "T", "w0")}
    ptrs.update({k: v.ctypes.data for k, v in out.items()})
    calls = SS.einval_calls()
    assert len(calls) >= 45 and len({n for n, _ in calls}) == len(calls)
    for name, kw in calls:
        kw = dict(workspace=wsp + 8) if kw is None else kw
        a = SS.sync_args(_lib, ptrs, b["view_begin"], b["edge_begin"], wsp, 1 << 20, kw)
        assert lib.relpose_pose_sync(C.byref(a)) == EINVAL, name
    assert SS.untouched(out) and ws[:] == [0.0] * 64


def test_pose_graph_host_logic():
    from relativepose_amd import util
    I = np.eye(4)
    A, B = I.copy(), I.copy()
    A[0, 3], B[1, 3] = 1.0, 2.0
    src, dst, T, w0, pair = util.pose_graph([(0, 1), (2, 1), (0, 2)], [A, np.stack([A, B, I]), B], [0.5, [1.0, 2.0, 3.0], None])
    assert src.tolist() == [0, 2, 2, 2, 0] and dst.tolist() == [1, 1, 1, 1, 2] and pair.tolist() == [0, 1, 1, 1, 2]
    assert w0.tolist() == [0.5, 1.0, 2.0, 3.0, 1.0] and np.array_equal(T, np.stack([A, A, B, I, B]))
    assert src.dtype == dst.dtype == pair.dtype == np.int32 and T.dtype == w0.dtype == np.float64 and T.shape == (5, 4, 4)
    recs = [{"src": 1, "dst": 0, "pose": A, "vis_agreement": 0.25}, {"src": 0, "dst": 2, "poses": np.stack([A, B])},
            {"src": 2, "dst": 1, "pose": B, "vis_agreement": float("nan")}, {"src": 2, "dst": 0, "pose": B, "vis_agreement": 0.0}]
    src, dst, T, w0, pair = util.pose_graph(recs, None)
    assert src.tolist() == [1, 0, 0, 2, 2] and dst.tolist() == [0, 2, 2, 1, 0] and pair.tolist() == [0, 1, 1, 2, 3]
    assert w0.tolist() == [0.25, 1.0, 1.0, 1.0, 1.0]                        # no agreement, or none usable: 1
    src, dst, T, w0, pair = util.pose_graph([], [])
    assert src.shape == dst.shape == w0.shape == pair.shape == (0,) and T.shape == (0, 4, 4)
    with pytest.raises(ValueError):
        util.pose_graph([(0, 1)], [A, B])
    with pytest.raises(ValueError):
        util.pose_graph([(0, 1)], [A], [1.0, 2.0])


def test_absolute_pose_errors_and_the_cli_flag():
    from relativepose_amd import evaluation as E
    from relativepose_amd import synth
    rs = np.random.RandomState(2)
    R = np.stack([synth.random_rigid(rs) for _ in range(5)])
    comp = np.array([0, 1, 0, 1, 0])
    hat = np.stack([np.matmul(R[k], np.linalg.inv(R[comp[k]])) for k in range(5)])
    rot, tr = E.absolute_pose_errors(hat, R, comp)
    assert rot.max() < 1e-5 and tr.max() < 1e-12
    off = synth.random_rigid(np.random.RandomState(3), 0.3, 0.5)
    hat[2] = np.matmul(off, hat[2])
    rot, tr = E.absolute_pose_errors(hat, R, comp)
    want = np.degrees(np.arccos((np.trace(off[:3, :3]) - 1) / 2))
    assert abs(rot[2] - want) < 1e-6 and rot[[0, 1, 3, 4]].max() < 1e-5 and tr[2] > 0.01
    assert E._cli_parser_completion().parse_args([]).reconstruct is False
    assert E._cli_parser_completion().parse_args(["--reconstruct", "--method", "fgs", "--scenes", "2", "--scene-views", "4"]).reconstruct is True
    for argv in (["--reconstruct", "--mine-pairs"], ["--reconstruct", "--gpus", "2"], ["--reconstruct", "--scene-views", "65"],
                 ["--reconstruct", "--scene-views", "1"], ["--reconstruct", "--descriptor-eval"], ["--reconstruct", "--method", "fgs"],
                 ["--reconstruct", "--keypoint-mode", "reference"]):
        with pytest.raises(SystemExit):
            E.main(argv)
