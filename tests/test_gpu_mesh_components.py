"""GPU: relpose_mesh_components and relpose_mesh_filter.  Every output is compared bit for bit with tests/components_model.py:
hand-built meshes with shuffled rows and vertex ids, the meshes relpose_tsdf_mesh extracts from mesh_scenes' volumes and from two disjoint
balls, truncated statistics, bad rows, a batch with an empty and a truncated scene; the filter's copies, map and untouched rows; repeats and
batch invariance; the operators and the Python layers against the C ABI; every RELPOSE_EINVAL path with pre-filled outputs.  Every test runs
under a time limit of its own: a watchdog ends the process if a GPU step hangs."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import components_model as CM
import components_scenes as CS
import mesh_model as MM
import mesh_scenes as MS
import tsdf_scenes as TS
from gpu_util import log
from relativepose_amd import synth

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                    # seconds per test; each takes a few
MAX_ROUNDS = 1024
LABEL_FILL, STAT_FILL = -77, 55


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    import torch
    return torch.device("cuda:0")


def up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def dev_mesh(m):
    return {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in m.items()}


def host_mesh(m):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in m.items()}


def components_raw(dm, cap_comp, max_rounds=MAX_ROUNDS, areas=True, stats=True, rc=0):
    """relpose_mesh_components through the C ABI into pre-filled outputs -> (the model's dict as numpy, rounds)"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, cap = dm["points"].shape[:2]
    cap_tri = dm["triangles"].shape[1]
    nbytes = L.relpose_mesh_components_workspace_bytes(S, cap, cap_tri)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    out = {"vertex_label": f((S, cap), LABEL_FILL, torch.int32), "tri_label": f((S, cap_tri), LABEL_FILL, torch.int32),
           "n_components": f((S,), LABEL_FILL, torch.int32), "bad_triangles": f((S,), LABEL_FILL, torch.int32)}
    if stats:
        out.update({k: f((S, cap_comp), STAT_FILL, torch.int64 if k == "comp_area" else torch.int32) for k in CM.STAT_KEYS})
    rounds = C.c_int(-1)
    a = _lib.MeshComponentsArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.max_rounds, a.area_scale = S, cap, cap_tri, cap_comp, max_rounds, dm["area_scale"]
    a.triangles, a.n_triangles, a.n_points = dm["triangles"].data_ptr(), dm["n_triangles"].data_ptr(), dm["n_points"].data_ptr()
    a.points = dm["points"].data_ptr() if areas else 0
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    a.rounds_host = C.addressof(rounds)
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_mesh_components(C.byref(a)) == rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, rounds.value


def filter_before(dm):
    import torch
    S, cap = dm["points"].shape[:2]
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    return {"points": f((S, cap, 3), -7.5, torch.float64), "normals": f((S, cap, 3), 9.25, torch.float64),
            "colors": None if dm["colors"] is None else f((S, cap, 3), -3.0, torch.float32), "valid": f((S, cap), 77, torch.uint8),
            "n_points": f((S,), -7, torch.int32), "triangles": f(tuple(dm["triangles"].shape), MS.TRI_FILL, torch.int32),
            "n_triangles": f((S,), -7, torch.int32), "vertex_map": f((S, cap), -5, torch.int32)}


def filter_raw(dm, comps, keep, drop_unused, with_map=True):
    """relpose_mesh_filter through the C ABI into pre-filled outputs -> (what it left as numpy, the fills as numpy)"""
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, cap = dm["points"].shape[:2]
    cap_tri = dm["triangles"].shape[1]
    nbytes = L.relpose_mesh_filter_workspace_bytes(S, cap, cap_tri)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    out = filter_before(dm)
    before = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    kp = up(np.ascontiguousarray(keep, dtype=np.uint8))
    vl, tl = up(comps["vertex_label"]), up(comps["tri_label"])
    a = _lib.MeshFilterArgs()
    a.struct_size = C.sizeof(a)
    a.n_scenes, a.cap, a.cap_tri, a.cap_comp, a.drop_unused = S, cap, cap_tri, kp.shape[1], drop_unused
    for k in ("points", "normals", "colors", "n_points", "triangles", "n_triangles"):
        setattr(a, k, 0 if dm[k] is None else dm[k].data_ptr())
        setattr(a, "out_" + k, 0 if out[k] is None else out[k].data_ptr())
    a.out_valid, a.vertex_map = out["valid"].data_ptr(), (out["vertex_map"].data_ptr() if with_map else 0)
    a.vertex_label, a.tri_label, a.keep = vl.data_ptr(), tl.data_ptr(), kp.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, _lib.stream_ptr()
    assert L.relpose_mesh_filter(C.byref(a)) == 0
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}, before


@pytest.mark.parametrize("name", CS.HAND)
def test_hand_built_meshes_match_the_model_bitwise(name):
    m = CS.hand(name)
    cap_comp, want = CS.expected("hand", name)
    dm = dev_mesh(m)
    got, rounds = components_raw(dm, cap_comp)
    bad = TS.differ(got, want, CM.KEYS)
    log("mesh_components_" + name, differ=bad, rounds=rounds, n_components=got["n_components"], bad_triangles=got["bad_triangles"])
    assert bad == [], (name, bad, got["n_components"], want["n_components"])
    assert 1 <= rounds <= MAX_ROUNDS
    again, _ = components_raw(dm, cap_comp)                                    # a second run
    assert TS.differ(again, got, CM.KEYS) == []
    if name == "batch":                                                        # a scene alone is the scene inside its batch
        assert got["n_components"][1] == 0 and (got["vertex_label"][1] == -1).all() and (got["tri_label"][1] == -1).all()
        assert m["n_triangles"][2] > m["triangles"].shape[1]
        for s in (0, 2):
            one, _ = components_raw(dev_mesh(CS.scene_of(m, s)), cap_comp)
            assert all(TS.bits_equal(one[k][0], got[k][s]) for k in CM.KEYS), s
    if name == "bad_rows":
        assert got["bad_triangles"][0] == 3 and (got["tri_label"][0, [4, 11, 23]] == -1).all()
    if name in ("bow_tie", "strip", "comb"):
        assert got["n_components"][0] == 1 and got["comp_root"][0, 0] == 0
    if name == "two_triangles":
        assert got["n_components"][0] == 2


def test_statistics_truncate_at_cap_comp_and_the_count_stays_true():
    m = CS.hand("random")
    dm = dev_mesh(m)
    full_cap, full = CS.expected("hand", "random")
    n = int(full["n_components"][0])
    assert n > 3
    _, want = CS.expected("hand", "random", 3)
    got, _ = components_raw(dm, 3)
    assert TS.differ(got, want, CM.KEYS) == [] and got["n_components"][0] == n
    assert all(TS.bits_equal(got[k][0], full[k][0, :3]) for k in CM.STAT_KEYS)
    count, _ = components_raw(dm, 0, stats=False)                              # the counting call: no statistics at all
    assert TS.differ(count, full, CM.LABEL_KEYS) == []
    no_area, _ = components_raw(dm, full_cap, areas=False)                     # without points: the areas are 0
    assert TS.differ(no_area, CM.components(m, full_cap, m["area_scale"], areas=False), CM.KEYS) == [] and (no_area["comp_area"] == 0).all()


def test_round_guard_returns_its_own_code():
    from relativepose_amd import _lib, util
    dm = dev_mesh(CS.hand("strip"))
    _, rounds = components_raw(dm, 4, max_rounds=1, rc=_lib.MESH_EROUNDS)
    assert rounds == 1
    with pytest.raises(RuntimeError):
        util.mesh_components_dev(dm, dm["area_scale"], 4, max_rounds=1)


def volume_device_mesh(name):
    """relpose_tsdf_mesh's mesh of a volume case on the device (as test_gpu_mesh.device_state builds the state), with its area_scale"""
    from relativepose_amd import util
    c = CS.volume_case(name)
    ts = c["tsdf_sum"]
    S, nz, ny, nx = ts.shape
    st = {"tsdf_sum": up(ts.astype(np.int32)), "weight": up(c["weight"].astype(np.int32)),
          "color_sum": None if c["color_sum"] is None else up(c["color_sum"].view(np.int32)),
          "origin": np.ascontiguousarray(c["origin"], dtype=np.float64), "dims": (nx, ny, nz), "voxel": c["voxel"]}
    dm = util.tsdf_mesh_dev(st, c["min_weight"])
    dm["area_scale"] = float(2 ** 20) / c["voxel"] ** 2
    dm["voxel"] = c["voxel"]
    return dm


@pytest.mark.parametrize("name", CS.VOLUMES)
def test_meshes_of_volumes_match_the_model_bitwise(name):
    from relativepose_amd import util
    dm = volume_device_mesh(name)
    hm = host_mesh(dm)
    ref = CS.volume_mesh(name)                                                 # the extracted mesh is the model's mesh
    for s in range(len(hm["n_points"])):
        n, nt = int(ref["n_points"][s]), int(ref["n_triangles"][s])
        assert hm["n_points"][s] == n and hm["n_triangles"][s] == nt
        assert TS.bits_equal(hm["points"][s, :n], ref["points"][s, :n]) and TS.bits_equal(hm["triangles"][s, :nt], ref["triangles"][s, :nt])
    cap_comp = int(CM.components(hm, 0, hm["area_scale"])["n_components"].max()) + 2
    want = CM.components(hm, cap_comp, hm["area_scale"])
    got, rounds = components_raw(dm, cap_comp)
    bad = TS.differ(got, want, CM.KEYS)
    log("mesh_components_volume_" + name, differ=bad, rounds=rounds, n_components=got["n_components"], largest=got["comp_triangles"].max(1))
    assert bad == [], (name, bad)
    shim = util.mesh_components_dev(dm)                                        # None: sized by a counting call; area_scale from the voxel
    assert shim["comp_root"].shape[1] == max(1, cap_comp - 2) and shim["area_scale"] == hm["area_scale"]
    for k in CM.KEYS:
        w = want[k] if k in CM.LABEL_KEYS else want[k][:, :shim[k].shape[1]]
        assert TS.bits_equal(shim[k].cpu().numpy(), w), k
    if name == "empty_in_batch":
        for s in (0, 2):
            one, _ = components_raw(dev_mesh(CS.scene_of(hm, s)), cap_comp)
            assert all(TS.bits_equal(one[k][0], got[k][s]) for k in CM.KEYS), s


def closed_surface(mesh):
    from relativepose_amd import evaluation as E
    hm = host_mesh(mesh)
    V, F = int(hm["n_points"][0]), int(hm["n_triangles"][0])
    st = E.mesh_stats(hm)[0]
    edges = np.unique(np.sort(MM.directed_edges(hm["triangles"][0, :F]), 1), axis=0)
    return st["border_edges"] == 0 and st["nonmanifold_edges"] == 0 and V - len(edges) + F == 2 and F > 0


def test_two_balls_clean_to_one_closed_surface():
    from relativepose_amd import util
    dm = volume_device_mesh("two_balls")
    comps = util.mesh_components_dev(dm)
    ct = comps["comp_triangles"][0].tolist()
    assert int(comps["n_components"][0]) == 2 and ct[0] > ct[1] > 0
    assert not closed_surface(dm)                                              # the pair is two closed surfaces: V - E + F = 4
    big, c1 = util.mesh_clean_dev(dm, largest=1)
    assert closed_surface(big) and int(big["n_triangles"][0]) == ct[0] and c1["keep"][0].tolist() == [True, False]
    same, _ = util.mesh_clean_dev(dm, min_triangles=ct[1] + 1)
    assert closed_surface(same) and all(TS.bits_equal(same[k].cpu().numpy(), big[k].cpu().numpy()) for k in CM.FILTER_KEYS if big[k] is not None)
    small, _ = util.mesh_clean_dev(dm, min_area=0.0, largest=2)                # both stay
    assert int(small["n_triangles"][0]) == ct[0] + ct[1]
    log("mesh_components_two_balls", triangles=ct, rounds=comps["rounds"])


FILTER_CASES = [("hand", "random"), ("hand", "batch"), ("hand", "bad_rows"), ("hand", "comb"), ("volume", "noise"), ("volume", "empty_in_batch")]


@pytest.mark.parametrize("kind,name", FILTER_CASES)
def test_filter_copies_survivors_bitwise_and_leaves_the_rest(kind, name):
    m = CS.hand(name) if kind == "hand" else CS.volume_mesh(name)
    cap_comp, comps = CS.expected(kind, name)
    dm = dev_mesh(m)
    S = m["points"].shape[0]
    keeps = {"some": (comps["comp_triangles"] >= 2) & (np.arange(cap_comp)[None] % 3 != 1), "all": np.ones((S, cap_comp), bool),
             "none": np.zeros((S, cap_comp), bool)}
    for label, keep in keeps.items():
        for drop in (1, 0):
            got, before = filter_raw(dm, comps, keep, drop)
            want = CM.filter_outputs(m, comps, keep, drop, before)
            assert TS.differ(got, want, CM.FILTER_KEYS) == [], (name, label, drop, TS.differ(got, want, CM.FILTER_KEYS))
            for s in range(S):                                                 # survivors are source rows; rows beyond the counts keep their fill
                n = int(got["n_points"][s])
                src = np.nonzero(got["vertex_map"][s] >= 0)[0]
                assert len(src) == n and np.array_equal(got["vertex_map"][s, src], np.arange(n))
                assert all(TS.bits_equal(got[k][s, :n], m[k][s, src]) for k in ("points", "normals", "colors") if m[k] is not None)
                assert all(TS.bits_equal(got[k][s, n:], before[k][s, n:]) for k in ("points", "normals", "colors") if m[k] is not None)
                assert TS.bits_equal(got["triangles"][s, int(got["n_triangles"][s]):], before["triangles"][s, int(got["n_triangles"][s]):])
    got, before = filter_raw(dm, comps, keeps["some"], 1)
    again, _ = filter_raw(dm, comps, keeps["some"], 1)                        # a second run; and without the optional map
    no_map, _ = filter_raw(dm, comps, keeps["some"], 1, with_map=False)
    assert TS.differ(again, got, CM.FILTER_KEYS) == []
    assert TS.differ(no_map, got, CM.FILTER_KEYS[:-1]) == [] and TS.bits_equal(no_map["vertex_map"], before["vertex_map"])
    if S > 1:                                                                  # a scene alone is the scene inside its batch
        for s in range(S):
            one, _ = filter_raw(dev_mesh(CS.scene_of(m, s)), {k: v[s:s + 1] for k, v in comps.items()}, keeps["some"][s:s + 1], 1)
            assert all(TS.bits_equal(one[k][0], got[k][s]) for k in CM.FILTER_KEYS if got[k] is not None), s


def test_operators_and_python_layers_give_what_the_c_abi_wrote():
    import torch
    from relativepose_amd import evaluation as E, ops, util  # noqa: F401
    m = CS.hand("batch")
    dm = dev_mesh(m)
    cap_comp, want = CS.expected("hand", "batch")
    raw, rounds = components_raw(dm, cap_comp)
    with pytest.raises(ValueError):                                            # a truncated scene needs truncated=True
        util.mesh_components_dev(dm, m["area_scale"], cap_comp)
    shim = util.mesh_components_dev(dm, m["area_scale"], cap_comp, truncated=True)
    op = torch.ops.relpose.mesh_components(dm["points"], dm["n_points"], dm["triangles"], dm["n_triangles"], m["area_scale"], cap_comp, 1024, True)
    assert set(shim) == set(CM.KEYS) | {"rounds", "area_scale"} and 1 <= shim["rounds"] <= MAX_ROUNDS and 1 <= int(op[8][0]) <= MAX_ROUNDS
    for got in ({k: shim[k].cpu().numpy() for k in CM.KEYS}, {k: v.cpu().numpy() for k, v in zip(CM.KEYS, op)}):
        assert TS.differ(got, raw, CM.KEYS) == [] and TS.differ(got, want, CM.KEYS) == []
    mm = torch.ops.relpose.mesh_components(dm["points"].to("meta"), dm["n_points"].to("meta"), dm["triangles"].to("meta"), dm["n_triangles"].to("meta"),
                                           m["area_scale"], cap_comp, 1024, True)
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(mm, op))
    # the filter: the shim and the operator pre-fill with zeros
    keep = (want["comp_triangles"] >= 2)
    zero = {k: (None if v is None else np.zeros_like(v)) for k, v in filter_raw(dm, want, keep, 1)[1].items()}
    model = CM.filter_outputs(m, want, keep, 1, zero)
    fs = util.mesh_filter_dev(dm, shim, up(keep), True, truncated=True)
    fo = torch.ops.relpose.mesh_filter(dm["points"], dm["normals"], dm["colors"], dm["n_points"], dm["triangles"], dm["n_triangles"],
                                       shim["vertex_label"], shim["tri_label"], up(keep.astype(np.uint8)), True, True)
    assert set(fs) == set(CM.FILTER_KEYS)
    for got in ({k: fs[k].cpu().numpy() for k in CM.FILTER_KEYS}, {k: v.cpu().numpy() for k, v in zip(CM.FILTER_KEYS, fo)}):
        assert TS.differ(got, model, CM.FILTER_KEYS) == []
    fm = torch.ops.relpose.mesh_filter(*(t.to("meta") for t in (dm["points"], dm["normals"], dm["colors"], dm["n_points"], dm["triangles"], dm["n_triangles"],
                                                                 shim["vertex_label"], shim["tri_label"], up(keep.astype(np.uint8)))), True, True)
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(fm, fo))
    # mesh_clean_dev's selection against numpy: the criteria ANDed, largest by triangles with ties to the lower id
    full = util.mesh_components_dev(dm, m["area_scale"], None, truncated=True)
    ct, ca, n = (full[k].cpu().numpy() for k in ("comp_triangles", "comp_area", "n_components"))
    exists = np.arange(ct.shape[1])[None] < n[:, None]
    for kw in ({"min_triangles": 3}, {"min_area": 0.5}, {"largest": 2}, {"min_triangles": 2, "largest": 3}, {}):
        k = exists.copy()
        if "min_triangles" in kw:
            k &= ct >= kw["min_triangles"]
        if "min_area" in kw:
            k &= ca.astype(np.float64) >= kw["min_area"] * m["area_scale"]
        if "largest" in kw:
            top = np.zeros_like(k)
            for s in range(len(n)):
                order = sorted(np.nonzero(k[s])[0], key=lambda c: (-ct[s, c], c))[:kw["largest"]]
                top[s, order] = True
            k &= top
        clean, comps = util.mesh_clean_dev(dm, truncated=True, area_scale=m["area_scale"], **kw)
        assert np.array_equal(comps["keep"].cpu().numpy(), k), kw
        w = CM.filter_outputs(m, {a: full[a].cpu().numpy() for a in ("vertex_label", "tri_label")}, k, 1, zero)
        assert TS.differ({a: clean[a].cpu().numpy() for a in CM.FILTER_KEYS}, w, CM.FILTER_KEYS) == [], kw
    st = E.mesh_component_stats(full)
    assert [s["components"] for s in st] == n.tolist() and st[1]["small_triangles"] == 0


def test_every_einval_returns_before_the_outputs_are_touched():
    import torch
    from relativepose_amd import _lib
    L = _lib.lib()
    S, cap, cap_tri, cap_comp = 2, 8, 6, 4
    f = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev())
    tri = torch.tensor([[0, 1, 2], [2, 3, 4], [5, 6, 7], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.int32, device=dev()).repeat(S, 1, 1).contiguous()
    src = {"triangles": tri, "n_triangles": f((S,), 3, torch.int32), "n_points": f((S,), 8, torch.int32),
           "points": torch.arange(S * cap * 3, dtype=torch.float64, device=dev()).reshape(S, cap, 3) ** 2, "normals": f((S, cap, 3), 0.5, torch.float64),
           "colors": f((S, cap, 3), 0.25, torch.float32), "keep": f((S, cap_comp), 1, torch.uint8)}
    out = {"vertex_label": f((S, cap), LABEL_FILL, torch.int32), "tri_label": f((S, cap_tri), LABEL_FILL, torch.int32),
           "n_components": f((S,), LABEL_FILL, torch.int32), "bad_triangles": f((S,), LABEL_FILL, torch.int32)}
    out.update({k: f((S, cap_comp), STAT_FILL, torch.int64 if k == "comp_area" else torch.int32) for k in CM.STAT_KEYS})
    fout = {"out_" + k if k != "vertex_map" else k: v for k, v in filter_before({"points": src["points"], "colors": src["colors"], "triangles": tri}).items()}
    before = {k: v.clone() for k, v in {**out, **fout}.items()}
    ws = torch.empty(max(L.relpose_mesh_components_workspace_bytes(S, cap, cap_tri), L.relpose_mesh_filter_workspace_bytes(S, cap, cap_tri)) + 512,
                     dtype=torch.uint8, device=dev())
    rounds = C.c_int(-9)
    cptrs = {k: {**src, **out}[k].data_ptr() for k in CS.COMPONENT_POINTERS}
    for name, kw in CS.components_einval_calls():
        a = CS.components_args(_lib, cptrs, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, rounds_host=C.addressof(rounds))
        a.stream = _lib.stream_ptr()
        assert L.relpose_mesh_components(C.byref(a)) == -1, name
    fptrs = {k: {**src, **out, **fout}[k].data_ptr() for k in CS.FILTER_POINTERS}
    for name, kw in CS.filter_einval_calls():
        a = CS.filter_args(_lib, fptrs, kw, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256)
        a.stream = _lib.stream_ptr()
        assert L.relpose_mesh_filter(C.byref(a)) == -1, name
    torch.cuda.synchronize()
    assert all(torch.equal({**out, **fout}[k], before[k]) for k in before) and rounds.value == -9
    a = CS.components_args(_lib, cptrs, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256, rounds_host=C.addressof(rounds))
    a.stream = _lib.stream_ptr()
    assert L.relpose_mesh_components(C.byref(a)) == 0                          # the base calls themselves are valid
    assert out["n_components"].tolist() == [2, 2] and out["comp_triangles"][0].tolist() == [2, 1, 0, 0] and 1 <= rounds.value <= 16
    assert out["comp_root"][1].tolist() == [0, 5, -1, -1] and out["comp_vertices"][1].tolist() == [5, 3, 0, 0]
    a = CS.filter_args(_lib, fptrs, {}, ws=ws.data_ptr(), ws_bytes=ws.numel() - 256)
    a.stream = _lib.stream_ptr()
    assert L.relpose_mesh_filter(C.byref(a)) == 0
    torch.cuda.synchronize()
    assert fout["out_n_points"].tolist() == [8, 8] and fout["out_n_triangles"].tolist() == [3, 3] and torch.equal(fout["out_triangles"][:, :3], tri[:, :3])


def test_fuse_views_cleans_only_when_asked():
    """synth.render_scene(7, 4, "suncg", 16) fused at voxel 0.25 (test_gpu_mesh.py's room): without min_component fuse_views(mesh=True) is
    what it was -- util.tsdf_mesh_dev of its state, with the keys it had; with it, the model's filter of that mesh."""
    from relativepose_amd import evaluation as E, util
    sc = synth.render_scene(7, 4, "suncg", 16)
    depth, rgb = up(sc["depth"].astype(np.float32)), up(sc["rgb"].astype(np.float32))
    mesh = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True)
    assert set(mesh) == set(MS.MESH_KEYS) | {"origin", "dims", "voxel", "state"}
    direct = util.tsdf_mesh_dev(mesh["state"], 1)
    assert all(TS.bits_equal(mesh[k].cpu().numpy(), direct[k].cpu().numpy()) for k in MS.MESH_KEYS)
    nt = int(mesh["n_triangles"][0])
    host = {k: mesh["state"][k][0].cpu().numpy() for k in ("tsdf_sum", "weight")}
    assert TS.bits_equal(mesh["triangles"][0, :nt].cpu().numpy(), MM.triangles(host["tsdf_sum"], host["weight"], 1)[0])
    hm = host_mesh({k: mesh[k] for k in MS.MESH_KEYS})
    scale = float(2 ** 20) / 0.25 ** 2
    n = int(CM.components(hm, 0, scale)["n_components"][0])
    want = CM.components(hm, max(n, 1), scale)
    N = int(want["comp_triangles"][0].max())                                   # keeps the largest component(s) only
    clean = E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, mesh=True, min_component=N)
    comps = clean["components"]
    assert TS.differ({k: comps[k].cpu().numpy() for k in CM.KEYS}, want, CM.KEYS) == []
    zero = {k: (None if hm.get(k) is None else np.zeros_like(hm[k])) for k in MS.MESH_KEYS}
    zero["vertex_map"] = np.zeros(hm["points"].shape[:2], np.int32)
    model = CM.filter_outputs(hm, want, want["comp_triangles"] >= N, 1, zero)
    assert TS.differ({k: clean[k].cpu().numpy() for k in CM.FILTER_KEYS}, model, CM.FILTER_KEYS) == []
    st = E.mesh_component_stats(comps)[0]
    log("mesh_components_room", rounds=comps["rounds"], removed=nt - int(clean["n_triangles"][0]), **st)
    assert st["components"] == n and int(clean["n_triangles"][0]) == nt - st["small_triangles"]
    with pytest.raises(ValueError):
        E.fuse_views(depth, rgb, sc["R"], "suncg", 0.25, min_component=5)
