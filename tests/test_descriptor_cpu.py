"""CPU: the descriptor-evaluation contract's numpy model (tests/descriptor_model.py) against scipy, float64 and the
reference's torch expression, and the C ABI / plumbing of relpose_dense_nn and relpose_descriptor_rank."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import descriptor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clouds(n, seed, ds, h):
    """(pc [2n,3,P], valid [2n,P], to_world [2n,4,4]) of synth.make_pairs through the oracle's pano2pc (suncg / matterport: every point valid)."""
    from oracle import geom_oracle as G
    from relativepose_amd import synth
    d = synth.make_pairs(n, seed, ds, h=h)
    dep = d["depth"].reshape(2 * n, h, 4 * h)
    pc = np.stack([G.pano2pc(x, ds) for x in dep])
    return pc, np.ones(pc.shape[::2], np.uint8), d["R"].reshape(2 * n, 4, 4)


@pytest.mark.parametrize("ds", ["suncg", "matterport"])
def test_nn_model_against_scipy(ds):
    from scipy.spatial import cKDTree
    pc, valid, R = _clouds(2, 500, ds, 16)
    P = pc.shape[2]
    query = np.tile(np.arange(P, dtype=np.int32), (2, 1))
    r = M.dense_nn(pc, valid, R, query)
    for b in range(2):
        ws, wt = M.to_world(pc[2 * b], R[2 * b]), M.to_world(pc[2 * b + 1], R[2 * b + 1])
        d2, i2 = cKDTree(wt.T).query(ws.T, k=2)
        assert np.array_equal(r["nn_dist"][b], d2[:, 0])
        distinct = d2[:, 0] != d2[:, 1]
        assert distinct.sum() > P // 2
        assert np.array_equal(r["nn_index"][b][distinct], i2[distinct, 0])
        assert np.array_equal(r["hit"][b] != 0, r["nn_dist"][b] < 0.08)


def test_nn_model_ties_invalid_points_and_unused_slots():
    h, P = 2, 16
    rs = np.random.RandomState(0)
    pc = rs.randn(2, 3, P)
    pc[1, :, 9] = pc[1, :, 3]                    # a duplicated target point: the lower index wins
    pc[0, :, 0] = pc[1, :, 3]
    valid = np.ones((2, P), np.uint8)
    valid[0, 5] = 0
    eye = np.tile(np.eye(4), (2, 1, 1))
    r = M.dense_nn(pc, valid, eye, np.array([[0, -1, 5, 0]], np.int32))
    assert r["nn_index"][0].tolist() == [3, -1, -1, 3] and r["nn_dist"][0].tolist() == [0.0, -1.0, -1.0, 0.0]
    assert r["hit"][0].tolist() == [1, 0, 0, 1] and r["idx_tgt"][0, 0].tolist() == [1 + 0 * h, 1] and r["idx_src"][0, 1].tolist() == [0, 0]
    valid[1, 3] = 0
    assert M.dense_nn(pc, valid, eye, np.array([[0]], np.int32))["nn_index"][0, 0] == 9
    valid[1] = 0                                  # a target without a valid point
    r = M.dense_nn(pc, valid, eye, np.array([[0, 1]], np.int32))
    assert r["nn_index"][0].tolist() == [-1, -1] and r["nn_dist"][0].tolist() == [-1.0, -1.0] and not r["hit"].any()


@pytest.mark.parametrize("h", [16, 20])
def test_pano_idx_inverts_the_face_major_order(h):
    ys, xs = np.meshgrid(np.arange(h), np.arange(4 * h), indexing="ij")
    # the face-major index of panorama pixel (x, y), as util.Pano2PointCloud concatenates the faces (util.py:751-811)
    index = (xs // h) * h * h + ys * h + xs % h
    got = M.pano_idx(index.ravel(), h)
    assert np.array_equal(got[:, 0], xs.ravel()) and np.array_equal(got[:, 1], ys.ravel())
    assert sorted(index.ravel().tolist()) == list(range(4 * h * h))


def _rank_case(seed, repeats):
    rs = np.random.RandomState(seed)
    C_, h, K = 32, 32, 100
    f = rs.randn(2, C_, h, 4 * h).astype(np.float32)
    if repeats:                                   # exactly repeated pixels: many distances equal the threshold
        f[1, :, :, 64:] = f[1, :, :, :64]
    idx_src = np.stack([rs.randint(0, 4 * h, K), rs.randint(0, h, K)], -1)[None].astype(np.int32)
    idx_tgt = np.stack([rs.randint(0, 4 * h, K), rs.randint(0, h, K)], -1)[None].astype(np.int32)
    # half of the correspondences are near matches (a small threshold), the rest random (about half of the map is closer)
    for k in range(0, K, 2):
        f[0, :, idx_src[0, k, 1], idx_src[0, k, 0]] = f[1, :, idx_tgt[0, k, 1], idx_tgt[0, k, 0]] + 0.3 * rs.randn(C_).astype(np.float32)
    return f, idx_src, idx_tgt


@pytest.mark.parametrize("repeats", [False, True])
def test_rank_counts_against_float64_and_the_reference_expression(repeats):
    """count must lie in #{d < thr - m} <= count <= #{d <= thr + m} of the float64 distances of the same fp32 inputs, m = 1e-5 max(d, thr):
    a sequential fp32 sum of C <= 64 squared differences is within (C + 2) 2^-24 <= 4e-6 relative on each side.  The reference's own torch
    form (mainPanoCompletion2view.py:403-405) lies in the same bracket; it is not equal to the sequential order where pixels repeat."""
    import torch
    f, idx_src, idx_tgt = _rank_case(3, repeats)
    C_, h = f.shape[1], f.shape[2]
    count, thr, typ = M.descriptor_rank(f, 0, C_, idx_src, idx_tgt)
    assert (typ == -1).all() and count.min() >= 0
    f64 = f.astype(np.float64)
    S = f64[0][:, idx_src[0, :, 1], idx_src[0, :, 0]]                           # [C, K]
    T = f64[1][:, idx_tgt[0, :, 1], idx_tgt[0, :, 0]]
    t64 = ((S - T) ** 2).sum(0)
    d64 = ((S[:, :, None] - f64[1].reshape(C_, 1, -1)) ** 2).sum(0)             # [K, HW]
    m = 1e-5 * np.maximum(d64, t64[:, None])
    lo, hi = (d64 < t64[:, None] - m).sum(1), (d64 <= t64[:, None] + m).sum(1)
    assert np.all(lo <= count[0]) and np.all(count[0] <= hi)
    assert np.allclose(thr[0], t64, rtol=4e-6, atol=0)
    ft = torch.from_numpy(f)
    ix = lambda a: torch.from_numpy(a.astype(np.int64))
    featSrc = ft[0][:, ix(idx_src[0, :, 1]), ix(idx_src[0, :, 0])]
    featTgt = ft[1][:, ix(idx_tgt[0, :, 1]), ix(idx_tgt[0, :, 0])]
    dist = (featSrc - featTgt).pow(2).sum(0)
    ref = ((featSrc.unsqueeze(2) - ft[1].view(C_, 1, -1)).pow(2).sum(0) < dist.unsqueeze(1)).sum(1).numpy()
    assert np.all(lo <= ref) and np.all(ref <= hi)
    # the true match is never counted: its distance is the threshold bit for bit
    tp = idx_tgt[0, :, 1] * 4 * h + idx_tgt[0, :, 0]
    d32 = M.sq_dist(f[0][:, idx_src[0, :, 1], idx_src[0, :, 0]][:, :, None], f[1].reshape(C_, 1, -1))
    assert np.array_equal(d32[np.arange(len(tp)), tp], thr[0])
    if repeats:
        assert np.all(hi - lo >= 1)               # every threshold is met by its repeated pixel as well: the bracket is not a point


def test_rank_model_types_selection_and_invalid_pairs():
    rs = np.random.RandomState(5)
    h, K = 8, 12
    f = rs.randn(4, 9, h, 4 * h).astype(np.float32)
    idx_src = np.stack([rs.randint(0, 4 * h, (2, K)), rs.randint(0, h, (2, K))], -1).astype(np.int32)
    idx_tgt = np.stack([rs.randint(0, 4 * h, (2, K)), rs.randint(0, h, (2, K))], -1).astype(np.int32)
    mask = np.zeros((4, 1, h, 4 * h), np.float32)
    mask[:, :, :, h:2 * h] = 1
    sel = np.array([[0, 3, -1, 3, 11], [1, 1, 2, -1, -1]])
    count, thr, typ = M.descriptor_rank(f, 2, 5, idx_src, idx_tgt, sel, np.array([1, 0]), mask)
    assert (count[1] == -1).all() and (typ[1] == -1).all() and count[0, 2] == -1 and typ[0, 2] == -1
    assert count[0, 1] == count[0, 3] and thr[0, 1] == thr[0, 3] and (count[0, [0, 1, 3, 4]] >= 0).all()
    obs = lambda x: int(h <= x < 2 * h)
    assert typ[0, 0] == obs(idx_src[0, 0, 0]) + obs(idx_tgt[0, 0, 0])
    full = M.descriptor_rank(f, 2, 5, idx_src, idx_tgt)[0]
    assert full.shape == (2, K) and full[0, 3] == count[0, 1]


@pytest.fixture(scope="module")
def selections():
    """hits and validity of make_pairs(4, 500, ds) under the model: h = 32 with 4096 queries, and h = 16 with 1024 (as many draws as the
    cloud has points; with 4096 draws from these 1024 points the same pairs collect 539-1068 hits and pass the bar of 500)."""
    out = {}
    for ds in ("suncg", "matterport"):
        for h, nq in ((32, 4096), (16, 1024)):
            pc, valid, R = _clouds(4, 500, ds, h)
            out[ds, h] = M.dense_correspondences(pc, valid, R, np.random.RandomState(500), n_query=nq)
    return out


@pytest.mark.parametrize("ds", ["suncg", "matterport"])
def test_fixed_thresholds_on_the_synthetic_pairs(selections, ds):
    """The reference's bars (0.08 m, 500 hits, datasets/SUNCG.py:328-333) on the synthetic rooms: passed as is, make_pairs' camera-to-world R
    aligns the clouds -- every pair is valid at h = 32 (1502-2558 hits of 4096 queries) and none at h = 16 (118-286 hits of 1024 queries)."""
    r = selections[ds, 32]
    print("hits h=32", ds, r["hits"])
    assert (r["valid"] == 1).all() and (r["hits"] >= 500).all()
    assert r["idxSrc"].shape == (4, 2000, 2) and r["idxSrc"][..., 0].max() < 128 and r["idxSrc"][..., 1].max() < 32
    r = selections[ds, 16]
    print("hits h=16", ds, r["hits"])
    assert (r["valid"] == 0).all() and not r["idxSrc"].any() and not r["idxTgt"].any()


def test_draw_order_is_the_references_for_one_pair():
    pc, valid, R = _clouds(1, 500, "suncg", 32)
    r = M.dense_correspondences(pc, valid, R, np.random.RandomState(9), n_query=4096)
    rs = np.random.RandomState(9)                                        # datasets/SUNCG.py:324, :338
    q = rs.choice(range(4096), 4096)
    nn = M.dense_nn(pc, valid, R, q[None].astype(np.int32))
    hit = nn["hit"][0] != 0
    pick = rs.choice(range(int(hit.sum())), 2000)
    assert np.array_equal(r["idxSrc"][0], M.pano_idx(q[hit], 32)[pick]) and np.array_equal(r["idxTgt"][0], nn["idx_tgt"][0][hit][pick])


# ----------------------------------------------------------------------------------------------------------------- ABI and plumbing
def test_header_declares_the_descriptor_symbols():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    for sym in ("relpose_dense_nn", "relpose_descriptor_rank"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "typedef struct RelposeDenseNnArgs" in h and "typedef struct RelposeDescRankArgs" in h
    for cite in ("datasets/SUNCG.py:315-341", "mainPanoCompletion2view.py:535-542", "mainPanoCompletion2view.py:383-414"):
        assert cite in h, cite
    from relativepose_amd import _lib, build
    assert int(re.search(r"#define RELPOSE_DESC_MAX_CHANNELS (\d+)", h).group(1)) == _lib.DESC_MAX_CHANNELS == 64
    assert ("descriptor.hip", ["-ffp-contract=off"]) in build.SOURCES
    for sym in ("relpose_dense_nn", "relpose_descriptor_rank"):
        assert sym in _lib.SIGNATURES


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
@pytest.mark.parametrize("name", ["DenseNnArgs", "DescRankArgs"])
def test_args_layout_matches_ctypes(tmp_path, name):
    from relativepose_amd import _lib
    cls = getattr(_lib, name)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof(Relpose{name}));\n' +
                   "".join(f'  printf(" %zu", offsetof(Relpose{name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]


def test_invalid_arguments_return_einval_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_double * 64)()                      # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)

    def nn(**kw):
        a = _lib.DenseNnArgs()
        a.struct_size = C.sizeof(a)
        a.n_pairs, a.n_points, a.n_query, a.h = 1, 16, 4, 2
        for k in ("pc", "valid", "to_world", "query", "nn_index", "nn_dist", "hit", "idx_src", "idx_tgt"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.relpose_dense_nn(C.byref(a))

    assert L.relpose_dense_nn(None) == -1
    for bad in (dict(pc=None), dict(query=None), dict(nn_index=None), dict(hit=None), dict(idx_tgt=None), dict(n_pairs=0), dict(n_points=0),
                dict(n_query=0), dict(h=0), dict(n_points=17), dict(max_dist=-1.0), dict(struct_size=8)):
        assert nn(**bad) == -1, bad

    def rank(**kw):
        a = _lib.DescRankArgs()
        a.struct_size = C.sizeof(a)
        a.n_pairs, a.h, a.total_channels, a.feat_off, a.n_channels, a.n_corres, a.n_slots = 1, 2, 8, 2, 5, 4, 4
        for k in ("f", "idx_src", "idx_tgt", "count", "thr", "type"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.relpose_descriptor_rank(C.byref(a))

    assert L.relpose_descriptor_rank(None) == -1
    for bad in (dict(f=None), dict(idx_src=None), dict(count=None), dict(thr=None), dict(type=None), dict(n_pairs=0), dict(h=0),
                dict(n_channels=0), dict(n_channels=65, total_channels=80), dict(feat_off=4), dict(feat_off=-1), dict(n_corres=0),
                dict(sel=p, n_slots=0), dict(f=p + 4), dict(struct_size=8)):
        assert rank(**bad) == -1, bad


def test_meta_kernel_shapes():
    import torch
    from relativepose_amd import ops
    assert "dense_nn" in ops.OPS and "descriptor_rank" in ops.OPS
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    r = torch.ops.relpose.dense_nn(e(64, 3, 102400, dt=torch.float64), e(64, 102400, dt=torch.uint8), e(64, 4, 4, dt=torch.float64),
                                   e(32, 5000, dt=torch.int32))
    assert [tuple(t.shape) for t in r] == [(32, 5000)] * 3 + [(32, 5000, 2)] * 2
    assert [t.dtype for t in r] == [torch.int32, torch.float64, torch.uint8, torch.int32, torch.int32]
    idx = e(32, 2000, 2, dt=torch.int32)
    c, t, y = torch.ops.relpose.descriptor_rank(e(64, 54, 160, 640), 22, 32, idx, idx, e(32, 100, dt=torch.int32))
    assert c.shape == t.shape == y.shape == (32, 100) and (c.dtype, t.dtype, y.dtype) == (torch.int32, torch.float32, torch.int32)
    c, _, _ = torch.ops.relpose.descriptor_rank(e(64, 54, 160, 640), 22, 32, idx, idx)
    assert c.shape == (32, 2000)


def test_cli_refuses_more_than_one_gpu():
    from relativepose_amd import evaluation
    with pytest.raises(SystemExit, match="one GPU"):
        evaluation.main(["--descriptor-eval", "--gpus", "2", "--dataset", "suncg"])
