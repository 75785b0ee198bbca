"""GPU: the descriptor-evaluation kernels (csrc/descriptor.hip: relpose_dense_nn, relpose_descriptor_rank) against the numpy model of their
contract (tests/descriptor_model.py), bit for bit, and their uses: descriptor.dense_correspondences / evalDLDescriptor,
torch.ops.relpose.dense_nn / descriptor_rank and evaluation --descriptor-eval.  Reference: datasets/SUNCG.py:315-341,
mainPanoCompletion2view.py:383-414, :535-542."""
import json

import numpy as np
import pytest

import descriptor_model as M
from gpu_util import log

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _clouds(n, seed, ds, h):
    """(pc, valid, R) numpy of make_pairs through the device's pano2pc, and the depth tensor."""
    import torch
    from relativepose_amd import synth, util
    d = synth.make_pairs(n, seed, ds, h=h)
    depth = _t(d["depth"].reshape(2 * n, h, 4 * h))
    pc, valid = util.pano2pc_dev(depth, ds)
    return pc.cpu().numpy(), valid.cpu().numpy(), d["R"].reshape(2 * n, 4, 4), depth


def _nn(pc, valid, R, query, **kw):
    from relativepose_amd import descriptor
    r = descriptor.dense_nn_dev(_t(pc), _t(valid), _t(R), _t(query), **kw)
    return dict(zip(("nn_index", "nn_dist", "hit", "idx_src", "idx_tgt"), (t.cpu().numpy() for t in r)))


def _same_nn(got, ref):
    for k in ("nn_index", "hit", "idx_src", "idx_tgt"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["nn_dist"].view(np.uint64), ref["nn_dist"].view(np.uint64))


@pytest.mark.parametrize("ds", ["suncg", "matterport"])
@pytest.mark.parametrize("h", [16, 20])
def test_dense_nn_matches_the_model_bitwise(h, ds):
    pc, valid, R, _ = _clouds(3, 500, ds, h)
    P = pc.shape[2]                                    # 1024, or 1600: not a multiple of the 256-query block or the 1024-point tile
    rs = np.random.RandomState(h)
    query = np.stack([np.concatenate([rs.permutation(P), [-1, 5, 5, -1, P - 1, 0, 0, -1, 7, 7, 7, -1, 1]]) for _ in range(3)]).astype(np.int32)
    valid = valid.copy()
    valid[3] = 0                                       # pair 1: a target without a valid point
    valid[4, ::7] = 0                                  # pair 2: invalid source points
    valid[5, 1::3] = 0                                 # ... and invalid target points
    got, ref = _nn(pc, valid, R, query), M.dense_nn(pc, valid, R, query)
    _same_nn(got, ref)
    assert (got["nn_index"][1] == -1).all() and (got["nn_index"][0][:P] >= 0).all() and (got["nn_index"][2][:P] == -1).sum() == len(range(0, P, 7))
    assert valid[5][got["nn_index"][2][got["nn_index"][2] >= 0]].all()
    log("dense_nn_model", h=h, dataset=ds, hits=got["hit"].sum(1))


def test_dense_nn_tie_goes_to_the_lowest_index():
    h, P = 24, 4 * 24 * 24                              # 2304 points: three tiles, the duplicates in different tiles
    rs = np.random.RandomState(1)
    pc = rs.randn(2, 3, P)
    T = np.stack([np.eye(4), np.eye(4)])
    T[1, :3, 3] = [0.5, -0.25, 2.0]                     # exact in binary: duplicated points stay duplicates after the transform
    q = np.arange(40)
    pc[1][:, 2000 + q] = pc[1][:, 100 + q]              # every target point 100.. also sits at 2000..
    pc[0][:, q] = pc[1][:, 100 + q] + T[1, :3, 3][:, None]
    valid = np.ones((2, P), np.uint8)
    query = np.concatenate([q, rs.randint(0, P, 300)])[None].astype(np.int32)
    got, ref = _nn(pc, valid, T, query), M.dense_nn(pc, valid, T, query)
    _same_nn(got, ref)
    assert np.array_equal(got["nn_index"][0, :40], 100 + q) and (got["nn_dist"][0, :40] == 0).all()
    valid[1, 100:120] = 0                               # without the first copy the second one wins
    got = _nn(pc, valid, T, query)
    _same_nn(got, M.dense_nn(pc, valid, T, query))
    assert np.array_equal(got["nn_index"][0, :20], 2000 + q[:20]) and np.array_equal(got["nn_index"][0, 20:40], 100 + q[20:])
    assert np.array_equal(_nn(pc, valid, T, query, max_dist=0.0)["hit"], got["hit"])          # 0 = the reference's 0.08


def _rank_case(h, Ct, off, C_, B=3, K=64, seed=0):
    rs = np.random.RandomState(seed + h + Ct)
    w = 4 * h
    f = rs.randn(2 * B, Ct, h, w).astype(np.float32)
    idx_src = np.stack([rs.randint(0, w, (B, K)), rs.randint(0, h, (B, K))], -1).astype(np.int32)
    idx_tgt = np.stack([rs.randint(0, w, (B, K)), rs.randint(0, h, (B, K))], -1).astype(np.int32)
    # a constant band in pair 0's target map: every pixel of rows 3 and 4 equals the true match of correspondences 0..3 exactly
    f[1, off:off + C_, 3:5, :] = f[1, off:off + C_, 3, 0][:, None, None]
    idx_tgt[0, :4, 1] = 3
    for b in range(B):                                  # near matches: small thresholds, small counts
        for k in range(0, K, 2):
            f[2 * b, off:off + C_, idx_src[b, k, 1], idx_src[b, k, 0]] = \
                f[2 * b + 1, off:off + C_, idx_tgt[b, k, 1], idx_tgt[b, k, 0]] + (0.4 * rs.randn(C_)).astype(np.float32)
    mask = np.zeros((2 * B, 1, h, w), np.float32)
    mask[:, :, :, h:2 * h] = 1
    return f, idx_src, idx_tgt, mask


def _rank(f, off, C_, idx_src, idx_tgt, sel=None, pair_valid=None, mask=None):
    from relativepose_amd import descriptor
    o = lambda a: None if a is None else _t(a)
    r = descriptor.descriptor_rank_dev(_t(f), off, C_, _t(idx_src), _t(idx_tgt), o(sel), o(pair_valid), o(mask))
    return tuple(t.cpu().numpy() for t in r)


def _same_rank(got, ref):
    assert np.array_equal(got[0], ref[0]), "count"
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), "thr"
    assert np.array_equal(got[2], ref[2]), "type"


# (54, 22, 32): SCNet's output with 15 classes; (9, 2, 5), (20, 1, 12) and (70, 3, 64): the other register tiles of the kernel (8, 16, 64 channels)
@pytest.mark.parametrize("shape", [(54, 22, 32), (9, 2, 5), (20, 1, 12), (70, 3, 64)])
@pytest.mark.parametrize("h", [16, 20])
def test_descriptor_rank_matches_the_model_bitwise(h, shape):
    Ct, off, C_ = shape
    f, idx_src, idx_tgt, mask = _rank_case(h, Ct, off, C_)
    rs = np.random.RandomState(7)
    sel = rs.randint(0, 64, (3, 37)).astype(np.int32)
    sel[:, [2, 11, 36]] = -1
    sel[:, 5] = sel[:, 4]
    sel[0, :4] = [0, 1, 2, 3]                           # the correspondences whose match lies in the constant band
    pv = np.array([1, 0, 1], np.uint8)
    got, ref = _rank(f, off, C_, idx_src, idx_tgt, sel, pv, mask), M.descriptor_rank(f, off, C_, idx_src, idx_tgt, sel, pv, mask)
    _same_rank(got, ref)
    assert (got[0][1] == -1).all() and (got[0][:, [11, 36]] == -1).all() and (got[0][0, :4] >= 0).all() and got[0][0, 4] == got[0][0, 5]
    # the band's 8 h pixels are at the threshold exactly: none of them is counted, whatever else is
    band = M.sq_dist(f[0, off:off + C_, idx_src[0, 0, 1], idx_src[0, 0, 0]][:, None], f[1, off:off + C_, 3:5].reshape(C_, -1))
    assert (band == got[1][0, 0]).all() and got[0][0, 0] <= 4 * h * h - 8 * h
    # every correspondence, no selection, no pair flags, no mask
    got, ref = _rank(f, off, C_, idx_src, idx_tgt), M.descriptor_rank(f, off, C_, idx_src, idx_tgt)
    _same_rank(got, ref)
    assert got[0].shape == (3, 64) and (got[2] == -1).all() and (got[0] >= 0).all()
    log("descriptor_rank_model", h=h, shape=shape, mean_count=float(got[0].mean()))


def test_descriptor_rank_more_slots_than_one_chunk():
    f, idx_src, idx_tgt, mask = _rank_case(20, 54, 22, 32)
    sel = np.random.RandomState(3).randint(-1, 64, (3, 300)).astype(np.int32)       # 300 slots: three LDS chunks of 128, the last one partial
    _same_rank(_rank(f, 22, 32, idx_src, idx_tgt, sel, None, mask), M.descriptor_rank(f, 22, 32, idx_src, idx_tgt, sel, None, mask))


def test_batch_of_8_equals_single_calls_and_repeats_bitwise():
    pc, valid, R, _ = _clouds(8, 500, "matterport", 16)
    query = np.random.RandomState(0).randint(-1, 1024, (8, 700)).astype(np.int32)
    a, a2 = _nn(pc, valid, R, query), _nn(pc, valid, R, query)
    f, idx_src, idx_tgt, mask = _rank_case(16, 54, 22, 32, B=8)
    sel = np.random.RandomState(1).randint(-1, 64, (8, 150)).astype(np.int32)
    pv = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
    r, r2 = _rank(f, 22, 32, idx_src, idx_tgt, sel, pv, mask), _rank(f, 22, 32, idx_src, idx_tgt, sel, pv, mask)
    for k in a:
        assert np.array_equal(a[k], a2[k]), k
    for x, y in zip(r, r2):
        assert np.array_equal(x, y)
    for b in range(8):
        s = _nn(pc[2 * b:2 * b + 2], valid[2 * b:2 * b + 2], R[2 * b:2 * b + 2], query[b:b + 1])
        for k in a:
            assert np.array_equal(a[k][b:b + 1], s[k]), (b, k)
        s = _rank(f[2 * b:2 * b + 2], 22, 32, idx_src[b:b + 1], idx_tgt[b:b + 1], sel[b:b + 1], pv[b:b + 1], mask[2 * b:2 * b + 2])
        for x, y in zip(r, s):
            assert np.array_equal(x[b:b + 1], y), b


@pytest.fixture(scope="module")
def shim_case():
    """make_pairs(4, 500, 'suncg', h = 32), its correspondences with the defaults from the device and from the model, and a feature map."""
    from relativepose_amd import descriptor
    pc, valid, R, depth = _clouds(4, 500, "suncg", 32)
    dev = descriptor.dense_correspondences(depth, R, "suncg", np.random.RandomState(11))
    ref = M.dense_correspondences(pc, valid, R, np.random.RandomState(11))
    f = np.random.RandomState(2).randn(8, 54, 32, 128).astype(np.float32)
    return dev, ref, f


def test_dense_correspondences_equal_the_model(shim_case):
    dev, ref, _ = shim_case
    assert set(dev) == {"idxSrc", "idxTgt", "valid"}
    assert dev["idxSrc"].shape == (4, 2000, 2) and dev["valid"].tolist() == [1, 1, 1, 1]
    for k in dev:
        assert np.array_equal(dev[k], ref[k]), k
    log("dense_correspondences", hits=ref["hits"])


@pytest.mark.parametrize("n_eval", [100, None])
def test_eval_dl_descriptor_equals_the_model(shim_case, n_eval):
    from relativepose_amd import descriptor, util
    import torch
    dev, _, f = shim_case
    dev = dict(dev, valid=np.array([1, 1, 0, 1]))
    _, mask = util.apply_mask_dev(torch.ones(8, 1, 32, 128, device=_dev()), "second")
    got = descriptor.evalDLDescriptor(_t(f), 22, 32, dev, mask, np.random.RandomState(4), n_eval=n_eval)
    ref = M.eval_dl_descriptor(f, 22, 32, dev, mask.cpu().numpy(), np.random.RandomState(4), n_eval=n_eval)
    assert len(got[0]) == len(ref[0]) and len(got[1]) == len(ref[1]) == 3
    for g, r in zip(got[0] + got[1], ref[0] + ref[1]):
        assert g.dtype == np.float32 and g == r
    assert all(0.0 <= g <= 1.0 for g in got[0] + got[1])


def test_small_panoramas_give_no_valid_pair():
    """h = 16 with one draw per cloud point (n_query = 1024): 118-286 hits per pair, below the reference's bar of 500 -- every pair comes
    back valid 0 and contributes nothing to the metric."""
    from relativepose_amd import descriptor
    pc, valid, R, depth = _clouds(4, 500, "suncg", 16)
    dev = descriptor.dense_correspondences(depth, R, "suncg", np.random.RandomState(500), n_query=1024)
    ref = M.dense_correspondences(pc, valid, R, np.random.RandomState(500), n_query=1024)
    assert dev["valid"].tolist() == [0, 0, 0, 0] and not dev["idxSrc"].any() and not dev["idxTgt"].any()
    assert np.array_equal(ref["valid"], dev["valid"]) and (ref["hits"] < 500).all()
    f = _t(np.random.RandomState(0).randn(8, 54, 16, 64).astype(np.float32))
    assert descriptor.evalDLDescriptor(f, 22, 32, dev, None, np.random.RandomState(0)) == ([], [])


def test_torch_ops_match_the_direct_calls():
    import torch
    from relativepose_amd import descriptor, ops  # noqa: F401
    pc, valid, R, _ = _clouds(2, 77, "suncg", 16)
    query = _t(np.random.RandomState(0).randint(-1, 1024, (2, 300)).astype(np.int32))
    a = torch.ops.relpose.dense_nn(_t(pc), _t(valid), _t(R), query)
    b = descriptor.dense_nn_dev(_t(pc), _t(valid), _t(R), query)
    assert len(a) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))
    f, idx_src, idx_tgt, mask = _rank_case(16, 54, 22, 32, B=2)
    sel = _t(np.random.RandomState(1).randint(-1, 64, (2, 20)).astype(np.int32))
    a = torch.ops.relpose.descriptor_rank(_t(f), 22, 32, _t(idx_src), _t(idx_tgt), sel, None, _t(mask))
    b = descriptor.descriptor_rank_dev(_t(f), 22, 32, _t(idx_src), _t(idx_tgt), sel, None, _t(mask))
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
    a = torch.ops.relpose.descriptor_rank(_t(f), 22, 32, _t(idx_src), _t(idx_tgt))
    assert a[0].shape == (2, 64) and int(a[2].max()) == -1


def test_evaluation_descriptor_eval_prints_one_json_line(capsys):
    from relativepose_amd import evaluation
    evaluation.main(["--descriptor-eval", "--dataset", "suncg", "--pairs", "4", "--batch", "4"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert {"metric", "pairs", "valid_pairs", "ratio_obs", "ratio_unobs", "seconds"} <= set(r)
    assert r["metric"] == "descriptor_rank" and r["pairs"] == 4 and 0 < r["valid_pairs"] <= 4
    assert 0.0 <= r["ratio_obs"] <= 1.0 and 0.0 <= r["ratio_unobs"] <= 1.0
    log("descriptor_eval_cli", **r)
