"""GPU: the completion-loss kernels (csrc/completion.hip: relpose_completion_loss, relpose_contrast_loss) against the numpy model of their
contract (tests/completion_model.py), and their uses: completion.contrast_loss on the reference's golden cases,
torch.ops.relpose.completion_loss / contrast_loss, evaluation.evaluate_completion and --completion-eval.  Reference:
mainPanoCompletion2view.py:429-455, :549-567."""
import json
import os

import numpy as np
import pytest

import completion_model as M
from gpu_util import log

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "completion.npz")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _loss_inputs(N, h, S, seed=0):
    """Ct = 7 + S + 32 channels like SCNet's output; 5 % zero-depth pixels, 1 % labels >= S, logits up to +-80 (an un-shifted float32 or
    float64-of-float32 exp of 80 is finite, but sum exp(z) against exp(-80) loses the small terms: the shift is what is tested)."""
    rs = np.random.RandomState(seed + 7 * N + h + S)
    H, W = h, 4 * h
    f = rs.randn(N, 7 + S + 32, H, W).astype(np.float32)
    f[:, 7:7 + S] = rs.uniform(-80, 80, (N, S, H, W)).astype(np.float32)
    f[:, 7:7 + S][rs.rand(N, S, H, W) < 0.02] = 80
    complete = rs.randn(N, 7, H, W).astype(np.float32)
    complete[:, 6][rs.rand(N, H, W) < 0.05] = 0
    label = rs.randint(0, S, (N, H, W)).astype(np.uint8)
    label[rs.rand(N, H, W) < 0.01] = rs.randint(S, 256)
    mask = np.zeros((N, 1, H, W), np.float32)
    mask[:, :, :, h:2 * h] = 1
    weight = (0.2 + rs.rand(N, H, W)).astype(np.float32)
    return f, complete, label, mask, weight


def _loss(f, complete, label, mask, weight, S, **kw):
    from relativepose_amd import completion
    r = completion.completion_loss_dev(_t(f), _t(complete), _t(label), _t(mask), _t(weight), S=S, **kw)
    return dict(zip(("sums", "ce_mag", "ce_cross", "n_bad_label"), (x.cpu().numpy() for x in r)))


def _check_loss(got, ref, tag):
    """rgb / n / d / w rows: identical non-negative fp32 terms, so a float64 sum of <= 2^23 of them in any order is within
    2^23 2^-53 = 9.3e-10 relative: 1e-9.  ce row and ce_cross: 1e-9 of the un-cancelled magnitude."""
    N = len(ref["sums"])
    worst = 0.0
    for r in (0, 1, 2, 4):
        err = np.abs(got["sums"][:, r] - ref["sums"][:, r])
        worst = max(worst, float((err / np.maximum(ref["sums"][:, r], 1e-300)).max()))
        assert (err <= 1e-9 * ref["sums"][:, r]).all(), (tag, M.ROWS[r], err, ref["sums"][:, r])
    ce_err = np.abs(got["sums"][:, 3] - ref["sums"][:, 3]).max(1)
    mag = np.maximum(ref["ce_mag"], 1e-300)
    print(f"{tag}: L1 / w rows worst rel {worst:.2e}; ce err / ce_mag {float((ce_err / mag).max()):.2e}")
    assert (ce_err <= 1e-9 * ref["ce_mag"]).all(), (tag, ce_err, ref["ce_mag"])
    assert (np.abs(got["ce_mag"] - ref["ce_mag"]) <= 1e-9 * ref["ce_mag"]).all(), tag
    assert abs(got["ce_cross"][0] - ref["ce_cross"]) <= 1e-9 * ref["ce_cross_mag"], (tag, got["ce_cross"], ref["ce_cross"])
    assert np.array_equal(got["n_bad_label"], ref["n_bad_label"]), tag
    assert got["sums"].shape == (N, 5, 2) and got["n_bad_label"].dtype == np.int32
    return worst, float((ce_err / mag).max())


# h = 20: 1600 pixels, no multiple of the 1024-pixel block or the 256-pixel block of the cross pass; h = 160: the real map, 100 blocks per image
@pytest.mark.parametrize("shape", [(2, 8, 15), (6, 8, 21), (2, 20, 15), (2, 160, 15)])
def test_completion_loss_matches_the_model(shape):
    N, h, S = shape
    f, complete, label, mask, weight = _loss_inputs(N, h, S)
    assert (complete[:, 6] == 0).any() and (label >= S).any() and np.abs(f[:, 7:7 + S]).max() >= 79
    for wt, tag in ((None, "plain"), (weight, "weight")):
        ref = M.completion_loss(f, complete, label, mask, wt, S=S)
        got = _loss(f, complete, label, mask, wt, S)
        worst = _check_loss(got, ref, f"{shape} {tag}")
        assert ref["n_bad_label"].sum() > 0 and (ref["sums"][:, 3] > 0).all() and (ref["sums"][:, :3, 0] > 0).all()
        log("completion_loss_model", shape=shape, weight=tag, l1_rel=worst[0], ce_rel_mag=worst[1])
        # without ce_cross the other outputs are the same bits
        g2 = _loss(f, complete, label, mask, wt, S, with_cross=False)
        assert np.array_equal(g2["sums"], got["sums"]) and np.array_equal(g2["ce_mag"], got["ce_mag"]) and g2["ce_cross"][0] == 0
    # no labels: no CE rows, the L1 rows unchanged
    ref = M.completion_loss(f, complete, None, mask, weight, S=S)
    got0 = _loss(f, complete, None, mask, weight, S)
    _check_loss(got0, ref, f"{shape} no label")
    assert not got0["sums"][:, 3].any() and not got0["ce_mag"].any() and got0["ce_cross"][0] == 0 and not got0["n_bad_label"].any()
    assert np.array_equal(got0["sums"][:, [0, 1, 2, 4]], got["sums"][:, [0, 1, 2, 4]])


def test_completion_loss_rows_do_not_depend_on_the_batch_and_repeat_bitwise():
    f, complete, label, mask, weight = _loss_inputs(6, 20, 15, seed=3)
    a, a2 = _loss(f, complete, label, mask, weight, 15), _loss(f, complete, label, mask, weight, 15)
    for k in a:
        assert np.array_equal(a[k], a2[k]), k
    sl = slice(2, 4)
    b = _loss(f[sl], complete[sl], label[sl], mask[sl], weight[sl], 15)
    for k in ("sums", "ce_mag", "n_bad_label"):
        assert np.array_equal(a[k][sl], b[k]), k
    assert a["ce_cross"][0] != b["ce_cross"][0]                   # the one output that is a property of the batch


def test_completion_loss_reads_no_feature_channel():
    S = 15
    f, complete, label, mask, weight = _loss_inputs(2, 20, S, seed=5)
    a = _loss(f, complete, label, mask, weight, S)
    f2 = f.copy()
    f2[:, 7 + S:] = np.nan
    b = _loss(f2, complete, label, mask, weight, S)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["sums"]).all()


def _contrast_inputs(B, h, K, M_, C_, seed=0):
    rs = np.random.RandomState(seed + B + K + C_)
    Ct, off = (54, 22) if C_ == 32 else (C_ + 10, 5)
    f = rs.randn(2 * B, Ct, h, 4 * h).astype(np.float32)
    f[:, off:off + C_] = (0.15 * np.tanh(rs.randn(2 * B, C_, h, 4 * h))).astype(np.float32)
    f[:, :off] = np.nan                                            # the other channels are never read
    f[:, off + C_:] = np.nan
    idx = lambda *s: np.stack([rs.randint(0, 4 * h, s), rs.randint(0, h, s)], -1).astype(np.int32)
    isrc, itgt, neg = idx(B, K), idx(B, K), idx(B, K, M_)
    isrc[0, 1] = [4 * h, 0]                                        # outside: x past the right edge (its M negatives are skipped too)
    itgt[0, 2] = [0, -1]
    neg[0, 0, 3] = [-1, 2]
    neg[B - 1, K - 1, M_ - 1] = [3, h]
    pv = np.ones(B, np.uint8)
    if B > 1:
        pv[1] = 0
    return f, off, isrc, itgt, pv, neg


def _contrast(f, off, C_, isrc, itgt, pv, neg, margin=0.5):
    from relativepose_amd import completion
    r = completion.contrast_loss_dev(_t(f), off, C_, _t(isrc), _t(itgt), _t(pv), _t(neg), margin)
    return tuple(x.cpu().numpy() for x in r)


# (3, 8, 5, 7, 32): fewer correspondences than a block holds and fewer negatives than a wave has lanes; (1, 16, 64, 100, 20): four blocks
@pytest.mark.parametrize("shape", [(2, 8, 16, 100, 32), (3, 8, 5, 7, 32), (1, 16, 64, 100, 20)])
def test_contrast_loss_matches_the_model(shape):
    B, h, K, M_, C_ = shape
    f, off, isrc, itgt, pv, neg = _contrast_inputs(*shape)
    got = _contrast(f, off, C_, isrc, itgt, pv, neg)
    ref = M.contrast_loss(f, off, C_, isrc, itgt, pv, neg)
    print(shape, "n_active", got[2], "of", K * M_, "n_skipped", got[3], "pos", got[0], "neg", got[1])
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert (np.abs(got[0] - ref[0]) <= 1e-9 * ref[0]).all() and (np.abs(got[1] - ref[1]) <= 1e-9 * ref[1]).all()
    assert ref[3][0] >= 2 + M_ + 1 and 0 < ref[2][0] < K * M_ and ref[0][0] > 0 and ref[1][0] > 0
    if B > 1:
        assert got[0][1] == 0 and got[1][1] == 0 and got[2][1] == 0 and got[3][1] == 0
    again = _contrast(f, off, C_, isrc, itgt, pv, neg)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    # pair_valid absent = all valid; pair 0 does not change with the batch around it
    allv = _contrast(f, off, C_, isrc, itgt, None, neg)
    assert all(x[0] == y[0] for x, y in zip(got, allv)) and (B == 1 or allv[0][1] > 0)
    one = _contrast(f[:2], off, C_, isrc[:1], itgt[:1], None, neg[:1])
    assert all(x[0] == y[0] for x, y in zip(got, one))
    log("contrast_loss_model", shape=shape, n_active=got[2], n_skipped=got[3])


@pytest.mark.parametrize("s", [0, 1, 2])
def test_contrast_loss_matches_the_reference_golden(s):
    """completion.contrast_loss (device) against learner.contrast_loss's own float32 scalars: 1e-5 (tests/test_completion_cpu.py)."""
    from relativepose_amd import completion
    g = np.load(GOLDEN)
    f = np.ascontiguousarray(np.stack([g[f"contrast_{s}_fs"], g[f"contrast_{s}_ft"]], 1).reshape(4, 32, 8, 32))
    dc = {"idxSrc": g[f"contrast_{s}_idx_src"].astype(np.float64), "idxTgt": g[f"contrast_{s}_idx_tgt"].astype(np.float64), "valid": g[f"contrast_{s}_valid"]}
    det = {}
    fl, lp, ln = completion.contrast_loss(_t(f), 0, 32, dc, np.random.RandomState(1000 + s), details=det)
    ref = g[f"contrast_{s}_loss"]
    rel = [abs(a - float(b)) / float(b) for a, b in zip((fl, lp, ln), ref)]
    print(f"seed {s}: rel", rel, det)
    assert max(rel) < 1e-5
    nv = int(g[f"contrast_{s}_valid"].sum())
    assert det["valid_pairs"] == nv and det["n_skipped"] == 0
    assert det["n_active"] / (nv * 16 * 100) == pytest.approx(float(g[f"contrast_{s}_active"]), abs=2e-3)
    model = M.contrast_scalars(f, 0, 32, dc, np.random.RandomState(1000 + s))
    assert max(abs(a - b) / b for a, b in zip((fl, lp, ln), model)) < 1e-9


def test_torch_ops_match_the_direct_calls():
    import torch
    from relativepose_amd import completion, ops  # noqa: F401
    f, complete, label, mask, weight = _loss_inputs(2, 8, 15)
    a = torch.ops.relpose.completion_loss(_t(f), _t(complete), _t(label), _t(mask), _t(weight), 15)
    b = completion.completion_loss_dev(_t(f), _t(complete), _t(label), _t(mask), _t(weight), S=15)
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    a = torch.ops.relpose.completion_loss(_t(f), _t(complete), None, _t(mask), None, 15)
    b = completion.completion_loss_dev(_t(f), _t(complete), None, _t(mask), None, S=15)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[2]) == 0
    f, off, isrc, itgt, pv, neg = _contrast_inputs(2, 8, 16, 100, 32)
    a = torch.ops.relpose.contrast_loss(_t(f), off, 32, _t(isrc), _t(itgt), _t(pv), _t(neg))
    b = completion.contrast_loss_dev(_t(f), off, 32, _t(isrc), _t(itgt), _t(pv), _t(neg))
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    a = torch.ops.relpose.contrast_loss(_t(f), off, 32, _t(isrc), _t(itgt), None, _t(neg), 0.75)
    b = completion.contrast_loss_dev(_t(f), off, 32, _t(isrc), _t(itgt), None, _t(neg), 0.75)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[2][1]) > 0


def _net(precision="f32", S=15):
    from types import SimpleNamespace
    from relativepose_amd import weights
    from relativepose_amd.model import SCNet
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(7, S))
    net.set_precision(precision)
    return net


@pytest.fixture(scope="module")
def eval_runs():
    """evaluate_completion on 2 synthetic SUNCG pairs at h = 32 in the three precisions the ordering test compares."""
    from relativepose_amd import evaluation
    out = {}
    for prec in ("f32", "bf16x6", "f16"):
        batches = [evaluation.SyntheticBatch(2, 500, "suncg", "second", 1, h=32)]
        out[prec] = evaluation.evaluate_completion(batches, _net(prec), _dev(), "suncg", "second", seed=9)
    return out


def _numbers(r):
    return [v for t in ("type0", "type1") for v in r[t].values()]


def test_evaluate_completion_reports_finite_numbers(eval_runs):
    r = eval_runs["f32"]
    assert r["pairs"] == 2 and 0 < r["valid_pairs"] <= 2 and r["n_bad_label"] == 0
    keys = {"errG_rgb", "errG_n", "errG_d", "errG_s", "ce_diag", "loss_fl", "loss_fl_pos", "loss_fl_neg", "n_active", "n_skipped"}
    for t in ("type0", "type1"):
        assert keys <= set(r[t])
        for n in ("errG_rgb", "errG_n", "errG_d", "ce_diag"):
            assert {n + "_obs", n + "_unobs"} <= set(r[t])
            assert r[t][n + "_obs"] + r[t][n + "_unobs"] == pytest.approx(r[t][n], rel=1e-12)
        assert r[t]["errG_rgb"] > 0 and r[t]["errG_s"] > 0 and r[t]["loss_fl_pos"] > 0 and r[t]["n_skipped"] == 0
    assert all(np.isfinite(v) for v in _numbers(r))
    assert r["type0"]["errG_rgb"] != r["type1"]["errG_rgb"]         # the second forward saw the warped other view
    log("evaluate_completion", **{f"{t}_{k}": v for t in ("type0", "type1") for k, v in r[t].items()})


def test_evaluate_completion_type0_equals_direct_kernel_calls(eval_runs):
    import torch
    from relativepose_amd import completion, descriptor, evaluation, synth, util
    from relativepose_amd.pipeline import RelativePosePipeline
    net = _net("f32")
    sub = evaluation.SyntheticBatch(2, 500, "suncg", "second", 1, h=32).take(np.arange(2))
    n, h = 2, 32
    pipe = RelativePosePipeline(net, "suncg", "second", alter_steps=1)
    st = pipe.prepare(sub["rgb"], sub["norm"], sub["depth"], np.zeros((n, 2, 1, 2)), np.zeros((n, 2, 1)), _dev())
    x = pipe._net_input(st)
    x[:, 8:].zero_()
    f = net.forward(x, out=st["f"], zero_warp=True)
    complete = torch.cat((st["rgb"], st["norm"], st["depth"][:, None]), 1).contiguous()
    label = _t(synth.make_labels(sub["norm"], 15).reshape(2 * n, h, 4 * h))
    _, mask = util.apply_mask_dev(torch.ones(2 * n, 1, h, 4 * h, dtype=torch.float32, device=_dev()), "second")
    sums, _, cross, _ = completion.completion_loss_dev(f, complete, label, mask, None, S=15)
    want = completion.completion_scalars(sums.cpu().numpy(), cross.cpu().numpy(), h, 4 * h)
    rng = np.random.RandomState(9)
    dc = descriptor.dense_correspondences(st["depth"], sub["R"].reshape(2 * n, 4, 4), "suncg", rng)
    completion.perturbed_poses(np.stack([sub["R"][b, 1] @ np.linalg.inv(sub["R"][b, 0]) for b in range(n)]), rng)      # (the draws in between)
    fl, lp, ln = completion.contrast_loss(f, pipe.feat_off, 32, dc, rng)
    got = eval_runs["f32"]["type0"]
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-13), k
    assert got["loss_fl_pos"] == pytest.approx(lp, rel=1e-13) and got["loss_fl_neg"] == pytest.approx(ln, rel=1e-13)


def test_bf16x6_is_closer_to_f32_than_f16_on_depth(eval_runs):
    """The split-precision mode must move the depth loss less than plain f16 does, on both input types."""
    for t in ("type0", "type1"):
        ref = eval_runs["f32"][t]["errG_d"]
        d6, d16 = abs(eval_runs["bf16x6"][t]["errG_d"] - ref), abs(eval_runs["f16"][t]["errG_d"] - ref)
        print(f"{t}: errG_d f32 {ref:.9g}; |bf16x6 - f32| {d6:.3e}; |f16 - f32| {d16:.3e}")
        log("completion_precision_order", type=t, errG_d=ref, bf16x6=d6, f16=d16)
        assert d6 < d16, (t, d6, d16)


def test_evaluation_completion_eval_prints_one_json_line(capsys):
    from relativepose_amd import evaluation
    evaluation.main(["--completion-eval", "--dataset", "scannet", "--pairs", "2", "--batch", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["metric"] == "completion_loss" and r["pairs"] == 2 and r["dataset"] == "scannet" and {"type0", "type1", "seconds"} <= set(r)
    assert all(np.isfinite(v) for v in _numbers(r))
    log("completion_eval_cli", **{k: v for k, v in r.items() if not isinstance(v, dict)})
