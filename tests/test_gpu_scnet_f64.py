"""GPU: every SCNet layer, head and resize in every precision mode, teacher-forced against the float64 reference (tests/scnet_f64.py).

Each layer's output tap is compared with that one layer recomputed in float64 from the kernel's own input taps, normalised per element
by the layer's magnitude, and held to its mode's bound (scnet_f64.MODE_BOUNDS, derived in tests/test_scnet_f64_cpu.py); conv1, the fused
heads and both resizes are fp32 kernels in every mode and get the f32-class bound.  The 224 / 112 / 56-row layers and the heads are
checked on scnet_f64.rows_subset() rows (all columns, both images; every layer and head is checked) to keep the float64 CPU work of the
file within a few minutes.  Every (case, mode, stage) value goes to the parity log."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import scnet_f64 as R
from cases import SCNET_CASES, SCNET_VARIANT_CASES
from gpu_util import log
from relativepose_amd import weights
from test_oracle_golden import oracle_scnet_input
from test_scnet_f64_cpu import S_CASES

pytestmark = pytest.mark.gpu

MODES = ("f32", "bf16x9", "bf16x6", "f16x3", "bf16x3", "f16")
TAPS = ("X0",) + tuple(R.TAP_MAP) + ("OUT",)
U = R.U


def make_net(case, prec):
    from relativepose_amd.model import SCNet
    tag, S, tanh, seed, ds, mm, bn, skip, otype = case
    sd = weights.make_state_dict(seed, S, bn, skip, otype)
    net = SCNet(SimpleNamespace(batchnorm=bn, useTanh=tanh, skipLayer=skip, outputType=otype, snumclass=S))
    net.load_state_dict(sd)
    net.set_precision(prec)
    return net, sd


def read_taps(net, pairs):
    """{pair: {buffer: [2,H,H,C] numpy}} -- each tap is sliced to the pairs on the device before it is copied."""
    out = {p: {} for p in pairs}
    for b in TAPS:
        t = net.read_tap(b)
        for p in pairs:
            out[p][b] = t[2 * p:2 * p + 2].cpu().numpy()
        del t
    return out


def bound(mode, r, S):
    """(max, rms) bound of one check: the mode's bound for the conv stack, the f32-class bound for the fp32 kernels (conv1, resizes and the
    fused heads of S = 15 / 21; other S run the heads as an implicit-GEMM group in the mode's arithmetic)."""
    if r["stage"] in ("resize_in", "resize_out") or r["layer"].startswith("conv1"):
        return R.F32_CLASS
    if r["stage"] == "head" and S in (15, 21):
        return R.F32_CLASS
    return R.MODE_BOUNDS[mode]


def check(net, sd, case, mode, x, y, taps, what):
    """The float64 check of one image pair; logs every value; returns the failures."""
    tag, S, tanh, seed, ds, mm, bn, skip, otype = case
    ref = R.F64Reference(sd, S, tanh, bn, skip, otype)
    t0 = time.time()
    res = R.check_pair(ref, taps, x, y, subset=True)
    secs = time.time() - t0
    bad = []
    for r in res:
        bmax, brms = bound(mode, r, S)
        log("scnet_f64", case=what, mode=mode, stage=r["stage"], buffer=r["buffer"], layer=r["layer"], call=r["call"], rows=r["rows"],
            max_u=r["max"] / U, rms_u=r["rms"] / U, bound_max_u=bmax / U, bound_rms_u=brms / U)
        if not (r["max"] <= bmax and r["rms"] <= brms):
            bad.append((r["layer"], r["call"], r["max"] / U, r["rms"] / U))
    log("scnet_f64_pair", case=what, mode=mode, checks=len(res), f64_seconds=secs, worst_max_u=max(r["max"] for r in res) / U,
        worst_rms_u=max(r["rms"] for r in res) / U, failures=len(bad))
    return bad, ref


def forward_and_check(case, mode, what, scale=1.0):
    import torch
    net, sd = make_net(case, mode)
    x = oracle_scnet_input(500 + case[3], case[4], case[5])
    if scale != 1.0:
        x = (x * np.float32(scale)).astype(np.float32)
    y = net(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    taps = read_taps(net, [0])[0]
    bad, ref = check(net, sd, case, mode, x, y.cpu().numpy(), taps, what)
    return bad, ref, taps


FULL_CASES = [c + (1, 1, "rgbdnsf") for c in SCNET_CASES]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FULL_CASES, ids=[c[0] for c in FULL_CASES])
def test_scnet_every_layer_vs_float64(case, mode):
    bad, _, _ = forward_and_check(case, mode, case[0])
    assert not bad, bad


VARIANT_RUNS = [(c, m) for c in SCNET_VARIANT_CASES + S_CASES for m in ("f32", "bf16x6")] + \
               [(SCNET_VARIANT_CASES[0], m) for m in ("f16x3", "bf16x3")]


@pytest.mark.parametrize("case,mode", VARIANT_RUNS, ids=[f"{c[0]}-{m}" for c, m in VARIANT_RUNS])
def test_scnet_variants_every_layer_vs_float64(case, mode):
    """The constructor variants (batchnorm=0: conv bias through the loader's {scale, shift} table; skipLayer=0; head subsets) and the
    generic heads path: snumclass 13 (one implicit-GEMM heads group) and 40 (the semantic head's cout_pad is 64, the others' 32)."""
    bad, _, _ = forward_and_check(case, mode, case[0])
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale_log2", [-12, 12])
def test_scnet_bn0_magnitude_edge(scale_log2, mode):
    """batchnorm=0: nothing rescales activations between layers, and the fp16 modes convert them to float16 unscaled.  With the input
    scaled by 2^-12 / 2^12 every mode must stay finite and within its bound; the largest activation a 16-bit mode converts is logged
    (measured on the oracle: about 0.24 at 2^-12 and 7.9e3 at 2^12, below float16's 65504)."""
    case = SCNET_VARIANT_CASES[0]
    bad, ref, taps = forward_and_check(case, mode, f"bn0*2^{scale_log2}", 2.0 ** scale_log2)
    amax = ref.max_activation(taps)
    log("scnet_f64_magnitude", case=f"bn0*2^{scale_log2}", mode=mode, max_activation=amax, finite=bool(np.isfinite(taps["OUT"]).all()))
    assert np.isfinite(taps["OUT"]).all()
    assert not bad, bad


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3"])
def test_scnet_production_batch_pairs_are_the_pair_forwards(mode):
    """64 images (the bench's batch; bf16x6 = configs 1-3, f16x3 = configs[4]): the taps and outputs of pairs 0, 17 and 31 equal, bit for
    bit, n = 2 forwards of the same pairs -- so the n = 2 float64 results hold for the batch -- and pair 31 passes the float64 check."""
    import torch
    case = FULL_CASES[0]
    net, sd = make_net(case, mode)
    xs = [oracle_scnet_input(500 + s, case[4], case[5]) for s in (case[3], 20, 21)]
    x = np.concatenate([xs[p % 3] for p in range(32)])
    xd = torch.from_numpy(x).cuda()
    y = net(xd).clone()
    torch.cuda.synchronize()
    pairs = (0, 17, 31)
    big = read_taps(net, pairs)
    yb = {p: y[2 * p:2 * p + 2].cpu().numpy() for p in pairs}
    del y
    for p in pairs:
        y2 = net(xd[2 * p:2 * p + 2].contiguous()).cpu().numpy()
        small = read_taps(net, [0])[0]
        assert np.array_equal(y2, yb[p]), p
        for b in TAPS:
            assert np.array_equal(small[b], big[p][b]), (p, b)
    bad, _ = check(net, sd, case, mode, x[62:64], yb[31], big[31], f"{case[0]}/n64/pair31")
    log("scnet_f64_batch", mode=mode, images=64, pairs=list(pairs), bitwise=True)
    assert not bad, bad
