"""GPU: SCNet's deconv4 / deconv5 on the phase strip kernel (deconv_strip_kernel, the default) against the implicit-GEMM kernel they ran on
(conv_igemm_kernel with the same K split, `_lib.tuning(deconv_strip=1)`).  Both kernels feed every accumulator the same MFMAs in the
same order (chunk outer, tap inner, slices cut at the same k-tiles) and leave their partial sums to the same reduce pass, so the raw
layer outputs (taps D5, D4) and the network output must agree in every bit -- no tolerance anywhere.

The internal resolution is fixed at 224, so small batches reach every edge: with 2 images a phase has 1568 = 12 x 128 + 32 rows on
deconv4's grid (a ragged last tile); with 6 images the BatchNorm group boundaries fall inside tiles on both grids (1568 / 128 = 12.25
tiles per group on deconv4, 392 / 128 = 3.06 on deconv5), so tiles cross an image boundary and two BatchNorm groups, and both sources
of the skip concatenation are read."""
from types import SimpleNamespace

import pytest

from gpu_util import log
from relativepose_amd import _lib, weights

pytestmark = pytest.mark.gpu

STRIP, IGEMM = 0, 1


def make_net(prec, skip=1, S=15):
    from relativepose_amd.model import SCNet
    otype = "rgbdnsf" if skip else "sf"          # (without skip connections the reference can only build the s / f heads)
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=skip, outputType=otype, snumclass=S))
    net.load_state_dict(weights.make_state_dict(23 + S, S, 1, skip, otype))
    net.set_precision(prec)
    return net


def forward_taps(net, sel, x, **kw):
    with _lib.tuning(deconv_strip=sel):
        y = net.forward(x, **kw).clone()
        return y, net.read_tap("D5").clone(), net.read_tap("D4").clone()


def assert_same(got, ref, what):
    import torch
    for name, a, b in zip(("output", "D5", "D4"), got, ref):
        assert torch.isfinite(b).all(), (what, name)
        assert torch.equal(a, b), (what, name, float((a - b).abs().max()))


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["f32", "bf16x6", "f16x3"])
def test_strip_deconvs_are_bitwise_the_implicit_gemm(prec, n):
    import torch
    net = make_net(prec)
    x = torch.randn(n, 16, 160, 640, generator=torch.Generator().manual_seed(300 + n)).cuda()
    ref = forward_taps(net, IGEMM, x)
    got = forward_taps(net, STRIP, x)
    assert ref[1].shape == (n, 28, 28, 256) and ref[2].shape == (n, 56, 56, 128)
    assert float(ref[1].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    assert_same(got, ref, (prec, n))
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["deconv_strip"], 0) == 0
    log("deconv_strip_bitwise", prec=prec, images=n, bitwise=True)


def test_strip_deconvs_single_source():
    """skipLayer = 0: the decoder chain without the second source."""
    import torch
    net = make_net("bf16x6", skip=0)
    x = torch.randn(6, 16, 160, 640, generator=torch.Generator().manual_seed(311)).cuda()
    assert_same(forward_taps(net, STRIP, x), forward_taps(net, IGEMM, x), "skipLayer=0")


def test_strip_deconvs_in_zero_warp_and_self_cached_plans():
    """The level-0 and self-cached plans run the same deconv launches: each is bitwise the full plan's forward of the same input, and
    bitwise the same plan on the implicit-GEMM arm."""
    import torch
    net = make_net("bf16x6")
    gen = torch.Generator().manual_seed(321)
    xa = torch.randn(6, 16, 160, 640, generator=gen).cuda()
    xb = torch.randn(6, 16, 160, 640, generator=gen).cuda()
    x0 = xa.clone(); x0[:, 8:] = 0
    x1 = xa.clone(); x1[:, 8:] = xb[:, 8:]
    res = {}
    for sel in (IGEMM, STRIP):
        full0, full1 = forward_taps(net, sel, x0), forward_taps(net, sel, x1)
        zw = forward_taps(net, sel, x0, zero_warp=True)
        tag = net.new_self_tag()
        lvl0 = forward_taps(net, sel, x0, zero_warp=True, self_tag=tag)
        cached = forward_taps(net, sel, x1, self_tag=tag)
        assert_same(zw, full0, (sel, "zero_warp"))
        assert_same(lvl0, full0, (sel, "level0_tagged"))
        assert_same(cached, full1, (sel, "self_cached"))
        res[sel] = (full0, full1)
    for a, b in zip(res[STRIP], res[IGEMM]):
        assert_same(a, b, "arms")


def test_deconv_strip_knob_switches_kernels_within_one_process():
    """The knob is part of the plan key: a plan built under one value is not used under another, the outputs under deconv_strip=1 and
    after it are both the default's, and the knob is back at 0 after the block."""
    import torch
    net = make_net("bf16x6")
    x = torch.randn(2, 16, 160, 640, generator=torch.Generator().manual_seed(5)).cuda()
    y0 = net.forward(x).clone()
    with _lib.tuning(deconv_strip=1):
        y1 = net.forward(x).clone()
    y2 = net.forward(x).clone()
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["deconv_strip"], 0) == 0
