"""GPU: SCNet's unsplit deconv4 (three-piece bf16 modes: the split rule leaves it at ksplit = 1) on the phase strip kernel's direct-store
epilogue (the default) against conv_igemm_kernel<2, 2, 2, 2> (`_lib.tuning(deconv_strip=1)`, the plan of the parent commit).  Every
accumulator receives the same MFMAs in the same order and the fused BatchNorm records [tile][2 slots][Cout][2] are added in the implicit
GEMM's order (a lane's chain over 32-row blocks 2 wm, 2 wm + 1, lane pair, 0 + wm 0 + wm 1), so the raw layer outputs (taps D6, D5, D4),
everything behind deconv4's BatchNorm (tap D3: it sees the records through the scale / shift table) and the network output must agree in
every bit -- no tolerance anywhere.  Each case asserts through the plan read-out (SCNet.layer_kernel) that the default arm ran the strip
kernel unsplit (ksplit = 1, direct stores) and the knob arm another kernel.

The internal resolution is fixed at 224: with 2 images a phase of deconv4 has 1568 = 12 x 128 + 32 rows (a ragged last tile, one
BatchNorm group: slot 1 of every record is zero); with 6 images the group boundaries at multiples of 1568 rows fall inside tiles, so
both slots of a record are live, and both sources of the skip concatenation are read.

deconv6 (7 x 7 input grid: a 128-row tile spans three BatchNorm groups) is not on the strip kernel in any mode; a test pins that through
the read-out instead of comparing an arm with itself."""
from types import SimpleNamespace

import pytest

from gpu_util import log
from relativepose_amd import _lib, weights

pytestmark = pytest.mark.gpu

STRIP, IGEMM = 0, 1
TAPS = ("D6", "D5", "D4", "D3")


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
        return (y,) + tuple(net.read_tap(t).clone() for t in TAPS)


def assert_same(got, ref, what):
    import torch
    for name, a, b in zip(("output",) + TAPS, got, ref):
        assert torch.isfinite(b).all(), (what, name)
        assert torch.equal(a, b), (what, name, float((a - b).abs().max()))


SPLITK, DIRECT = 1, 2          # SCNet.layer_kernel: deconv_strip_kernel as a split-K launch / unsplit with direct stores


def assert_arms_differ(net, n, launch=DIRECT, layer="deconv4"):
    """The default arm runs `layer` on deconv_strip_kernel in the launch form named (DIRECT: ksplit = 1, the epilogue under test), the knob
    arm runs another kernel, and the context manager put the knob back."""
    assert net.layer_kernel(layer, n) == launch, (layer, n, net.layer_kernel(layer, n), "default arm")
    with _lib.tuning(deconv_strip=IGEMM):
        assert net.layer_kernel(layer, n) == 0, (layer, n, "knob arm is on the strip kernel")
    # (the library has no getter: relpose_set_tuning returns the value it replaces, i.e. what _lib.tuning left behind)
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["deconv_strip"], 0) == 0


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9"])
def test_direct_deconv4_is_bitwise_the_implicit_gemm(prec, n):
    import torch
    net = make_net(prec)
    x = torch.randn(n, 16, 160, 640, generator=torch.Generator().manual_seed(400 + n)).cuda()
    ref = forward_taps(net, IGEMM, x)
    got = forward_taps(net, STRIP, x)
    assert_arms_differ(net, n)
    assert ref[3].shape == (n, 56, 56, 128) and ref[4].shape == (n, 112, 112, 320)
    assert float(ref[3].abs().max()) > 0 and float(ref[4].abs().max()) > 0
    assert_same(got, ref, (prec, n))
    log("deconv_strip_direct_bitwise", prec=prec, images=n, bitwise=True)


def test_direct_deconv4_single_source():
    """skipLayer = 0: the decoder chain without the second source."""
    import torch
    net = make_net("bf16x6", skip=0)
    x = torch.randn(6, 16, 160, 640, generator=torch.Generator().manual_seed(411)).cuda()
    assert_arms_differ(net, 6)
    assert_same(forward_taps(net, STRIP, x), forward_taps(net, IGEMM, x), "skipLayer=0")


def test_direct_deconv4_in_zero_warp_and_self_cached_plans():
    """The level-0 and self-cached plans run the same deconv4 launch: each is bitwise the full plan's forward of the same input, and
    bitwise the same plan on the implicit-GEMM arm."""
    import torch
    net = make_net("bf16x6")
    gen = torch.Generator().manual_seed(421)
    xa = torch.randn(6, 16, 160, 640, generator=gen).cuda()
    xb = torch.randn(6, 16, 160, 640, generator=gen).cuda()
    x0 = xa.clone(); x0[:, 8:] = 0
    x1 = xa.clone(); x1[:, 8:] = xb[:, 8:]
    assert_arms_differ(net, 6)
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


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_split_modes_keep_deconv4_on_the_split_k_strip_launch(prec):
    """The modes whose split rule cuts deconv4 in two never reach the direct epilogue; the strip kernel still has the layer."""
    net = make_net(prec)
    assert_arms_differ(net, 6, SPLITK)


@pytest.mark.parametrize("n", [2, 12])
@pytest.mark.parametrize("prec", ["f32", "bf16x6", "f16x3"])
def test_deconv6_stays_on_the_implicit_gemm(prec, n):
    """deconv6's 7 x 7 grid puts three BatchNorm groups of 98 rows into a 128-row tile (12 images: rows 384-511 lie in groups 3, 4 and
    5); the strip kernel keeps the scale / shift of two.  A path for a third group was built and dropped (it spilled registers in the
    16-bit instantiations: DESIGN.md), so the layer deliberately stays on conv_igemm_kernel in every mode, whatever the knob -- asserted
    through the read-out; comparing the arms would compare conv_igemm_kernel with itself."""
    net = make_net(prec)
    for sel in (STRIP, IGEMM):
        with _lib.tuning(deconv_strip=sel):
            assert not net.layer_on_strip_kernel("deconv6", n), (prec, n, sel)


def test_read_out_knows_the_other_layers():
    """deconv7 (4 x 4 grid: five groups per tile) is never on the strip kernel; an unknown layer is an error, not a 'no'."""
    net = make_net("bf16x6")
    assert net.layer_kernel("deconv5", 6) == SPLITK and net.layer_kernel("deconv4", 6) == DIRECT and net.layer_kernel("deconv7", 6) == 0
    with pytest.raises(KeyError):
        net.layer_on_strip_kernel("deconv99", 6)
