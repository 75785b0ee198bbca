"""GPU: the streamed heads kernel (heads_kernel: coalesced loads and stores through LDS, the default) against the lane-per-pixel
kernel it replaced (heads_lanepix_kernel, `_lib.tuning(heads_kernel=1)`): the same arithmetic in the same order, so every bit of
the returned output and of the raw 224 x 224 head outputs (tap OUT) must agree -- no tolerance anywhere.

Plans: plain forward, zero-warp forward, a tagged level-0 forward followed by two self-cached forwards (the level-0 forward's kernel
WRITES the 12-float-per-pixel snapshot of the rgb / n / d skip halves, the cached forwards' kernel READS it: the two kernels share that
layout, so they are also crossed, snapshot written by one and read by the other, both ways round), the pose-outputs plan alone and on
a cached forward."""
from types import SimpleNamespace

import pytest

from gpu_util import log
from relativepose_amd import _lib, weights

pytestmark = pytest.mark.gpu

STREAMED, LANEPIX = 0, 1


def make_net(S, tanh, prec):
    from relativepose_amd.model import SCNet
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(11 + S + tanh, S))
    net.set_precision(prec)
    return net


def run_plans(net, x0, x1, x2, fill, read):
    """Every plan once: the level-0 forward that fills the self-stream cache (and the heads' snapshot) on kernel `fill`, everything else
    on kernel `read`.  Returns [(plan, output, OUT tap)]."""
    res = []

    def fwd(plan, sel, x, **kw):
        with _lib.tuning(heads_kernel=sel):
            y = net.forward(x, **kw).clone()
            res.append((plan, y, net.read_tap("OUT").clone()))

    fwd("plain", read, x1)
    fwd("zero_warp", read, x0, zero_warp=True)
    tag = net.new_self_tag()
    fwd("level0_tagged", fill, x0, zero_warp=True, self_tag=tag)
    fwd("cached_1", read, x1, self_tag=tag)
    fwd("cached_2", read, x2, self_tag=tag)
    fwd("pose", read, x1, outputs="pose")
    tag = net.new_self_tag()
    fwd("full_tagged", fill, x1, self_tag=tag)
    fwd("cached_pose", read, x2, outputs="pose", self_tag=tag)
    return res


@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("tanh", [0, 1])
@pytest.mark.parametrize("S", [15, 21])
def test_streamed_heads_are_bitwise_the_lane_per_pixel_heads(S, tanh, n, prec):
    import torch
    lib = _lib.lib()
    net = make_net(S, tanh, prec)
    gen = torch.Generator().manual_seed(1000 + 7 * S + n)
    xa = torch.randn(n, 16, 160, 640, generator=gen).cuda()
    xb = torch.randn(n, 16, 160, 640, generator=gen).cuda()
    x0 = xa.clone(); x0[:, 8:] = 0                     # level 0: zero warp
    x1 = xa                                            # levels 1, 2: the same own views, two warped views
    x2 = xa.clone(); x2[:, 8:] = xb[:, 8:]
    try:
        ref = run_plans(net, x0, x1, x2, LANEPIX, LANEPIX)
        for fill, read in ((STREAMED, STREAMED), (STREAMED, LANEPIX), (LANEPIX, STREAMED)):
            got = run_plans(net, x0, x1, x2, fill, read)
            for (plan, y, out), (rplan, ry, rout) in zip(got, ref):
                assert plan == rplan
                assert torch.isfinite(ry).all(), plan
                assert torch.equal(y, ry), (plan, "output", fill, read)
                assert torch.equal(out, rout), (plan, "OUT", fill, read)
    finally:
        # (the context manager restores the knob whatever happens; this reads it back)
        assert lib.relpose_set_tuning(_lib.TUNE_KEYS["heads_kernel"], 0) == 0
    log("heads_stream_bitwise", S=S, tanh=tanh, images=n, prec=prec, plans=len(ref), bitwise=True)


def test_heads_knob_switches_kernels_within_one_process():
    """The knob is read at every launch: the output under heads_kernel=1 and after it are both the default's (the two kernels agree), and the
    knob is back at 0 after the block."""
    import torch
    net = make_net(15, 1, "bf16x6")
    x = torch.randn(2, 16, 160, 640, generator=torch.Generator().manual_seed(5)).cuda()
    y0 = net.forward(x).clone()
    with _lib.tuning(heads_kernel=1):
        y1 = net.forward(x).clone()
    y2 = net.forward(x).clone()
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["heads_kernel"], 0) == 0
