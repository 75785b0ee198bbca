"""GPU: SCNet's zero-tile skipping (the default) against `_lib.tuning(zero_tiles=1)`, which computes every conv2 / conv3 patch like the
parent commit.  A dropped patch is a copy of a computed patch of its edge class (tile and BatchNorm record), so the network output and
the raw layer outputs A2, A3, A4, D3 must agree in every bit -- compared as int32 bit patterns (stricter than torch.equal: signed zeros,
and a NaN equals itself), no tolerance anywhere.  Every default-arm forward's read-out (SCNet.zero_tiles) must equal the counts of the
numpy model (tests/zero_tiles_model.py) on the X0 the GPU itself resized, so no case can pass by skipping nothing -- or too much.

The internal grid is 224 x 224 whatever the input: 2 images = one BatchNorm group, 6 images = three (representatives are per group; the
conv3 pair 24 of a group straddles its two images)."""
from types import SimpleNamespace

import numpy as np
import pytest

import zero_tiles_model as Z
from gpu_util import log
from relativepose_amd import _lib, synth, weights

pytestmark = pytest.mark.gpu

TAPS = ("A2", "A3", "A4", "D3")
SKIP, ALL = 0, 1
H, W = 160, 640
_nets = {}


def make_net(prec, skip=1, S=15):
    from relativepose_amd.model import SCNet
    key = (skip, S)
    if key not in _nets:
        otype = "rgbdnsf" if skip else "sf"
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=skip, outputType=otype, snumclass=S))
        net.load_state_dict(weights.make_state_dict(31 + S, S, 1, skip, otype))
        _nets[key] = net
    return _nets[key].set_precision(prec)


def masked_input(n, dataset, mask, seed):
    """[n, 16, 160, 640]: channels 0:8 the masked view (oracle build_view), 8:16 the partner view warped by a random rigid pose."""
    import torch
    from oracle import geom_oracle as G
    from relativepose_amd.util import warp_pairs_dev
    d = synth.make_pairs(n // 2, seed, dataset)
    x = np.zeros((n, 16, H, W), np.float32)
    for b in range(n // 2):
        for v in range(2):
            x[2 * b + v, :8] = G.build_view(d["rgb"][b, v], d["norm"][b, v], d["depth"][b, v], mask)[0][0]
    rs = np.random.RandomState(seed)
    pose = np.stack([synth.random_rigid(rs, 0.6, 0.5) for _ in range(n)])
    xd = torch.from_numpy(x).cuda()
    warp_pairs_dev(xd, torch.from_numpy(pose).cuda(), dataset)
    return xd


def run(net, sel, x, plan="full", **kw):
    """(output, A2, A3, A4, D3) as int32 bit patterns, the read-out, and what the model expects for the X0 of this forward."""
    import torch
    with _lib.tuning(zero_tiles=sel):
        y = net.forward(x, **kw).clone()
        taps = [net.read_tap(t).clone() for t in TAPS]
        got = net.zero_tiles()
        x0 = net.read_tap("X0").cpu().numpy()
    if plan == "zero_warp":          # the warped blocks of A2 / A3 are written for the first image pair only
        taps[0] = taps[0].view(*taps[0].shape[:3], 6, -1)[..., 0::2, :].contiguous()
        taps[1] = taps[1].view(*taps[1].shape[:3], 6, -1)[..., 0::2, :].contiguous()
    want = Z.counts(x0, plan, skip=(sel == SKIP))
    assert got == want, (plan, sel, got, want)
    return [t.view(torch.int32) for t in [y] + taps], got


def assert_same(a, b, what, names=("output",) + TAPS):
    import torch
    for name, u, v in zip(("output",) + TAPS, a, b):
        if name in names:
            assert torch.equal(u, v), (what, name, int((u != v).sum()))


def assert_finite(r, what):
    import torch
    assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in r), what


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9", "f32", "f16x3"])
def test_masked_views_are_bitwise_and_counted(prec, n):
    net = make_net(prec)
    for dataset, mask in (("suncg", "second"), ("scannet", "kinect")):
        x = masked_input(n, dataset, mask, 500 + n)
        ref, c_ref = run(net, ALL, x)
        got, c = run(net, SKIP, x)
        assert_finite(ref, (prec, n, mask))
        assert c_ref[2] == (6 * n * 49, 0) and c_ref[3] == (6 * n * 49 // 2, 0)
        assert c[2][1] > 0 and c[3][1] > 0, c                           # these inputs do have redundant patches in both layers
        assert_same(got, ref, (prec, n, mask))
        log("zero_tiles_bitwise", prec=prec, images=n, mask=mask, conv2=c[2], conv3=c[3])


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9", "f32", "f16x3"])
def test_zero_warp_and_self_cached_plans(prec):
    """Each plan is bitwise the full plan's forward of the same input (output, A4, D3: the level-0 plan leaves the warped blocks of A2 / A3
    to the first image pair) and bitwise itself on the knob arm."""
    net = make_net(prec)
    x1 = masked_input(6, "suncg", "second", 521)
    x0 = x1.clone(); x0[:, 8:] = 0
    res = {}
    for sel in (ALL, SKIP):
        full0, _ = run(net, sel, x0)
        full1, _ = run(net, sel, x1)
        zw, _ = run(net, sel, x0, "zero_warp", zero_warp=True)
        tag = net.new_self_tag()
        lvl0, c0 = run(net, sel, x0, "zero_warp", zero_warp=True, self_tag=tag)
        cached, c1 = run(net, sel, x1, "self_cached", self_tag=tag)
        far = ("output", "A4", "D3")
        assert_same(zw, full0, (prec, sel, "zero_warp"), far)
        assert_same(lvl0, full0, (prec, sel, "level0_tagged"), far)
        assert_same(cached, full1, (prec, sel, "self_cached"))
        res[sel] = (full0, full1, zw, lvl0, cached)
        if sel == SKIP:
            # level 0: the three warped members run on one image pair and keep their 9 class representatives (conv3: the pairs' class pairs)
            assert c0[2][1] > 3 * (98 - 9) and c1[2][1] > 0 and c1[3][1] > 0, (c0, c1)
    assert_finite(res[ALL][0] + res[ALL][1], prec)
    for a, b, what in zip(res[SKIP], res[ALL], ("full0", "full1", "zero_warp", "level0_tagged", "self_cached")):
        assert_same(a, b, (prec, "arms", what))


def test_dense_input_drops_nothing():
    import torch
    net = make_net("bf16x6")
    x = torch.randn(6, 16, H, W, generator=torch.Generator().manual_seed(531)).cuda()
    ref, _ = run(net, ALL, x)
    got, c = run(net, SKIP, x)
    assert c == {2: (6 * 6 * 49, 0), 3: (6 * 6 * 49 // 2, 0)}
    assert_same(got, ref, "dense")


def test_zero_warped_channels_without_the_flag():
    """The full plan on an input whose warped channels are zero: every warped patch but the representatives is a copy."""
    import torch
    net = make_net("bf16x6")
    x = torch.randn(6, 16, H, W, generator=torch.Generator().manual_seed(541)).cuda()
    x[:, 8:] = 0
    ref, _ = run(net, ALL, x)
    got, c = run(net, SKIP, x)
    pair_classes = len({(Z.edge_class(2 * u % 49), Z.edge_class((2 * u + 1) % 49)) for u in range(49)})
    assert c[2] == (3 * 6 * 49 + 3 * 3 * 9, 3 * 3 * (98 - 9)), c
    assert c[3] == (3 * 3 * 49 + 3 * 3 * pair_classes, 3 * 3 * (49 - pair_classes)), c
    assert_finite(ref, "zero warped")
    assert_same(got, ref, "zero warped")


def probe_pixels():
    """Input pixels whose resized footprint lies at the X0 rows / columns of the CPU probes: around the borders of patch 3's tested block
    range and exact fields, the patch corners, and the four image borders."""
    ys = sorted({0, H - 1} | {int(round((r + 0.5) * H / 224 - 0.5)) for r in (87, 88, 92, 94, 95, 129, 131, 135, 136)})
    xs = sorted({0, W - 1} | {int(round((c + 0.5) * W / 224 - 0.5)) for c in (87, 88, 92, 94, 95, 129, 131, 135, 136)})
    return [(y, x) for y in (ys[0], ys[2], ys[5], ys[-1]) for x in xs[::3]] + [(y, xs[4]) for y in ys]


@pytest.mark.parametrize("value", [1.0, -0.0, 1e-40, float("nan")])
def test_single_value_probes(value):
    """One value per image (six probes per forward), walking the probe pixels and the channels of every stream (depth 6 / 14 and mask
    7 / 15 included); the rest of the input is zero.  A NaN makes its BatchNorm group NaN: nothing of that group's stream is dropped and
    the bits still agree."""
    import torch
    net = make_net("bf16x6")
    px = probe_pixels()
    chans = [0, 3, 6, 7, 8, 12, 14, 15]
    for rnd in range(3):
        x = torch.zeros(6, 16, H, W)
        for i in range(6):
            y, xx = px[(6 * rnd + i) * 5 % len(px)]
            x[i, chans[(6 * rnd + i) % len(chans)], y, xx] = value
        x = x.cuda()
        ref, _ = run(net, ALL, x)
        got, c = run(net, SKIP, x)
        if value == 1.0:
            assert_finite(ref, "probe")
            assert 0 < c[2][1] < 6 * 6 * 49 - 3 * 6 * 9, c            # the probes' patches run, most others are copies
        assert_same(got, ref, ("probe", value, rnd))


def test_skip_layer_0_variant():
    net = make_net("bf16x6", skip=0)
    x = masked_input(6, "suncg", "second", 551)
    ref, _ = run(net, ALL, x)
    got, c = run(net, SKIP, x)
    assert c[2][1] > 0 and c[3][1] > 0
    assert_finite(ref, "skipLayer=0")
    assert_same(got, ref, "skipLayer=0")


def test_knob_switches_within_a_process_and_is_restored():
    net = make_net("bf16x6")
    x = masked_input(2, "suncg", "second", 561)
    seen = []
    for sel in (SKIP, ALL, SKIP, ALL):
        _, c = run(net, sel, x)
        seen.append(c)
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0][2][1] > 0 and seen[1][2][1] == 0 and seen[1][3][1] == 0
    assert sum(seen[0][2]) == sum(seen[1][2]) == 6 * 2 * 49
    # (the library has no getter: relpose_set_tuning returns the value it replaces, i.e. what _lib.tuning left behind)
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["zero_tiles"], 0) == 0
