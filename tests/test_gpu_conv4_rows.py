"""GPU: conv4's row lists (`_lib.tuning(conv4_rows=0)`, the default; 2 = the row-list launch for every slice) against conv4_rows=1, which
runs every row on the strip kernel like the parent commit.  A dropped row's partial sums are read from a computed row of its edge class
and a listed row is computed by the same MFMAs in the same order, so the network output and the raw layer outputs A4 and D3 must agree in
every bit -- compared as int32 bit patterns, no tolerance anywhere.  Every default-arm forward's read-out (SCNet.conv4_rows) must equal
the numpy model (tests/conv4_rows_model.py) on the X0 the GPU itself resized, so no case can pass by skipping nothing -- or too much.

conv4's partial sums live in a workspace region no other layer writes, and the tests share one workspace per batch size.  So every list-arm
forward is preceded by `scrub`: a knob-1 forward of an unrelated dense input on the same workspace, which overwrites every row of every
slice with wrong values.  A listed row the row-list launch failed to write, or a map entry that points at a row nobody computed, then
reads those values and shows as a mismatch (a self-cached forward is not scrubbed: it must find what its tagged level 0 left, and that
level 0 was scrubbed).

The internal grid is 224 x 224 whatever the input: 2 images = one BatchNorm group, 6 images = three."""
import numpy as np
import pytest

import conv4_rows_model as M
from gpu_util import log
from relativepose_amd import _lib
from test_gpu_zero_tiles import H, W, make_net, masked_input

pytestmark = pytest.mark.gpu

TAPS = ("A4", "D3")
LISTS, STRIP, ALL_LISTED = 0, 1, 2


_scrub_x = {}


def scrub(net, n):
    """Overwrite conv4's partial sums (all six slices, every row) on the workspace of n-image forwards with those of an unrelated input."""
    import torch
    if n not in _scrub_x:
        _scrub_x[n] = 3.0 * torch.randn(n, 16, H, W, generator=torch.Generator().manual_seed(977 + n)).cuda()
    with _lib.tuning(conv4_rows=STRIP):
        net.forward(_scrub_x[n])


def run(net, sel, x, plan="full", **kw):
    """(output, A4, D3) as int32 bit patterns and the read-out, checked against the model for the X0 of this forward."""
    import torch
    if sel != STRIP and plan != "self_cached":
        scrub(net, x.shape[0])
    with _lib.tuning(conv4_rows=sel):
        y = net.forward(x, **kw).clone()
        taps = [net.read_tap(t).clone() for t in TAPS]
        got = net.conv4_rows()
        x0 = net.read_tap("X0").cpu().numpy()
    if sel == STRIP:
        assert got is None
    else:
        want = M.counts(x0, plan, sel)
        assert got == want, (plan, sel, got, want)
    return [t.view(torch.int32) for t in [y] + taps], got


def assert_same(a, b, what):
    import torch
    for name, u, v in zip(("output",) + TAPS, a, b):
        assert torch.equal(u, v), (what, name, int((u != v).sum()))


def assert_finite(r, what):
    import torch
    assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in r), what


def dense(n, seed):
    import torch
    return torch.randn(n, 16, H, W, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9", "f32", "f16x3"])
def test_masked_views_are_bitwise_and_counted(prec, n):
    net = make_net(prec)
    for dataset, mask in (("suncg", "second"), ("scannet", "kinect")):
        x = masked_input(n, dataset, mask, 600 + n)
        ref, _ = run(net, STRIP, x)
        got, c = run(net, LISTS, x)
        every, c2 = run(net, ALL_LISTED, x)
        assert_finite(ref, (prec, n, mask))
        assert all(d > 0 and lp for _, d, lp in c), c                  # these inputs have redundant rows in every slice
        assert c2 == c
        assert_same(got, ref, (prec, n, mask, "lists"))
        assert_same(every, ref, (prec, n, mask, "every slice listed"))
        log("conv4_rows_bitwise", prec=prec, images=n, mask=mask, rows=c)


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9", "f32", "f16x3"])
def test_dense_input_every_row_listed(prec, n):
    """Nothing is redundant: under knob 2 every row goes through the row-list launch (the test of its K order), under knob 0 every slice
    stays on the strip kernel."""
    net = make_net(prec)
    x = dense(n, 610 + n)
    ref, _ = run(net, STRIP, x)
    every, c2 = run(net, ALL_LISTED, x)
    got, c = run(net, LISTS, x)
    assert c2 == [(n * 784, 0, True)] * 6 and c == [(n * 784, 0, False)] * 6
    assert_finite(ref, (prec, n))
    assert_same(every, ref, (prec, n, "every row listed"))
    assert_same(got, ref, (prec, n, "dense, default"))


@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
def test_zero_warp_and_self_cached_plans(prec):
    """Each plan is bitwise the full plan's forward of the same input; a second tagged level 0 with other self views on the same workspace,
    then its self-cached forward, would show a stale self-slice map."""
    net = make_net(prec)
    xa = masked_input(6, "suncg", "second", 621)
    xb = masked_input(6, "scannet", "kinect", 622)
    for sel in (LISTS, ALL_LISTED):
        for x1 in (xa, xb):
            x0 = x1.clone(); x0[:, 8:] = 0
            full0, _ = run(net, STRIP, x0)
            full1, _ = run(net, STRIP, x1)
            zw, cz = run(net, sel, x0, "zero_warp", zero_warp=True)
            tag = net.new_self_tag()
            lvl0, c0 = run(net, sel, x0, "zero_warp", zero_warp=True, self_tag=tag)
            cached, c1 = run(net, sel, x1, "self_cached", self_tag=tag)
            assert cz == c0 and all(c0[q] == (9, 2 * 784 - 9, True) for q in (1, 3, 5)), c0
            assert all(c1[q] == (0, 0, False) for q in (0, 2, 4)) and all(c1[q][1] > 0 for q in (1, 3, 5)), c1
            assert_same(zw, full0, (prec, sel, "zero_warp"))
            assert_same(lvl0, full0, (prec, sel, "level0_tagged"))
            assert_same(cached, full1, (prec, sel, "self_cached"))
            assert not bool((cached[1] == lvl0[1]).all())              # the warped channels did change A4


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x9", "f32", "f16x3"])
def test_more_than_two_groups_in_128_listed_rows(prec):
    """All-zero input but a short run of pixels per image (wide enough for the resize to sample it): every (group, slice) lists its nine
    representatives and a patch of at most 4 x 4 rows per image, so the three groups' lists together are shorter than one 128-row tile."""
    import torch
    net = make_net(prec)
    x = torch.zeros(6, 16, H, W)
    for i in range(6):
        x[i, :, 20 + 20 * i, 50 + 90 * i:54 + 90 * i] = 1.0 + i
    x = x.cuda()
    ref, _ = run(net, STRIP, x)
    got, c = run(net, LISTS, x)
    every, c2 = run(net, ALL_LISTED, x)
    assert c == c2 and all(3 * 9 + 6 <= r <= 3 * 9 + 6 * 16 and lp for r, _, lp in c), c
    assert_finite(ref, prec)
    assert_same(got, ref, (prec, "lists"))
    assert_same(every, ref, (prec, "every slice listed"))


def test_single_value_probes():
    """One value per image (three pixels wide, so that the resize samples it) at input pixels whose resized footprint lies on both sides
    of an occupancy block boundary, and at the image corners; the channels walk every stream."""
    import torch
    net = make_net("bf16x6")
    edge = lambda r, size: int(round((r + 0.5) * size / 224 - 0.5))
    ys = [0, edge(7, H), edge(8, H), edge(15, H), edge(16, H), edge(216, H), H - 1]
    xs = [0, edge(7, W), edge(8, W), edge(15, W), edge(16, W), edge(216, W), W - 1]
    chans = [0, 3, 6, 7, 8, 12, 14, 15]
    for rnd in range(3):
        x = torch.zeros(6, 16, H, W)
        for i in range(6):
            k = 6 * rnd + i
            xx = xs[(5 * k + rnd) % 7]
            x[i, chans[k % len(chans)], ys[(3 * k) % 7], max(xx - 1, 0):xx + 2] = 1.0
        x = x.cuda()
        ref, _ = run(net, STRIP, x)
        got, c = run(net, LISTS, x)
        assert_finite(ref, "probe")
        assert all(lp and d > 6 * 784 - 3 * 9 - 6 * 16 for _, d, lp in c), c          # nine representatives per group, a few rows per probe
        assert_same(got, ref, ("probe", rnd))


def test_nonfinite_value_in_one_stream():
    """One Inf in stream 3 of group 1: nothing of that group and stream is redundant, and the stream's slice stays on the strip kernel (its
    NaN rows keep the kernel that has always computed them); the other slices drop what they dropped before."""
    net = make_net("bf16x6")
    x = masked_input(6, "suncg", "second", 641)
    clean = run(net, LISTS, x)[1]
    x[3, 11, 80, 300] = float("inf")                                   # channel 11: stream 3 (normals, warped view)
    ref, _ = run(net, STRIP, x)
    for sel in (LISTS, ALL_LISTED):
        got, c = run(net, sel, x)
        assert c[3] == (6 * 784, 0, False) and [c[q] for q in (0, 1, 2, 4, 5)] == [clean[q] for q in (0, 1, 2, 4, 5)], (c, clean)
        assert all(lp and d > 0 for _, d, lp in clean)
        assert_same(got, ref, ("inf", sel))


def test_knob_switches_within_a_process_and_is_restored():
    net = make_net("bf16x6")
    x = masked_input(2, "suncg", "second", 651)
    seen = []
    for sel in (LISTS, STRIP, ALL_LISTED, LISTS, STRIP):
        r, c = run(net, sel, x)
        seen.append((r, c))
    assert seen[0][1] == seen[3][1] and seen[1][1] is None and seen[4][1] is None and seen[0][1][0][1] > 0
    for r, _ in seen[1:]:
        assert_same(r, seen[0][0], "knob")
    # (the library has no getter: relpose_set_tuning returns the value it replaces, i.e. what _lib.tuning left behind)
    assert _lib.lib().relpose_set_tuning(_lib.TUNE_KEYS["conv4_rows"], 0) == 0
