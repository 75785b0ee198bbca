"""GPU: conv1's zero units and the occupancy words from the input resize (the default) against `_lib.tuning(conv1_zero=1)`, which runs the
separate occupancy pass and computes and stores every launched conv1 block like the parent commit.  Nothing is reordered: the network
output, the raw X0 / A1 / A2 and the occupancy words must agree in every bit -- compared as int32 bit patterns (signed zeros count, a NaN
equals itself), no tolerance anywhere.  A1 is compared WHOLE after every forward, blocks a plan did not launch included: what conv1 skips
must be in memory already, whatever ran before on the workspace.

Each arm runs its sequence on a workspace of its own (the state bytes describe one workspace's A1).  The default arm's read-out
(SCNet.conv1_zero) must equal what the occupancy words of that forward imply for the plan's launched units, so no case can pass by
skipping nothing -- or too much.  2 images = one BatchNorm group, 6 = three.

The sequence is A (masked), B (A's mask shifted by 40 columns), C (dense), A, A, a tagged zero-warp forward, two self-cached forwards.
The dense forward computes every unit and so clears every state byte: the A behind it has to STORE its zeros again (skipping there would
leave C's values in A1), and only the A after that one skips without a store -- hence two of them; B, right after A, already skips the
units that are zero in both."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import zero_tiles_model as Z
from gpu_util import log
from relativepose_amd import _lib, synth, weights

pytestmark = pytest.mark.gpu

TAPS = ("X0", "A1", "A2")
ZERO, KNOB = 0, 1
H, W = 160, 640
_nets = {}


def make_net(prec, S=15):
    from relativepose_amd.model import SCNet
    if S not in _nets:
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(31 + S, S, 1, 1, "rgbdnsf"))
        _nets[S] = net
    return _nets[S].set_precision(prec)


_inputs = {}


def masked_input(n, seed=600):
    """[n, 16, 160, 640]: channels 0:8 the masked view (oracle build_view), 8:16 the partner view warped by a random rigid pose."""
    import torch
    from oracle import geom_oracle as G
    from relativepose_amd.util import warp_pairs_dev
    if (n, seed) not in _inputs:
        d = synth.make_pairs(n // 2, seed, "suncg")
        x = np.zeros((n, 16, H, W), np.float32)
        for b in range(n // 2):
            for v in range(2):
                x[2 * b + v, :8] = G.build_view(d["rgb"][b, v], d["norm"][b, v], d["depth"][b, v], "second")[0][0]
        rs = np.random.RandomState(seed)
        pose = np.stack([synth.random_rigid(rs, 0.6, 0.5) for _ in range(n)])
        xd = torch.from_numpy(x).cuda()
        warp_pairs_dev(xd, torch.from_numpy(pose).cuda(), "suncg")
        _inputs[(n, seed)] = xd
    return _inputs[(n, seed)].clone()


def launched(plan, n):
    m = np.zeros((n, 6), bool)
    for q, nimg in Z.plan_members(plan, n):
        m[:nimg, q] = True
    return m


def zero_units(occ, plan):
    """occ [n, 6, 28] words -> how many launched (image, stream, tile) units have only clear bits (and no non-finite flag) in block rows
    by - 1 .. by + 1, block columns 4 tx - 1 .. 4 tx + 4."""
    n = occ.shape[0]
    m = launched(plan, n)
    cnt = 0
    for by in range(28):
        rows = occ[:, :, max(by - 1, 0):min(by + 2, 28)]
        bad = ((rows >> 31) & 1).any(2)
        for tx in range(7):
            lo, hi = max(4 * tx - 1, 0), min(4 * tx + 5, 28)
            mask = ((1 << hi) - 1) & ~((1 << lo) - 1)
            cnt += int((((rows & mask) == 0).all(2) & ~bad & m).sum())
    return cnt


def forward(net, sel, x, ws, plan="full", skips=None, **kw):
    """One forward under arm `sel` on workspace `ws`: ([output, X0, A1, A2] as int32, occupancy words, read-out).  The words must be those
    of the numpy model on the X0 the GPU resized, the read-out what they imply (skips=False: conv1 must not have skipped anything)."""
    import torch
    n = x.shape[0]
    with _lib.tuning(conv1_zero=sel):
        y = net.forward(x, ws_key=ws, **kw).clone()
        taps = [net.read_tap(t).clone() for t in TAPS]
        counts, occ_all = net.conv1_zero(occupancy=True)
    # a self-cached forward judges channels 8:16 only: nobody reads the self words
    streams = slice(1, None, 2) if plan == "self_cached" else slice(None)
    occ = occ_all[:, streams]
    want_occ, want_nf = Z.occupancy(taps[0].cpu().numpy())
    bits = (occ[..., None] >> np.arange(28)) & 1
    assert np.array_equal(bits.astype(bool), want_occ[:, streams]), (plan, sel, "occupancy bits")
    assert np.array_equal(((occ >> 31) & 1).any(2), want_nf[:, streams]), (plan, sel, "non-finite flags")
    units = int(launched(plan, n).sum()) * 196
    assert counts[0] == units, (plan, sel, counts, units)
    if sel == KNOB or skips is False:
        assert counts[1:] == (0, 0), (plan, counts)
    else:
        assert counts[1] + counts[2] == zero_units(occ_all, plan), (plan, counts)
    return [t.view(torch.int32) for t in [y] + taps], occ, counts


def assert_same(a, b, what):
    import torch
    for name, u, v in zip(("output",) + TAPS, a[0], b[0]):
        assert torch.equal(u, v), (what, name, int((u != v).sum()))
    assert np.array_equal(a[1], b[1]), (what, "occupancy words")


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
def test_stateful_sequence(prec, n):
    import torch
    net = make_net(prec)
    xa = masked_input(n)
    xb = torch.roll(xa, 40, dims=3)                               # tiles go zero -> non-zero and non-zero -> zero
    xc = torch.randn(n, 16, H, W, generator=torch.Generator().manual_seed(611)).cuda()
    x0 = xa.clone(); x0[:, 8:] = 0
    w1 = masked_input(n, 601); w1[:, :8] = xa[:, :8]
    w2 = torch.roll(w1, -56, dims=3); w2[:, :8] = xa[:, :8]
    zw_plan = "zero_warp" if n > 2 else "full"
    res = {}
    for sel in (ZERO, KNOB):
        ws = f"conv1_zero_{prec}_{n}_{sel}"
        tag = net.new_self_tag()
        seq = [("A", xa, "full", {}), ("B", xb, "full", {}), ("C dense", xc, "full", {}), ("A again", xa, "full", {}), ("A third", xa, "full", {}),
               ("zero warp", x0, zw_plan, dict(zero_warp=True, self_tag=tag)), ("cached 1", w1, "self_cached", dict(self_tag=tag)),
               ("cached 2", w2, "self_cached", dict(self_tag=tag))]
        res[sel] = [(name, forward(net, sel, x, ws, plan, **kw)) for name, x, plan, kw in seq]
    for (name, a), (_, b) in zip(res[ZERO], res[KNOB]):
        assert_same(a, b, (prec, n, name))
    c = {name: r[2] for name, r in res[ZERO]}
    assert c["A"][1] == 0 and c["A"][2] > 0, c                    # a fresh workspace: nothing is known to be zero yet
    assert c["B"][1] > 0 and c["B"][2] > 0, c                     # B: tiles zero in A and B are skipped, tiles that went zero are stored
    assert c["C dense"][1:] == (0, 0), c
    assert c["A again"][1] == 0 and c["A again"][2] == c["A"][2], c        # after the dense forward every zero has to be stored again
    assert c["A third"][2] == 0 and c["A third"][1] == c["A"][2], c        # ... and then none
    assert c["cached 2"][1] > 0, c
    log("conv1_zero_sequence", prec=prec, images=n, counts={k: list(v) for k, v in c.items()})


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
def test_signed_zeros_and_non_finite_values(prec, n):
    import torch
    net = make_net(prec)
    x = masked_input(n)
    checker = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 == 0).cuda()
    x = torch.where((x == 0) & checker, torch.full_like(x, -0.0), x)
    zero_px = (x[0] == 0).all(0).nonzero()                         # pixels of image 0 / 1 with zeros in all 16 channels
    ya, xa_ = [int(v) for v in zero_px[len(zero_px) // 3]]
    x[0, 9, ya, xa_] = float("nan")
    zero_px = (x[1] == 0).all(0).nonzero()
    yb, xb_ = [int(v) for v in zero_px[2 * len(zero_px) // 3]]
    x[1, 2, yb, xb_] = float("inf")
    res = {}
    for sel in (ZERO, KNOB):
        ws = f"conv1_zero_edge_{prec}_{n}_{sel}"
        res[sel] = [forward(net, sel, x, ws) for _ in range(2)]
    for i in range(2):
        assert_same(res[ZERO][i], res[KNOB][i], (prec, n, "signed zeros / NaN / Inf", i))
    assert res[ZERO][1][2][1] > 0, res[ZERO][1][2]                 # -0.0 is zero: units are skipped all the same
    assert (res[ZERO][0][1] >> 31).any()


def raw_forward(net, x, ws, gen):
    import torch
    n = x.shape[0]
    out = torch.empty(n, net.out_channels, H, W, dtype=torch.float32, device=x.device)
    a = _lib.ForwardArgs()
    a.struct_size = C.sizeof(_lib.ForwardArgs)
    a.flags = 0
    a.x, a.out = x.data_ptr(), out.data_ptr()
    a.n_images, a.H, a.W = n, H, W
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.stream = a.tail_stream = torch.cuda.current_stream().cuda_stream
    a.workspace_generation = gen
    _lib.check(_lib.lib().relpose_scnet_forward_ex(net.handle, C.byref(a)), "relpose_scnet_forward_ex")
    net._ws, net._ws_n = ws, n                                     # (read_tap / conv1_zero read the workspace of the last forward)
    taps = [net.read_tap(t).clone() for t in TAPS]
    return [t.view(torch.int32) for t in [out] + taps], net.conv1_zero()


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
def test_plan_for_another_n_on_the_same_workspace(prec, n):
    """One allocation, one generation, forwards of 8 - n and then n images on it: every offset inside the workspace moves, the state bytes
    of the new shape lie where something else was (the workspace starts as 0x01 bytes: 'known zero' everywhere, were it believed)."""
    import torch
    net = make_net(prec)
    other = 8 - n
    nbytes = max(_lib.lib().relpose_scnet_workspace_bytes(net.handle, k, H, W) for k in (n, other))
    xo, xn = masked_input(other, 602), masked_input(n)
    res = {}
    for sel in (ZERO, KNOB):
        ws = torch.full((nbytes,), 1, dtype=torch.uint8, device="cuda")
        gen = 1 << 40 | sel                                        # (names no allocation of SCNet._workspace)
        with _lib.tuning(conv1_zero=sel):
            res[sel] = [raw_forward(net, xo, ws, gen), raw_forward(net, xo, ws, gen), raw_forward(net, xn, ws, gen), raw_forward(net, xn, ws, gen),
                        raw_forward(net, xo, ws, gen)]
        net._ws = None
    for i, (a, b) in enumerate(zip(res[ZERO], res[KNOB])):
        for name, u, v in zip(("output",) + TAPS, a[0], b[0]):
            assert torch.equal(u, v), (prec, n, i, name, int((u != v).sum()))
        assert b[1][1:] == (0, 0)
    c = [r[1] for r in res[ZERO]]
    assert c[0][1] == 0 and c[1][1] > 0 and c[2][1] == 0 and c[3][1] > 0 and c[4][1] == 0, c


@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
def test_non_finite_conv1_weight_skips_nothing(prec, n):
    from relativepose_amd.model import SCNet
    sd = weights.make_state_dict(46, 15, 1, 1, "rgbdnsf")
    w = sd["conv1rgb.0.weight"].copy()
    w.reshape(-1)[5] = np.inf
    sd["conv1rgb.0.weight"] = w
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=15))
    net.load_state_dict(sd).set_precision(prec)
    x = masked_input(n)
    res = {sel: [forward(net, sel, x, f"conv1_zero_inf_{sel}", skips=False) for _ in range(2)] for sel in (KNOB, ZERO)}
    for i in range(2):
        assert_same(res[ZERO][i], res[KNOB][i], (prec, n, "Inf weight", i))
        assert res[ZERO][i][2][1:] == (0, 0), res[ZERO][i][2]
