"""GPU: the rgb and semantic heads computed at a step's last level only (RelativePosePipeline(level_outputs="last"), the default).

Levels before the last run the pose-outputs forward, the last level a full forward that is self-cached BEHIND them: it takes everything
head-independent and the n / d skip halves from the workspace and computes the rgb head's skip halves itself.  Everything such a step
hands out must be what a step of three full forwards hands out, in every bit -- compared as int32 bit patterns (signed zeros count, a NaN
equals itself), no tolerance anywhere.  Inputs are masked views as tests/test_gpu_zero_tiles.py builds them; n = 4 is the smallest batch
the zero-warp plan accepts, n = 6 has three BatchNorm groups."""
import pytest

from gpu_util import log
from relativepose_amd import _lib, params, synth
from test_gpu_zero_tiles import make_net, masked_input

pytestmark = pytest.mark.gpu

S = 15
TAPS = ("D3", "D2", "A4")
PRECS = ["bf16x6", "bf16x9", "f32", "f16x3"]
_levels = {}


def levels(n):
    """The three inputs of one step: one set of masked own views (channels 0:8), warped channels zero / set / others."""
    if n not in _levels:
        x1 = masked_input(n, "suncg", "second", 700 + n)
        x2 = x1.clone(); x2[:, 8:] = masked_input(n, "suncg", "second", 710 + n)[:, 8:]
        x0 = x1.clone(); x0[:, 8:] = 0
        _levels[n] = (x0, x1, x2)
    return _levels[n]


def fwd(net, x, flags=0, **kw):
    """(output, D3, D2, A4) of one forward as int32 bit patterns; fwd.units = the conv1 blocks it launched (a self-cached forward launches
    the warped streams' half: no case can pass by recomputing everything, or by trusting a cache it must not trust)."""
    import torch
    y = (net.forward_flags(x, flags=flags, self_tag=kw.get("self_tag", 0)) if flags else net.forward(x, **kw)).clone()
    fwd.units = net.conv1_zero()[0]
    return [t.view(torch.int32) for t in [y] + [net.read_tap(t).clone() for t in TAPS]]


def full_units(net, x):
    fwd(net, x)
    return fwd.units


def same(a, b, what, taps=True):
    import torch
    for name, u, v in zip(("output",) + TAPS, a, b):
        if taps or name == "output":
            assert torch.equal(u, v), (what, name, int((u != v).sum()))


def pose_channels_same(a, b, what):
    import torch
    assert torch.equal(a[0][:, 3:7], b[0][:, 3:7]) and torch.equal(a[0][:, 7 + S:], b[0][:, 7 + S:]), what


def sequence(net, x, outputs):
    """One step's forwards on one workspace under one fresh tag, then a fourth forward (all outputs, same tag)."""
    full = full_units(net, x[1])
    tag = net.new_self_tag()
    r = [fwd(net, x[0], zero_warp=True, outputs=outputs[0], self_tag=tag)]
    for xl, o in ((x[1], outputs[1]), (x[2], "all"), (x[1], "all")):
        r.append(fwd(net, xl, outputs=o, self_tag=tag))
        assert fwd.units * 2 == full, ("not self-cached", len(r) - 1, outputs)
    return r


@pytest.mark.parametrize("n", [4, 6])
@pytest.mark.parametrize("prec", PRECS)
def test_last_level_behind_pose_levels_is_the_full_forward(prec, n):
    import torch
    net = make_net(prec)
    x = levels(n)
    plain1, plain2 = fwd(net, x[1]), fwd(net, x[2])                      # tag-less: always the complete forward
    A = sequence(net, x, ("pose", "pose"))
    B = sequence(net, x, ("all", "all"))
    same(A[2], B[2], (prec, n, "level 2, A against B"))                   # all 54 channels, D3, D2, A4
    for lvl in (0, 1):
        pose_channels_same(A[lvl], B[lvl], (prec, n, "level", lvl))
    same(A[2], plain2, (prec, n, "level 2 against the tag-less forward"))
    same(A[3], plain1, (prec, n, "fourth forward"))
    same(B[3], plain1, (prec, n, "fourth forward, B"))
    assert bool(torch.isfinite(plain2[0].view(torch.float32)).all()) and int((plain2[0][:, :3] != 0).sum()) > 0
    assert int((A[0][0][:, :3] != 0).sum()) == 0 and int((A[1][0][:, 7:7 + S] != 0).sum()) == 0      # the pose levels really ran the pose plan
    log("last_level_outputs_bitwise", prec=prec, images=n)


@pytest.mark.parametrize("prec", PRECS)
def test_snapshot_mask_logic(prec):
    net = make_net(prec)
    n = 4
    x = levels(n)
    plain1, plain2 = fwd(net, x[1]), fwd(net, x[2])
    full = fwd.units
    # all, pose, all under one tag: the pose forward (cached) leaves the first forward's rgb snapshots alone, the third may start from them
    tag = net.new_self_tag()
    same(fwd(net, x[1], self_tag=tag), plain1, (prec, "fill, all outputs"))
    pose_channels_same(fwd(net, x[2], outputs="pose", self_tag=tag), plain2, (prec, "cached pose forward"))
    same(fwd(net, x[2], self_tag=tag), plain2, (prec, "all behind all + pose"))
    assert fwd.units * 2 == full
    # a pose fill, then all outputs with another tag / on a workspace declared new / at another n: everything is recomputed
    tag = net.new_self_tag()
    fwd(net, x[1], outputs="pose", self_tag=tag)
    same(fwd(net, x[2], self_tag=net.new_self_tag()), plain2, (prec, "another tag"))
    assert fwd.units == full
    tag = net.new_self_tag()
    fwd(net, x[1], outputs="pose", self_tag=tag)
    same(fwd(net, x[2], flags=net.FLAG_NEW_WORKSPACE, self_tag=tag), plain2, (prec, "new workspace"))
    assert fwd.units == full
    tag = net.new_self_tag()
    fwd(net, x[1], outputs="pose", self_tag=tag)
    x6 = levels(6)
    same(fwd(net, x6[2], self_tag=tag), fwd(net, x6[2]), (prec, "another n"), taps=True)
    # the pose fill of a zero-warp level (level 0 as the pipeline runs it), then the cached full forward
    tag = net.new_self_tag()
    fwd(net, x[0], zero_warp=True, outputs="pose", self_tag=tag)
    same(fwd(net, x[2], self_tag=tag), plain2, (prec, "all behind a level-0 pose fill"))
    assert fwd.units * 2 == full


@pytest.mark.parametrize("knobs", [dict(zero_tiles=1), dict(conv4_rows=1)])
def test_sequences_agree_without_the_lists(knobs):
    net = make_net("bf16x6")
    x = levels(6)
    with _lib.tuning(**knobs):
        A = sequence(net, x, ("pose", "pose"))
        B = sequence(net, x, ("all", "all"))
    same(A[2], B[2], (knobs, "level 2"))
    same(A[3], B[3], (knobs, "fourth forward"))
    for lvl in (0, 1):
        pose_channels_same(A[lvl], B[lvl], (knobs, lvl))


def test_lane_per_pixel_heads_kernel_carries_the_mixed_case():
    net = make_net("bf16x6")
    x = levels(6)
    plain1, plain2 = fwd(net, x[1]), fwd(net, x[2])
    with _lib.tuning(heads_kernel=1):
        A = sequence(net, x, ("pose", "pose"))
    same(A[2], plain2, "lane-per-pixel heads, level 2")
    same(A[3], plain1, "lane-per-pixel heads, fourth forward")


def test_pipeline_last_against_every():
    import torch
    from relativepose_amd.pipeline import RelativePosePipeline
    dev = torch.device("cuda:0")
    Bp, N = 2, 80
    net = make_net("bf16x6")
    sig = params.final_params("suncg")
    batches = []
    for k in range(4):
        d = synth.make_pairs(Bp, 900 + k, "suncg")
        pts, ptw = synth.make_keypoints(Bp, N, 900 + k, "second")
        batches.append((d, pts, ptw))
    res = {}
    for mode in ("last", "every"):
        pipe = RelativePosePipeline(net, "suncg", "second", sig, level_outputs=mode)
        sts = [pipe.prepare(d["rgb"], d["norm"], d["depth"], pts, ptw, dev) for d, pts, ptw in batches]
        pose, status, _ = pipe.run(sts[0])
        out = {"run": (pose.clone(), status.clone(), sts[0]["f"].clone())}
        r = pipe.run_pipelined(sts, 4, depth=3)
        torch.cuda.synchronize()
        out["pipelined"] = [(p.clone(), s.clone(), st["f"].clone()) for (p, s), st in zip(r, sts)]
        r = pipe.run_interleaved(sts[:2])
        torch.cuda.synchronize()
        out["interleaved"] = [(p.clone(), s.clone(), st["f"].clone()) for (p, s), st in zip(r, sts[:2])]
        if mode == "last":
            keep = []
            pipe.run(sts[0], keep=keep)
            assert int((keep[0]["f"][:, :3] != 0).sum()) > 0 and int((keep[0]["f"][:, 7:7 + S] != 0).sum()) > 0     # keep: every level's maps
        res[mode] = out

    def eq(a, b, what):
        for u, v, name in zip(a, b, ("pose", "status", "f")):
            if u.dtype == torch.float32:
                u, v = u.view(torch.int32), v.view(torch.int32)
            elif u.dtype == torch.float64:
                u, v = u.view(torch.int64), v.view(torch.int64)
            assert torch.equal(u, v), (what, name)

    eq(res["last"]["run"], res["every"]["run"], "run")
    for k in range(4):
        eq(res["last"]["pipelined"][k], res["every"]["pipelined"][k], ("run_pipelined", k))
    for k in range(2):
        eq(res["last"]["interleaved"][k], res["every"]["interleaved"][k], ("run_interleaved", k))
    assert int((res["last"]["run"][2][:, :3] != 0).sum()) > 0                  # the final maps are there
