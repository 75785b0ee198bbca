"""Float64 teacher-forced reference of SCNet (test infrastructure, no GPU).

Every conv / transposed conv of the network is recomputed in float64 from the *given* raw taps of its inputs (the NHWC pre-BatchNorm
buffers `SCNet.read_tap` returns, or the fp32 oracle's own taps): BatchNorm over the image pair (batch statistics, biased variance,
eps 1e-5) or, for batchnorm=0 nets, the producer's conv bias (the consumer's loader adds it), LeakyReLU 0.1, the skip concatenation of
model/mymodel.py, then `F.conv2d` / `F.conv_transpose2d` in float64.  An error of a layer's output tap is then the error of that one
layer, and each precision mode can be held to the bound its arithmetic predicts.

Errors are normalised per element by a magnitude: the same layer computed with |W| on |x * scale| + |shift| (the size of the loader's
fp32 transform, before the activation's slope), + |bias| for the heads.  That bounds what fp32 rounding of the loader, of the products
and of the accumulation can do to that element, so border pixels and near-cancelling outputs are judged like the rest.

The three fp32 stages get the same treatment: resize_in (X0 vs a float64 bilinear resize of the input), the heads (OUT vs float64 1x1
convs + bias (+ tanh on f) of the D2 / A1 taps) and resize_out (the output vs a float64 bilinear resize of OUT)."""
import numpy as np
import torch
import torch.nn.functional as F

# buffer -> list of (oracle tap name, call index, channel offset, channels)
TAP_MAP = {
    "A1": [("conv1rgb", 0, 0, 32), ("conv1rgb", 1, 32, 32), ("conv1n", 0, 64, 32), ("conv1n", 1, 96, 32), ("conv1d", 0, 128, 32), ("conv1d", 1, 160, 32)],
    "A2": [("conv2rgb", 0, 0, 64), ("conv2rgb", 1, 64, 64), ("conv2n", 0, 128, 64), ("conv2n", 1, 192, 64), ("conv2d", 0, 256, 64), ("conv2d", 1, 320, 64)],
    "A3": [("conv3rgb", 0, 0, 128), ("conv3rgb", 1, 128, 128), ("conv3n", 0, 256, 128), ("conv3n", 1, 384, 128), ("conv3d", 0, 512, 128), ("conv3d", 1, 640, 128)],
    "A4": [("conv4", 0, 0, 256)], "A5": [("conv5", 0, 0, 512)], "A6": [("conv6", 0, 0, 512)], "A7": [("conv7", 0, 0, 512)],
    "A8": [("conv8", 0, 0, 512)], "A9": [("conv9", 0, 0, 1024)], "D9": [("deconv9", 0, 0, 512)], "D8": [("deconv8", 0, 0, 512)],
    "D7": [("deconv7", 0, 0, 512)], "D6": [("deconv6", 0, 0, 512)], "D5": [("deconv5", 0, 0, 256)], "D4": [("deconv4", 0, 0, 128)],
    "D3": [("deconv3rgb", 0, 0, 64), ("deconv3n", 0, 64, 64), ("deconv3d", 0, 128, 64), ("deconv3s", 0, 192, 64), ("deconv3f", 0, 256, 64)],
    "D2": [("deconv2rgb", 0, 0, 32), ("deconv2n", 0, 32, 32), ("deconv2d", 0, 64, 32), ("deconv2s", 0, 96, 64), ("deconv2f", 0, 160, 64)],
}
HEAD_NAMES = ("rgb", "n", "d", "s", "f")
EPS_BN = 1e-5
SLOPE = 0.1
U = 2.0 ** -24                       # unit roundoff of float32

# Per-mode bounds of a layer's normalised error (max, rms over the layer's elements), in units of U.  Derived from the float64 emulation of
# each mode's products on one layer per kernel family (tests/test_scnet_f64_cpu.py, case a): MARGIN x the largest emulated level,
# rounded up.  Emulated levels (max / rms): f32 = bf16x9 = bf16x6 2.0 / 0.23, f16x3 2.0 / 0.23, bf16x3 19.7 / 3.6, f16 1122 / 202.
# The fp32 stages (conv1's direct kernel, the fused heads, both resizes) are held to the f32-class bound in every mode.
MARGIN = 4
F32_CLASS = (10 * U, 1.0 * U)
MODE_BOUNDS = {"f32": F32_CLASS, "bf16x9": F32_CLASS, "bf16x6": F32_CLASS, "f16x3": F32_CLASS,
               "bf16x3": (80 * U, 15 * U), "f16": (4500 * U, 810 * U)}

# (stride, pad) of every layer (model/mymodel.py:259-380, as oracle/scnet_oracle.py restates it)
_CONV_SP = {"conv1": (1, 1), "conv2": (2, 1), "conv3": (2, 1), "conv4": (2, 1), "conv5": (2, 1), "conv6": (2, 1), "conv7": (2, 0),
            "conv8": (1, 1), "conv9": (1, 0)}
_DECONV_SP = {"deconv9": (1, 0), "deconv8": (1, 1), "deconv7": (2, 0), "deconv6": (2, 1), "deconv5": (2, 1), "deconv4": (2, 1),
              "deconv3": (2, 1), "deconv2": (2, 1)}


def head_channels(S):
    return {"rgb": 3, "n": 3, "d": 1, "s": S, "f": 32}


def layer_calls(S=15, skip=1, output_type="rgbdnsf"):
    """Every conv / transposed-conv call of the forward, in order: dicts with
    name (weight key prefix), call (index among the calls of that name), kind ('conv' / 'deconv'), stride, pad,
    srcs: the input's channel blocks in concatenation order, (buffer, channel offset, channels), and out: (buffer, offset, channels)."""
    blk = {(o, ci): (b, off, ch) for b, lst in TAP_MAP.items() for (o, ci, off, ch) in lst}
    calls = []

    def add(name, call, kind, base, srcs):
        s, p = (_CONV_SP if kind == "conv" else _DECONV_SP)[base]
        calls.append(dict(name=name, call=call, kind=kind, stride=s, pad=p, srcs=srcs, out=blk[(name, call)]))

    for m, ch in (("rgb", (0, 3)), ("n", (3, 6)), ("d", (6, 7))):
        for s, off in ((0, 0), (1, 8)):
            add(f"conv1{m}", s, "conv", "conv1", [("X0", off + ch[0], ch[1] - ch[0]), ("X0", off + 7, 1)])
            add(f"conv2{m}", s, "conv", "conv2", [blk[(f"conv1{m}", s)]])
            add(f"conv3{m}", s, "conv", "conv3", [blk[(f"conv2{m}", s)]])
    add("conv4", 0, "conv", "conv4", [blk[(f"conv3{m}", s)] for m in ("rgb", "n", "d") for s in (0, 1)])
    for i in range(5, 10):
        add(f"conv{i}", 0, "conv", f"conv{i}", [blk[(f"conv{i - 1}", 0)]])
    add("deconv9", 0, "deconv", "deconv9", [blk[("conv9", 0)]])
    for i in range(8, 3, -1):
        add(f"deconv{i}", 0, "deconv", f"deconv{i}", [blk[(f"deconv{i + 1}", 0)]] + ([blk[(f"conv{i}", 0)]] if skip else []))
    for m in ("rgb", "n", "d"):
        if m in output_type:
            add(f"deconv3{m}", 0, "deconv", "deconv3", [blk[("deconv4", 0)]] + ([blk[(f"conv3{m}", 0)]] if skip else []))
            add(f"deconv2{m}", 0, "deconv", "deconv2", [blk[(f"deconv3{m}", 0)]] + ([blk[(f"conv2{m}", 0)]] if skip else []))
    for m in ("s", "f"):
        if m in output_type:
            add(f"deconv3{m}", 0, "deconv", "deconv3", [blk[("deconv4", 0)]])
            add(f"deconv2{m}", 0, "deconv", "deconv2", [blk[(f"deconv3{m}", 0)]])
    return calls


def head_calls(S=15, skip=1, output_type="rgbdnsf"):
    """The 1x1 output convs: dicts with name, head, srcs (as layer_calls) and the head's channel offset / width in OUT."""
    blk = {(o, ci): (b, off, ch) for b, lst in TAP_MAP.items() for (o, ci, off, ch) in lst}
    hc, off, out = head_channels(S), 0, []
    for h in HEAD_NAMES:
        if h in output_type:
            srcs = [blk[(f"deconv2{h}", 0)]] + ([blk[(f"conv1{h}", 0)]] if skip and h in ("rgb", "n", "d") else [])
            out.append(dict(name=f"deconv1{h}", head=h, srcs=srcs, off=off, ch=hc[h]))
        off += hc[h]
    return out


def _producers():
    return {(b, off): o for b, lst in TAP_MAP.items() for (o, ci, off, ch) in lst}


def rows_subset(H):
    """The output rows checked when a layer is checked on a subset: first and last rows (the image boundary of the NHWC buffer lies
    between the last row of one image and the first of the next, and every image of the pair is checked), their neighbours, the rows
    around the middle and a fixed spread in between.  All columns of every checked row are compared."""
    if H <= 28:
        return None
    r = {0, 1, 2, H // 2 - 1, H // 2, H - 3, H - 2, H - 1}
    r |= set(int(v) for v in np.linspace(3, H - 4, 9).round())
    return sorted(r)


def _conv_rows(x, w, stride, pad, rows):
    """F.conv2d(x, w, stride=stride, padding=pad) restricted to the output rows `rows` (None = all): [n, Cout, len(rows), Wout]."""
    if rows is None:
        return F.conv2d(x, w, None, stride, pad)
    n, C, H, W = x.shape
    k = w.shape[2]
    xp = F.pad(x, (0, 0, pad, pad + k))
    slab = torch.stack([xp[:, :, r * stride:r * stride + k] for r in rows], 1)         # [n, R, C, k, W]
    y = F.conv2d(slab.reshape(n * len(rows), C, k, W), w, None, (1, stride), (0, pad))
    return y.reshape(n, len(rows), w.shape[0], -1).permute(0, 2, 1, 3)


def _deconv_rows(x, w, stride, pad, rows):
    """F.conv_transpose2d(x, w, stride=stride, padding=pad) restricted to output rows: the direct conv of the zero-upsampled input with
    the flipped kernel."""
    if rows is None:
        return F.conv_transpose2d(x, w, None, stride, pad)
    n, C, H, W = x.shape
    k = w.shape[2]
    xu = x.new_zeros(n, C, (H - 1) * stride + 1, (W - 1) * stride + 1)
    xu[:, :, ::stride, ::stride] = x
    return _conv_rows(xu, w.flip(2, 3).transpose(0, 1), 1, k - 1 - pad, rows)


def _nchw(a):
    """numpy / torch NHWC -> float64 NCHW torch."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(torch.float64).permute(0, 3, 1, 2).contiguous()


def _lin(n_out, n_in):
    """align_corners=False source coordinates of torch / the kernels: (i0, i1, l0, l1, src) in float64."""
    src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(1 - l1), torch.from_numpy(l1), torch.from_numpy(src)


def bilinear(x, hw):
    """float64 bilinear resize of x [n,C,H,W] to hw (align_corners=False) and its magnitude: the blend of |x|, plus, per direction,
    (source coordinate + 1) x |difference of the two blended samples| -- a fp32 implementation computes the source coordinate with a
    rounding error of a few ulp of its size, which moves the blend weights by that much."""
    ho, wo = hw
    y0, y1, ly0, ly1, sy = _lin(ho, x.shape[2])
    x0, x1, lx0, lx1, sx = _lin(wo, x.shape[3])
    r0, r1 = x[:, :, y0], x[:, :, y1]
    a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    ly0, ly1, sy = ly0[:, None], ly1[:, None], sy[:, None]
    y = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    mag = (ly0 * (lx0 * a.abs() + lx1 * b.abs()) + ly1 * (lx0 * c.abs() + lx1 * d.abs())
           + (sx + 1) * ((b - a).abs() + (d - c).abs()) + (sy + 1) * ((c - a).abs() + (d - b).abs()))
    return y, mag


class F64Reference:
    """Teacher-forced float64 reference for one image pair.

    sd: the state dict ({key: array}); S, use_tanh, batchnorm, skip_layer, output_type: the constructor arguments.
    taps: {buffer: [2, H, H, C] raw NHWC array} for X0, A1..A9, D9..D2 (and OUT for the heads / resize_out); x: the input [2,16,H,W]."""

    def __init__(self, sd, S=15, use_tanh=1, batchnorm=1, skip_layer=1, output_type="rgbdnsf"):
        self.p = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32))).to(torch.float64) for k, v in
                  (sd.items() if isinstance(sd, dict) else sd)}
        self.S, self.use_tanh, self.bn, self.skip, self.otype = S, use_tanh, batchnorm, skip_layer, output_type
        self.calls = layer_calls(S, skip_layer, output_type)
        self.heads = head_calls(S, skip_layer, output_type)
        self.prod = _producers()

    # ---- the loader's transform of one source block: (activation, magnitude), float64 NCHW
    def transform(self, taps, src):
        b, off, ch = src
        raw = _nchw(taps[b][..., off:off + ch])
        if b == "X0":
            return raw, raw.abs()
        prod = self.prod[(b, off)]
        if self.bn:
            mean = raw.mean((0, 2, 3))
            var = raw.var((0, 2, 3), unbiased=False)
            scale = self.p[f"{prod}.1.weight"] / torch.sqrt(var + EPS_BN)
            shift = self.p[f"{prod}.1.bias"] - mean * scale
        else:
            scale = torch.ones(ch, dtype=torch.float64)
            shift = self.p[f"{prod}.0.bias"]
        v = raw * scale[None, :, None, None] + shift[None, :, None, None]
        mag = (raw * scale[None, :, None, None]).abs() + shift.abs()[None, :, None, None]
        return torch.where(v >= 0, v, SLOPE * v), mag

    def layer_input(self, taps, srcs):
        acts, mags = zip(*(self.transform(taps, s) for s in srcs))
        return torch.cat(acts, 1), torch.cat(mags, 1)

    def layer(self, taps, c, rows=None):
        """float64 (reference, magnitude) of one call, NHWC [2, R, W, Cout] (R = all rows or `rows`)."""
        a, m = self.layer_input(taps, c["srcs"])
        w = self.p[f"{c['name']}.0.weight"]
        op = _conv_rows if c["kind"] == "conv" else _deconv_rows
        y = op(a, w, c["stride"], c["pad"], rows)
        mag = op(m, w.abs(), c["stride"], c["pad"], rows)
        return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()

    def head(self, taps, h, rows=None):
        """float64 (reference, magnitude) of one 1x1 head, NHWC [2, R, 224, ch]: conv + bias (+ tanh on f)."""
        a, m = self.layer_input(taps, h["srcs"])
        if rows is not None:
            a, m = a[:, :, rows], m[:, :, rows]
        w, b = self.p[f"{h['name']}.weight"], self.p[f"{h['name']}.bias"]
        y = F.conv2d(a, w, b)
        mag = F.conv2d(m, w.abs(), b.abs())
        if h["head"] == "f" and self.use_tanh:
            y = torch.tanh(y)
        return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()

    @staticmethod
    def resize_in(x):
        """X0 = bilinear resize of the input to 224 x 224 (align_corners=False), NHWC float64, and its magnitude."""
        y, mag = bilinear(torch.from_numpy(np.ascontiguousarray(x)).to(torch.float64), (224, 224))
        return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()

    @staticmethod
    def resize_out(out224, hw, channels=None):
        """The output = bilinear resize of the OUT tap ([2,224,224,C] NHWC) to hw, NCHW float64 (channels: the selected ones)."""
        o = _nchw(out224)
        if channels is not None:
            o = o[:, channels]
        y, mag = bilinear(o, hw)
        return y.numpy(), mag.numpy()

    def max_activation(self, taps):
        """Largest |loader output| over the inputs of every layer after conv1: the activations a 16-bit mode converts."""
        amax = 0.0
        for c in self.calls + self.heads:
            for s in c["srcs"]:
                if s[0] == "X0":
                    continue
                a, _ = self.transform(taps, s)
                amax = max(amax, float(a.abs().max()))
        return amax


def norm_err(got, ref, mag):
    """(max, rms) of |got - ref| / mag; a zero magnitude admits only an exact zero error.  Non-finite values give inf."""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - ref)
    if not np.isfinite(d).all():
        return float("inf"), float("inf")
    e = np.where(mag > 0, d / np.where(mag > 0, mag, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(e.max()), float(np.sqrt((e ** 2).mean()))


def check_pair(ref, taps, x, y=None, subset=False):
    """Every layer, the heads and both resizes of one image pair: a list of dicts (stage, buffer, layer, call, max, rms).
    taps: numpy NHWC per buffer (2 images); x: the input [2,16,H,W]; y: the network output [2,C,H,W], the heads that exist in the
    reference's channel order (None: no resize_out check);
    subset: check the 224 / 112 / 56-row layers and the heads on rows_subset() only."""
    res = []
    x0, m0 = ref.resize_in(x)
    res.append(dict(stage="resize_in", buffer="X0", layer="resize_in", call=0, rows=224, **dict(zip(("max", "rms"), norm_err(taps["X0"], x0, m0)))))
    for c in ref.calls:
        b, off, ch = c["out"]
        H = taps[b].shape[1]
        rows = rows_subset(H) if subset else None
        yr, mr = ref.layer(taps, c, rows)
        got = taps[b][..., off:off + ch]
        if rows is not None:
            got = got[:, rows]
        res.append(dict(stage="layer", buffer=b, layer=c["name"], call=c["call"], rows=H if rows is None else len(rows),
                        **dict(zip(("max", "rms"), norm_err(got, yr, mr)))))
    if "OUT" in taps:
        rows = rows_subset(224) if subset else None
        for h in ref.heads:
            yr, mr = ref.head(taps, h, rows)
            got = taps["OUT"][..., h["off"]:h["off"] + h["ch"]]
            if rows is not None:
                got = got[:, rows]
            res.append(dict(stage="head", buffer="OUT", layer=h["name"], call=0, rows=224 if rows is None else len(rows),
                            **dict(zip(("max", "rms"), norm_err(got, yr, mr)))))
        if y is not None:
            sel = [c for h in ref.heads for c in range(h["off"], h["off"] + h["ch"])]
            yr, mr = ref.resize_out(taps["OUT"], y.shape[2:], sel)
            res.append(dict(stage="resize_out", buffer="y", layer="resize_out", call=0, rows=int(y.shape[2]),
                            **dict(zip(("max", "rms"), norm_err(y, yr, mr)))))
    return res


def oracle_taps(orc, x):
    """The fp32 TapOracle's own taps in the library's NHWC buffer layout (blocks of absent heads = zero; batchnorm=0: without the conv
    bias, like the library's buffers: subtracted unless the oracle's `tap_has_bias` is False), X0 and OUT; the oracle must have run its
    forward on x."""
    p = orc.p
    taps = {"X0": F.interpolate(torch.from_numpy(np.ascontiguousarray(x)).float(), [224, 224], mode="bilinear",
                                align_corners=False).permute(0, 2, 3, 1).numpy()}
    for b, lst in TAP_MAP.items():
        C = max(off + ch for (_, _, off, ch) in lst)
        H = None
        blocks = []
        for (o, ci, off, ch) in lst:
            if o in orc.calls:
                t = orc.calls[o][ci]
                if not orc.batchnorm and getattr(orc, "tap_has_bias", True):
                    t = t - p[f"{o}.0.bias"][None, :, None, None]
                blocks.append((off, ch, t.permute(0, 2, 3, 1).numpy()))
                H = t.shape[2]
        a = np.zeros((2, H, H, C), np.float32)
        for off, ch, t in blocks:
            a[..., off:off + ch] = t
        taps[b] = a
    hc = head_channels(orc.S)
    outs, off = [], 0
    cat = orc.taps["out224"].permute(0, 2, 3, 1).numpy()
    full = np.zeros((2, 224, 224, sum(hc.values())), np.float32)
    src = 0
    for h in HEAD_NAMES:
        if h in orc.output_type:
            full[..., off:off + hc[h]] = cat[..., src:src + hc[h]]
            src += hc[h]
        off += hc[h]
    taps["OUT"] = full
    return taps
