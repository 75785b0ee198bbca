"""numpy model of SCNet's zero-tile skipping (csrc/scnet.hip: x0_occupancy_kernel, zero_tile_list_kernel).

The resized network input X0 [n, 224, 224, 16] is mostly exact zeros (util.apply_mask keeps one face; the warped partner view is that
face splatted into a zero panorama).  conv1 has no bias, so A1 is +0 wherever the 3 x 3 neighbourhood of X0 is zero, and after
BatchNorm + LeakyReLU such a region is one constant per channel and BatchNorm group: a conv2 / conv3 patch whose whole receptive field
lies in it computes a tile that depends on the patch's edge class only.

Geometry (all inclusive ranges, clipped to the image):
  conv2 patch p (16 outputs of 112)  reads A1 rows 32p - 1 .. 32p + 32   = X0 rows 32p - 2 .. 32p + 33
  conv3 patch p (8 outputs of 56)    reads A2 rows 16p - 1 .. 16p + 16   = A1 rows 32p - 3 .. 32p + 34 = X0 rows 32p - 4 .. 32p + 35
Both lie inside the 8-pixel occupancy blocks 4p - 1 .. 4p + 4 (X0 rows 32p - 8 .. 32p + 39): the one block range the kernels test.
"""
import numpy as np

RS, BLK, NB, NP = 224, 8, 28, 7          # X0 size, occupancy block, blocks per side, patches per side (conv2: 16 of 112, conv3: 8 of 56)
PPI = NP * NP                            # patches per image and stream


def stream_channels(q):
    """Input channels of conv1 block q = 2 m + s (m: rgb, n, d; s: self, warped) -- conv1_inputs in csrc/scnet.hip."""
    m, off = q // 2, 8 * (q % 2)
    return [[off + 0, off + 1, off + 2, off + 7], [off + 3, off + 4, off + 5, off + 7], [off + 6, off + 7]][m]


def occupancy(x0):
    """x0 [n, 224, 224, 16] float32 -> (occ [n, 6, 28, 28] bool, nonfinite [n, 6] bool).
    A block is occupied iff some channel of the stream has a bit pattern other than +0 / -0 in it (NaN and Inf are occupied)."""
    x0 = np.asarray(x0, np.float32)
    n = x0.shape[0]
    bits = x0.view(np.uint32) & np.uint32(0x7fffffff)
    occ = np.zeros((n, 6, NB, NB), bool)
    nonfinite = np.zeros((n, 6), bool)
    nz = (bits != 0).reshape(n, NB, BLK, NB, BLK, 16).any((2, 4))                 # [n, 28, 28, 16]
    bad = (bits >= np.uint32(0x7f800000)).any((1, 2))                            # [n, 16]
    for q in range(6):
        occ[:, q] = nz[..., stream_channels(q)].any(-1)
        nonfinite[:, q] = bad[:, stream_channels(q)].any(-1)
    return occ, nonfinite


def block_range(p):
    """Occupancy blocks [lo, hi) tested for patch row / column p."""
    return max(4 * p - 1, 0), min(4 * p + 5, NB)


def field_rows(layer, p):
    """Exact X0 rows [lo, hi] (inclusive, clipped) in the receptive field of patch row p of conv2 / conv3."""
    m = 2 if layer == 2 else 4
    return max(32 * p - m, 0), min(32 * p + 31 + m, RS - 1)


def redundant(occ, nonfinite):
    """-> red [n, 6, 7, 7] bool.  A non-finite value anywhere in a BatchNorm group's stream makes the group's {scale, shift} NaN: nothing
    in that group and stream is redundant."""
    n = occ.shape[0]
    red = np.zeros((n, 6, NP, NP), bool)
    for py in range(NP):
        y0, y1 = block_range(py)
        for px in range(NP):
            x0, x1 = block_range(px)
            red[:, :, py, px] = ~occ[:, :, y0:y1, x0:x1].any((2, 3))
    bad = nonfinite.reshape(n // 2, 2, 6).any(1)                      # [G, 6]
    red &= ~np.repeat(bad, 2, 0)[:, :, None, None]
    return red


def edge_class(p):
    """0..8: 3 * (top, middle, bottom) + (left, middle, right) of patch index p (0..48) within its image."""
    cls = lambda i: 0 if i == 0 else (2 if i == NP - 1 else 1)
    return 3 * cls(p // NP) + cls(p % NP)


def tile_lists(red_q, pair):
    """red_q [nimg, 7, 7] bool (one launch member).  -> (computed, fills): `computed` the ascending list of units (patches, or pairs of
    consecutive patches for conv3) that run, `fills` the list of (dropped unit, representative unit).  Per BatchNorm group (2 images) and
    key (the edge class, or the two classes of a pair) the lowest-index all-redundant unit is the representative and runs."""
    nimg = red_q.shape[0]
    flat = red_q.reshape(nimg * PPI)
    per = 2 if pair else 1
    units_per_group = 2 * PPI // per
    computed, fills = [], []
    for u in range(nimg * PPI // per):
        ps = [per * u + k for k in range(per)]
        if not all(flat[p] for p in ps):
            computed.append(u)
            continue
        key = tuple(edge_class(p % PPI) for p in ps)
        g = u // units_per_group
        rep = None
        for v in range(g * units_per_group, u):
            pv = [per * v + k for k in range(per)]
            if all(flat[p] for p in pv) and tuple(edge_class(p % PPI) for p in pv) == key:
                rep = v
                break
        if rep is None:
            computed.append(u)
        else:
            fills.append((u, rep))
    return computed, fills


def plan_members(plan, n):
    """(q, images) of the conv2 / conv3 launch members of a plan: 'full', 'zero_warp' (warped streams on the first image pair only: the caller
    promises zeros in every image's warped channels, the lists still read what is there), 'self_cached' (warped streams only)."""
    if plan == "full":
        return [(q, n) for q in range(6)]
    if plan == "zero_warp":
        return [(q, n) for q in (0, 2, 4)] + [(q, 2) for q in (1, 3, 5)]
    if plan == "self_cached":
        return [(q, n) for q in (1, 3, 5)]
    raise ValueError(plan)


def counts(x0, plan="full", skip=True):
    """What the library's read-out reports for a forward over x0: {layer: (units computed, units dropped)} for layers 2 and 3
    (units: conv2 patches, conv3 patch pairs), summed over the launch members of the plan."""
    n = x0.shape[0]
    occ, nf = occupancy(x0)
    red = redundant(occ, nf)
    out = {}
    for layer in (2, 3):
        comp = drop = 0
        for q, nimg in plan_members(plan, n):
            units = nimg * PPI // (2 if layer == 3 else 1)
            if skip:
                c, f = tile_lists(red[:nimg, q], layer == 3)
                assert len(c) + len(f) == units
                comp += len(c)
                drop += len(f)
            else:
                comp += units
        out[layer] = (comp, drop)
    return out


def x0_support(in_nz):
    """Integer propagation of support through the bilinear resize (align_corners=False, the oracle's F.interpolate): in_nz [n, 16, H, W]
    bool -> [n, 224, 224, 16] bool, True where an X0 pixel has a tap on a nonzero input pixel (whatever the tap's weight)."""
    n, c, H, W = in_nz.shape

    def taps(size):
        src = np.maximum((np.arange(RS) + 0.5) * size / RS - 0.5, 0.0)
        i0 = np.minimum(np.floor(src + 1e-6).astype(int), size - 1)            # (+- 1e-6: both candidates when src is within rounding of an integer)
        lo = np.minimum(np.floor(src - 1e-6).astype(int).clip(0), size - 1)
        return lo, np.minimum(i0 + 1, size - 1)
    ylo, yhi = taps(H)
    xlo, xhi = taps(W)
    cs = np.zeros((n, c, H + 1, W + 1), np.int64)
    cs[:, :, 1:, 1:] = in_nz.cumsum(2).cumsum(3)
    box = (cs[:, :, yhi + 1][:, :, :, xhi + 1] - cs[:, :, ylo][:, :, :, xhi + 1] - cs[:, :, yhi + 1][:, :, :, xlo] + cs[:, :, ylo][:, :, :, xlo])
    return (box > 0).transpose(0, 2, 3, 1)
