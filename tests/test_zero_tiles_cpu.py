"""CPU: the numpy model of SCNet's zero-tile skipping (tests/zero_tiles_model.py = x0_occupancy_kernel + zero_tile_list_kernel).

* A patch the model calls redundant has an exactly zero A1 footprint: the support of the input is propagated with integer arithmetic
  through the oracle's resize (every tap counts, whatever its weight), conv1's 3 x 3 window and the 4 x 4 stride-2 pad-1 windows of conv2 /
  conv3, and must miss the patch's receptive field.
* Probes: one non-zero value (1.0, -0.0 next to it, a denormal, NaN) in X0 one pixel inside and one pixel outside every margin -- of
  the exact receptive field (inside => never redundant: the safety property) and of the tested block range (outside => redundant: the
  model is what its docstring says) -- at patch corners and edges and at all four image borders, in every stream's channel set.
* The nine edge classes: float64 torch conv2 / conv3 of a constant field give equal tiles within a class (tile against tile; no value
  is compared with the GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import zero_tiles_model as Z

RS = Z.RS


def a1_support(x0_nz, q):
    """[n, 224, 224] bool: A1 pixels of stream q with a non-zero X0 value under conv1's 3 x 3 pad-1 window."""
    s = x0_nz[..., Z.stream_channels(q)].any(-1)
    p = np.pad(s, ((0, 0), (1, 1), (1, 1)))
    return np.stack([p[:, dy:dy + RS, dx:dx + RS] for dy in range(3) for dx in range(3)]).any(0)


def s2_support(s):
    """Support under a 4 x 4 stride-2 pad-1 window: out(y) reads in(2y - 1 .. 2y + 2)."""
    H = s.shape[1]
    p = np.pad(s, ((0, 0), (1, 1), (1, 1)))
    return np.stack([p[:, dy:dy + H:2, dx:dx + H:2] for dy in range(4) for dx in range(4)]).any(0)


def assert_redundant_means_zero_footprint(x0_nz, red):
    for q in range(6):
        a1 = a1_support(x0_nz, q)
        a2 = s2_support(a1)                  # A2 pixels that are NOT the class constant
        a3 = s2_support(a2)
        for layer, sup, sz in ((2, a2, 16), (3, a3, 8)):
            tiles = sup.reshape(-1, 7, sz, 7, sz).any((2, 4))
            bad = red[:, q] & tiles
            # conv2: a redundant patch computes from zero A1 only; conv3 (same flags): from constant A2 only
            assert not bad.any(), (q, layer, np.argwhere(bad)[:4])


def test_redundant_patches_have_zero_footprint_on_masked_views():
    rs = np.random.RandomState(5)
    n, H, W = 4, 160, 640
    x = np.zeros((n, 16, H, W), np.float32)
    x[0, :8, :, 160:320] = rs.rand(8, H, 160) + 0.1                    # 'second'
    x[1, :8, 47:113, 196:284] = rs.rand(8, 66, 88) + 0.1               # 'kinect' box
    for i in range(n):                                                 # warped views: sparse splats
        k = rs.rand(H, W) < (0.0, 0.002, 0.05, 0.2)[i]
        x[i, 8:] = (rs.rand(8, H, W) + 0.1) * k
    x[2, 6] = 0                                                        # a depth channel of zeros, the mask channel alone carries the stream
    x0 = F.interpolate(torch.from_numpy(x), [RS, RS], mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    sup = Z.x0_support(x != 0)
    assert not ((x0 != 0) & ~sup).any()                                # the integer propagation covers the oracle's resize
    occ, nf = Z.occupancy(x0)
    assert not nf.any()
    red = Z.redundant(occ, nf)
    assert red.any() and not red.all()
    assert_redundant_means_zero_footprint(sup, red)


def probe_positions():
    """X0 rows / columns one pixel inside and outside the exact field and the tested block range of patches 0, 3 and 6, and the borders."""
    pos = {0, 1, RS - 2, RS - 1}
    for layer in (2, 3):
        for p in (0, 3, 6):
            lo, hi = Z.field_rows(layer, p)
            b0, b1 = Z.block_range(p)
            pos |= {lo - 1, lo, hi, hi + 1, 8 * b0 - 1, 8 * b0, 8 * b1 - 1, 8 * b1}
    return sorted(v for v in pos if 0 <= v < RS)


PROBE_VALUES = [1.0, np.float32(1e-40), np.float32(np.nan)]


@pytest.mark.parametrize("channel", [0, 3, 6, 7, 8, 12, 14, 15])
def test_single_value_probes_at_every_margin(channel):
    pos = probe_positions()
    streams = [q for q in range(6) if channel in Z.stream_channels(q)]
    assert streams
    for vi, val in enumerate(PROBE_VALUES):
        # (1.0: every margin along one axis against a third of them along the other, the axes swapped from channel to channel)
        full, part = (pos, pos[::3]) if vi == 0 else (pos[::5], pos[::5])
        for y in (full if channel % 2 else part):
            for x in (part if channel % 2 else full):
                x0 = np.zeros((2, RS, RS, 16), np.float32)
                x0[1, y, x, channel] = val
                x0[0, y, x, (channel + 1) % 16] = -0.0                 # a negative zero is a zero
                occ, nf = Z.occupancy(x0)
                assert not occ[0].any() and occ[1, streams].sum() == len(streams) and occ.sum() == len(streams)
                red = Z.redundant(occ, nf)
                if not np.isfinite(val):
                    assert not red[:, streams].any() and red[:, [q for q in range(6) if q not in streams]].all()
                    continue
                assert red[0].all()
                for q in range(6):
                    if q not in streams:
                        assert red[1, q].all()
                        continue
                    for py in range(7):
                        for px in range(7):
                            in_field = any(Z.field_rows(l, py)[0] <= y <= Z.field_rows(l, py)[1] and Z.field_rows(l, px)[0] <= x <= Z.field_rows(l, px)[1]
                                           for l in (2, 3))
                            in_blocks = (8 * Z.block_range(py)[0] <= y < 8 * Z.block_range(py)[1] and 8 * Z.block_range(px)[0] <= x < 8 * Z.block_range(px)[1])
                            assert not (in_field and not in_blocks)
                            assert red[1, q, py, px] == (not in_blocks), (val, y, x, q, py, px)


def test_lists_keep_one_representative_per_group_and_class():
    red = np.ones((4, 7, 7), bool)
    red[1, 3, 3] = False
    comp, fills = Z.tile_lists(red, pair=False)
    assert len(comp) == 9 + 1 + 9 and len(fills) == 4 * 49 - 19
    assert all(Z.edge_class(u % 49) == Z.edge_class(r % 49) and u // 98 == r // 98 and r < u and r in comp for u, r in fills)
    comp, fills = Z.tile_lists(red, pair=True)
    assert len(comp) + len(fills) == 98 and (49 + 24) // 2 in comp          # the pair that holds the active patch runs
    for u, r in fills:
        assert r in comp and u // 49 == r // 49 and [Z.edge_class(p % 49) for p in (2 * u, 2 * u + 1)] == [Z.edge_class(p % 49) for p in (2 * r, 2 * r + 1)]
    assert Z.tile_lists(np.zeros((2, 7, 7), bool), pair=True) == (list(range(49)), [])


def test_nine_edge_classes_on_a_constant_field():
    g = torch.Generator().manual_seed(3)
    c1, c2, c3 = 3, 5, 4
    a1 = torch.rand(c1, generator=g, dtype=torch.float64).view(1, c1, 1, 1).expand(1, c1, RS, RS)     # BatchNorm + LeakyReLU of a zero A1
    w2 = torch.randn(c2, c1, 4, 4, generator=g, dtype=torch.float64)
    w3 = torch.randn(c3, c2, 4, 4, generator=g, dtype=torch.float64)
    a2 = F.conv2d(a1, w2, None, 2, 1)
    a3 = F.conv2d(F.leaky_relu(a2 * 0.7 + 0.1, 0.1), w3, None, 2, 1)
    for a, sz in ((a2, 16), (a3, 8)):
        tiles = a[0].reshape(-1, 7, sz, 7, sz).permute(1, 3, 0, 2, 4)
        seen = {}
        for p in range(49):
            t = tiles[p // 7, p % 7]
            ref = seen.setdefault(Z.edge_class(p), t)
            assert torch.equal(t, ref), (sz, p)
        assert len(seen) == 9
        flat = [seen[k] for k in sorted(seen)]
        assert all(not torch.equal(flat[i], flat[j]) for i in range(9) for j in range(i))            # the classes do differ
