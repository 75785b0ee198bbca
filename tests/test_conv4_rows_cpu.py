"""CPU: the numpy model of conv4's row lists (tests/conv4_rows_model.py) on hand-made occupancy patterns, and the geometry it rests on
checked against a torch-CPU conv stack (conv1 3 x 3 stride 1 pad 1, then three 4 x 4 stride 2 pad 1 convs: X0 224 -> conv4's 28)."""
import numpy as np
import pytest

import conv4_rows_model as M
import zero_tiles_model as Z


def occ_of(blocks, n=2, nonfinite=()):
    """occ [n, 6, 28, 28] with the listed (img, q, by, bx) blocks set; nonfinite: (img, q) pairs."""
    occ = np.zeros((n, 6, M.N, M.N), bool)
    nf = np.zeros((n, 6), bool)
    for img, q, by, bx in blocks:
        occ[img, q, by, bx] = True
    for img, q in nonfinite:
        nf[img, q] = True
    return occ, nf


@pytest.mark.parametrize("by,bx,rows", [(0, 0, 4), (27, 27, 4), (0, 13, 6), (13, 27, 6), (13, 13, 9)])
def test_single_block_lists(by, bx, rows):
    """One occupied block at a corner / an edge / in the interior: its 2 x 2 / 2 x 3 / 3 x 3 rows are computed, and the nine
    representatives (lowest redundant row of each class) beside them."""
    occ, nf = occ_of([(1, 2, by, bx)])
    red = M.redundant(occ, nf)
    assert int((~red[1, 2]).sum()) == rows and red[0].all() and red[1, [0, 1, 3, 4, 5]].all()
    ys, xs = np.nonzero(~red[1, 2])
    assert ys.min() == max(by - 1, 0) and ys.max() == min(by + 1, 27) and xs.min() == max(bx - 1, 0) and xs.max() == min(bx + 1, 27)
    lists, rowmap = M.row_lists(red[:, 2])
    assert len(lists) == 1 and len(lists[0]) == 9 + rows and lists[0] == sorted(lists[0])
    # image 0 is all empty: it holds every representative, each the first row of its class
    reps = {M.edge_class(m // 28, m % 28): m for m in reversed(range(784))}
    assert sorted(reps.values()) == [0, 1, 27, 28, 29, 55, 756, 757, 783]
    assert lists[0][:9] == sorted(reps.values())
    for m in range(2 * 784):
        rem = m % 784
        if m >= 784 and not red[1, 2, rem // 28, rem % 28]:
            assert rowmap[m] == m
        else:
            assert rowmap[m] == reps[M.edge_class(rem // 28, rem % 28)]


def test_representatives_are_per_group_and_lowest():
    # group 1 (images 2, 3): image 2 fully occupied, so its representatives are the first rows of image 3
    occ, nf = occ_of([(2, 0, by, bx) for by in range(28) for bx in range(28)], n=4)
    red = M.redundant(occ, nf)
    lists, rowmap = M.row_lists(red[:, 0])
    assert len(lists[0]) == 9 and len(lists[1]) == 784 + 9
    assert lists[1][784:] == [3 * 784 + r for r in (0, 1, 27, 28, 29, 55, 756, 757, 783)]
    assert rowmap[3 * 784 + 30] == 3 * 784 + 29 and rowmap[784 + 30] == 29 and rowmap[2 * 784 + 30] == 2 * 784 + 30
    # a representative need not be at the class's first position: occupy block (0, 0) of image 0
    occ, nf = occ_of([(0, 1, 0, 0)])
    lists, rowmap = M.row_lists(M.redundant(occ, nf)[:, 1])
    assert lists[0][:6] == [0, 1, 2, 27, 28, 29]            # rows (0, 0), (0, 1), (1, 0), (1, 1) computed; (0, 2) is the top-edge representative
    assert rowmap[3] == 2 and rowmap[784] == 784 and rowmap[785] == 2      # the corner class has no redundant row in image 0: image 1's is its own


def test_nonfinite_group_drops_nothing():
    occ, nf = occ_of([(0, 3, 5, 5)], n=4, nonfinite=[(1, 3)])
    red = M.redundant(occ, nf)
    assert not red[:2, 3].any() and red[2:, 3].all() and red[:2, 2].all()
    x0 = np.zeros((4, 224, 224, 16), np.float32)
    x0[1, 100, 100, 11] = np.inf                              # channel 11 = stream 3 (normals, warped view)
    lists, _ = M.row_lists(red[:, 3])
    assert len(lists[0]) == 2 * 784 and len(lists[1]) == 9
    for mode in (0, 2):
        c = M.counts(x0, mode=mode)
        assert c[3] == (4 * 784, 0, False)                    # the non-finite stream's slice stays on the strip kernel
        assert c[0] == (18, 4 * 784 - 18, True)


def test_counts_threshold_and_plans():
    x0 = np.zeros((4, 224, 224, 16), np.float32)
    x0[..., 0] = 1.0                                          # stream 0 dense
    x0[0, 9, 9, 3] = 2.0                                      # stream 2: one value in block (1, 1)
    c = M.counts(x0)
    assert c[0] == (4 * 784, 0, False)                        # a dense slice stays on the strip kernel: every row computed
    assert c[2] == (18 + 9, 4 * 784 - 27, True) and c[1] == (18, 4 * 784 - 18, True)
    assert M.counts(x0, mode=2)[0] == (4 * 784, 0, True)
    assert M.counts(x0, "zero_warp")[1] == (9, 2 * 784 - 9, True)
    assert M.counts(x0, "self_cached")[0] == (0, 0, False) and M.counts(x0, "self_cached")[1] == c[1]


@pytest.fixture(scope="module")
def stack():
    """conv1 (3 x 3, stride 1) and conv2-4 (4 x 4, stride 2), one channel, small integer weights in float64: every sum is exact, so equal
    fields give equal bits whatever the order of the additions.  conv1 has no bias; the constant added behind it stands for BatchNorm's
    shift (a zero A1 becomes one constant everywhere, the border included; the zero padding of conv2 comes after it)."""
    import torch
    rs = np.random.RandomState(7)
    ws = [torch.from_numpy(rs.randint(1, 4, size=(1, 1, k, k)).astype(np.float64)) for k in (3, 4, 4, 4)]

    def run(x0):
        import torch.nn.functional as F
        a = F.conv2d(torch.from_numpy(x0)[None, None], ws[0], padding=1) + 5.0
        for w in ws[1:]:
            a = F.conv2d(a, w, stride=2, padding=1)
        return a[0, 0].numpy()
    return run


def test_receptive_field_is_three_blocks(stack):
    base = stack(np.zeros((224, 224)))
    assert base.shape == (28, 28)
    pos = (0, 7, 8, 15, 16, 216, 223)
    for y in pos:
        for x in pos:
            x0 = np.zeros((224, 224))
            x0[y, x] = 1.0
            changed = stack(x0) != base
            want = np.zeros((28, 28), bool)
            for oy in range(28):
                for ox in range(28):
                    ylo, yhi = M.block_range(oy)
                    xlo, xhi = M.block_range(ox)
                    lo_y, hi_y = M.field_rows(oy)
                    lo_x, hi_x = M.field_rows(ox)
                    blocks = ylo <= y // 8 < yhi and xlo <= x // 8 < xhi
                    assert blocks == (lo_y <= y <= hi_y and lo_x <= x <= hi_x)       # the block rule is the exact field
                    want[oy, ox] = blocks
            assert np.array_equal(changed, want), (y, x)


def test_constant_region_gives_nine_classes(stack):
    out = stack(np.zeros((224, 224))).view(np.int64)
    by_class = {}
    for oy in range(28):
        for ox in range(28):
            by_class.setdefault(M.edge_class(oy, ox), set()).add(int(out[oy, ox]))
    assert sorted(by_class) == list(range(9))
    assert all(len(v) == 1 for v in by_class.values()), by_class                      # o = 1 and o = 26 see no padding at any layer
    assert len({next(iter(v)) for v in by_class.values()}) == 9


def test_model_on_a_resized_view():
    """The model's counts hang together on a realistic support pattern: a vertical band."""
    x0 = np.zeros((2, 224, 224, 16), np.float32)
    x0[:, :, 56:112, :8] = 1.0
    x0[:, :, 60:100, 8:] = 1.0
    occ, nf = Z.occupancy(x0)
    red = M.redundant(occ, nf)
    assert red[0, 0].sum() == 28 * (28 - 9) and red[0, 1].sum() == 28 * (28 - 8)
    c = M.counts(x0)
    assert c[0] == (2 * 28 * 9 + 9, 2 * 784 - 2 * 28 * 9 - 9, True)        # the band's 9 columns of both images + the nine classes beside it
    assert c[1] == (2 * 28 * 8 + 9, 2 * 784 - 2 * 28 * 8 - 9, True)
