"""numpy model of SCNet's conv4 row lists (csrc/scnet.hip: conv4_row_list_kernel, conv_igemm_kernel<ROWS>).

conv4's K slice q is stream block q of A3, so a row of slice q's partial sums depends on stream q only.  Output pixel (oy, ox) of the
28 x 28 grid reads (inclusive, before clipping)
  A3 rows 2oy - 1 .. 2oy + 2,  A2 rows 4oy - 3 .. 4oy + 6,  A1 rows 8oy - 7 .. 8oy + 14,  X0 rows 8oy - 8 .. 8oy + 15
which are exactly the 8-pixel occupancy blocks oy - 1 .. oy + 1 (the same in x): the test is exact, there is no margin.  Only o = 0 and
o = 27 ever see zero padding, at any of the four layers, so a row whose 3 x 3 blocks are empty computes partial sums that depend on its
edge class only (first / last / other row x column).  Per BatchNorm group, slice and class the lowest-index such row is computed (the
representative); the split-K reduce reads the others' sums from it through a row map.
"""
import numpy as np

import zero_tiles_model as Z

N = 28                      # conv4's output grid = the occupancy grid
HW = N * N
THETA_1024 = 717            # a slice takes the row-list launch iff rows listed * 1024 < THETA_1024 * rows (scnet.hip C4R_THETA_1024)


def field_rows(o):
    """Exact X0 rows [lo, hi] (inclusive, unclipped) in the receptive field of conv4 output row o."""
    return 8 * o - 8, 8 * o + 15


def block_range(o):
    """Occupancy blocks [lo, hi) of output row / column o."""
    return max(o - 1, 0), min(o + 2, N)


def edge_class(oy, ox):
    cls = lambda i: 0 if i == 0 else (2 if i == N - 1 else 1)
    return 3 * cls(oy) + cls(ox)


def redundant(occ, nonfinite):
    """occ [n, 6, 28, 28] bool, nonfinite [n, 6] bool (zero_tiles_model.occupancy) -> red [n, 6, 28, 28] bool.  A non-finite value
    anywhere in a BatchNorm group's stream makes that group's {scale, shift} NaN: nothing of that group and stream is redundant."""
    n = occ.shape[0]
    pad = np.zeros((n, 6, N + 2, N + 2), bool)
    pad[:, :, 1:-1, 1:-1] = occ
    any3 = np.zeros_like(occ)
    for dy in range(3):
        for dx in range(3):
            any3 |= pad[:, :, dy:dy + N, dx:dx + N]
    bad = nonfinite.reshape(n // 2, 2, 6).any(1)
    return ~any3 & ~np.repeat(bad, 2, 0)[:, :, None, None]


def row_lists(red_q):
    """red_q [nimg, 28, 28] bool, one slice.  -> (lists, rowmap): lists[g] the ascending rows of group g to compute (rows are indices
    img * 784 + oy * 28 + ox), rowmap [nimg * 784] the row whose partial sums stand for each row (itself, or its representative)."""
    nimg = red_q.shape[0]
    flat = red_q.reshape(nimg * HW)
    rowmap = np.arange(nimg * HW)
    lists = []
    for g in range(nimg // 2):
        rep, lst = {}, []
        for m in range(2 * g * HW, (2 * g + 2) * HW):
            rem = m % HW
            c = edge_class(rem // N, rem % N)
            if flat[m] and c in rep:
                rowmap[m] = rep[c]
                continue
            if flat[m]:
                rep[c] = m
            lst.append(m)
        lists.append(lst)
    return lists, rowmap


def plan_slices(plan, n):
    """Images whose rows K slice q has in a plan: 'full'; 'zero_warp' (the warped slices are shared: the first image pair's rows serve
    every pair); 'self_cached' (the self slices are not computed: 0)."""
    if plan == "full":
        return [n] * 6
    if plan == "zero_warp":
        return [n, 2] * 3
    if plan == "self_cached":
        return [0, n] * 3
    raise ValueError(plan)


def counts(x0, plan="full", mode=0):
    """What SCNet.conv4_rows() reports for a forward over x0 [n, 224, 224, 16]: per slice (rows computed, rows dropped, list path).
    mode = RELPOSE_TUNE_CONV4_ROWS: 0 = list path where the list is sparser than theta, 2 = list path for every finite slice."""
    n = x0.shape[0]
    occ, nf = Z.occupancy(x0)
    red = redundant(occ, nf)
    out = []
    for q, nimg in enumerate(plan_slices(plan, n)):
        if nimg == 0:
            out.append((0, 0, False))
            continue
        rows = nimg * HW
        listed = sum(len(l) for l in row_lists(red[:nimg, q])[0])
        # (a stream with a non-finite value stays on the strip kernel in either mode: its NaN rows keep the kernel that always computed them)
        lp = not nf[:nimg, q].any() and (mode == 2 or listed * 1024 < THETA_1024 * rows)
        out.append((listed, rows - listed, True) if lp else (rows, 0, False))
    return out
