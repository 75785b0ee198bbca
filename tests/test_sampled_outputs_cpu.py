"""CPU: the numpy model of the sampled tail's element set (tests/sampled_model.py) against the oracle's sampling.

The sampled tail of the SCNet forward writes only the elements of the network output that the keypoint sampler loads.  Here the model of
that set is held against what the ORACLE's sampler (oracle/pipeline_oracle.sample_primitives behind geom_oracle.compose) really depends
on: with every element outside the set replaced by NaN the oracle's primitives do not change in a bit (the set is sufficient), and a
NaN in any single element of a keypoint's set reaches that keypoint's primitives (nothing in the set is unread).  The source taps of an
output pixel are held against the oracle network's own output resize (torch bilinear, align_corners=False)."""
import numpy as np
import pytest

from oracle import geom_oracle as G
from oracle import pipeline_oracle as P
from sampled_model import RS, lin_coef, read_mask, resize_out, sample_pixels, source_taps

H, W, S = 160, 640, 15
CF = 7 + S + 32


def edge_keypoints(h):
    """Keypoints at the ends of the sampler's domain, on both sides of every face boundary, inside / outside / on the edge of the observed
    box of the 'second' mask (columns h .. 2h), at integer coordinates, duplicated, and with a feature block that differs from the
    normal / depth block ((xi, yi) != (tx, ty): x * (W - 1) / W falls below the integer x)."""
    w = 4 * h
    p = [(0.0, 0.0), (0.25, 0.75), (w - 2.0, h - 2.0), (w - 1.5, h - 1.25), (w - 1.001, 3.5), (5.5, h - 1.001), (0.5, h - 2.0), (w - 2.0, 0.5)]
    for f in (1, 2, 3):
        p += [(f * h - 1.5, 40.25), (f * h - 1.0, 41.0), (f * h - 0.001, 42.5), (f * h + 0.0, 43.0), (f * h + 0.5, 44.75)]
    p += [(h + 60.5, 80.5), (h - 2.5, 80.5), (2 * h + 1.5, 80.5), (h + 0.0, 0.0), (2 * h - 1.0, h - 2.0)]
    p += [(17.0, 23.0), (300.0, 100.0), (123.25, 77.5), (123.25, 77.5), (123.25, 77.5)]
    p += [(200.0, 100.0), (639.0 * 400 / 640, 159.0 * 80 / 160), (400.0, 80.0)]
    return np.array(p, np.float64)


def keypoints(seed, k, h):
    rs = np.random.RandomState(seed)
    r = np.stack((rs.uniform(0, 4 * h - 1, k), rs.uniform(0, h - 1, k)), 1)
    return np.concatenate((edge_keypoints(h), r))


def oracle_primitives(f, mask, obs_n, obs_d, pts):
    n, d = G.compose(f, mask, obs_n, obs_d)
    pc, nn, des = P.sample_primitives(d, n, f[7 + S:], pts, "suncg")
    return np.concatenate((pc, nn, des.astype(np.float64)), 1)          # [k, 3 + 3 + 32]


@pytest.fixture(scope="module")
def scene():
    rs = np.random.RandomState(5)
    f = rs.uniform(0.5, 1.5, (CF, H, W)).astype(np.float32)
    obs_n = rs.uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
    obs_d = rs.uniform(0.5, 1.5, (H, W)).astype(np.float32)
    mask = np.zeros((H, W, 1), np.float32)
    mask[:, H:2 * H] = 1                                               # the 'second' mask's observed box
    return f, mask, obs_n, obs_d


def test_blocks_differ_and_stay_inside():
    pts = keypoints(1, 400, H)
    tx, ty, xi, yi = sample_pixels(pts, H)
    assert tx.min() == 0 and tx.max() == W - 2 and ty.min() == 0 and ty.max() == H - 2
    assert xi.min() >= 0 and xi.max() <= W - 2 and yi.min() >= 0 and yi.max() <= H - 2
    assert int(((xi != tx) | (yi != ty)).sum()) > 0 and int(((xi == tx) & (yi == ty)).sum()) > 0


def test_the_set_is_what_the_oracle_reads(scene):
    f, mask, obs_n, obs_d = scene
    pts = keypoints(2, 200, H)
    ref = oracle_primitives(f, mask, obs_n, obs_d, pts)
    assert np.isfinite(ref).all()
    m = read_mask(pts[None], [len(pts)], H, S)[0]
    assert not m[:3].any() and not m[7:7 + S].any() and m[3:7].any() and m[7 + S:].any()
    g = np.where(m, f, np.float32(np.nan))
    got = oracle_primitives(g, mask, obs_n, obs_d, pts)
    assert np.array_equal(ref.view(np.int64), got.view(np.int64))        # sufficient: nothing outside the set is read
    # entries k >= npts are not part of the set
    m2 = read_mask(np.concatenate((pts[:10], np.full((5, 2), np.nan)))[None], [10], H, S)[0]
    assert np.array_equal(m2, read_mask(pts[None, :10], [10], H, S)[0])


def test_every_element_of_the_set_is_read(scene):
    f, mask, obs_n, obs_d = scene
    for p in edge_keypoints(H)[[0, 2, 11, 33]]:
        m = read_mask(p[None, None], [1], H, S)[0]
        c, y, x = np.nonzero(m)
        assert len(c) == 4 * 4 + 32 * 4
        for ci, yi, xi in zip(c, y, x):
            g = f.copy()
            g[ci, yi, xi] = np.nan
            assert np.isnan(oracle_primitives(g, mask, obs_n, obs_d, p[None])).any(), (tuple(p), ci, yi, xi)


def test_source_taps_are_the_oracle_resize():
    import torch
    import torch.nn.functional as F
    rs = np.random.RandomState(9)
    v = rs.standard_normal((RS, RS)).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(v)[None, None], [H, W], mode="bilinear", align_corners=False)[0, 0].numpy()
    got = resize_out(v, H, W)
    # float32 sums of four products of O(1) values with weights in [0, 1], evaluated in two orders: a few ulp of 4
    assert np.abs(got - ref).max() < 8 * 2.0 ** -23
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = source_taps(np.arange(H), np.arange(W), H, W)
    assert y0.min() == 0 and y1.max() == RS - 1 and x0.min() == 0 and x1.max() == RS - 1
    assert ((y1 - y0) | 1).max() == 1 and ((x1 - x0) | 1).max() == 1 and (ly0 + ly1 == 1).all() and (lx0 + lx1 == 1).all()
    # a 2 x 2 output block draws on at most 4 x 3 distinct source pixels at this shape (rows shrink by 1.4, columns grow by 2.86)
    ny = max(len({y0[o], y1[o], y0[o + 1], y1[o + 1]}) for o in range(H - 1))
    nx = max(len({x0[o], x1[o], x0[o + 1], x1[o + 1]}) for o in range(W - 1))
    assert (ny, nx) == (4, 3)
    i0, i1, l0, l1 = lin_coef(np.arange(4), 0.25, 8)
    assert list(i0) == [0, 0, 0, 0] and list(i1) == [1, 1, 1, 1] and l1[0] == 0            # src clamps at 0 from below
