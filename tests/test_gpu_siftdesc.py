"""GPU: the SIFT descriptor and rank kernels (csrc/siftdesc.hip: relpose_sift_describe, relpose_sift_rank) against the numpy model of their
contract (tests/siftdesc_model.py) and their uses: rputil.sift_describe_dev / sift_describe_grid_dev,
descriptor.sift_rank_dev / evalSiftDescriptor, torch.ops.relpose.sift_describe / sift_rank and evaluation --descriptor-eval --sift-baseline.
Reference: mainPanoCompletion2view.py:353-381."""
import json

import numpy as np
import pytest

import siftdesc_model as M
from gpu_util import log

pytestmark = pytest.mark.gpu
F = np.float32


def random_blobs(rs, h, w, n):
    """A texture of n random Gaussian blobs (both signs, std 1.5-6 px) on a mid-grey background, uint8 [h, w] (as in test_gpu_sift.py)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 128.0)
    for _ in range(n):
        cx, cy, s, a = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(1.5, 6.0), rs.uniform(-90, 90)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _describe(images, kp, count=None, crop=None, **kw):
    from relativepose_amd import rputil
    r = rputil.sift_describe_dev(images, crop, kp, count, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _grid(images, step, crop=None, **kw):
    from relativepose_amd import rputil
    r = rputil.sift_describe_grid_dev(images, crop, step, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- G1 base image
def test_base_image_equals_the_model_bitwise():
    rs = np.random.RandomState(0)
    gray = rs.randint(0, 256, (3, 32, 48)).astype(np.uint8)
    got = _describe(gray, np.zeros((3, 0, 4), F), want_base=True)
    assert got["desc"].shape == (3, 0, 128) and np.array_equal(_bits(got["base"]), _bits(M.base_image(gray)))
    bgr = rs.randint(0, 256, (1, 50, 160, 3)).astype(np.uint8)
    crop = (17, 9, 128, 32)
    got = _describe(bgr, np.array([[[60, 16, 5, -1]]], F), crop=crop, want_base=True)
    ref = M.base_image(np.stack([M.gray_of(bgr[0])])[:, 9:41, 17:145])
    assert got["base"].shape == (1, 32, 128) and np.array_equal(_bits(got["base"]), _bits(ref))
    assert got["desc"][0, 0].any()


# ----------------------------------------------------------------------------------------------------------------- G2 descriptors
def _keypoints(h, w, seed):
    """Integer, fractional and x.5 positions; points 0-3 px from each border and in the corners; sizes {2, 5, 12.3} and angles
    {-1, 0, 77.7, 359.9} cycled over them; a NaN slot, an infinite one and slots with size 0 / negative size."""
    rs = np.random.RandomState(seed)
    xy = [(w // 2, h // 2), (w // 3, h // 4), (w / 2 + 0.3, h / 2 - 0.7), (w / 3 + 0.25, h / 3 + 0.8), (10.5, 11.5), (w / 2 + 0.5, 12.5), (13.5, h / 2)]
    for d in range(4):
        xy += [(d, h // 2), (w - 1 - d, h // 2 + 0.4), (w // 2 + 0.6, d), (w // 2, h - 1 - d)]
    xy += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1.5, 1.5), (w - 2.5, h - 1.5), (-2, 5), (w + 1.2, h + 0.7)]
    xy += [tuple(p) for p in rs.uniform((0, 0), (w, h), (9, 2))]
    sizes, angles = (2, 5, 12.3), (-1, 0, 77.7, 359.9)
    kp = [(x, y, sizes[i % 3], angles[(i // 3) % 4]) for i, (x, y) in enumerate(xy)]
    kp += [(w // 2, h // 2, s, a) for s in sizes for a in angles]
    kp += [(np.nan, 5, 5, -1), (7, np.inf, 5, -1), (w // 2, h // 2, 0, -1), (w // 2, h // 2, -5, -1), (w // 2, h // 2, np.nan, -1)]
    return np.array(kp, F)


@pytest.fixture(scope="module")
def describe_cases():
    """Per image size: the blob textures (view 1 has count 0), the keypoints, the kernel's outputs and the model's."""
    out = {}
    for h, w, n in ((32, 48, 40), (96, 160, 300)):
        rs = np.random.RandomState(h)
        img = np.stack([random_blobs(rs, h, w, n), random_blobs(rs, h, w, n)])
        kp = np.stack([_keypoints(h, w, 1), _keypoints(h, w, 2)])
        count = np.array([kp.shape[1], 0], np.int32)
        got = _describe(img, kp, count, want_f32=True)
        u, desc, _ = M.describe(img, kp, count)
        out[h, w] = dict(img=img, kp=kp, count=count, got=got, u=u, desc=desc)
    return out


@pytest.mark.parametrize("shape", [(32, 48), (96, 160)])
def test_descriptors_match_the_model(describe_cases, shape):
    """|desc_f32 - u_model| <= 0.02: a bin is a sum of at most ~900 non-negative float32 terms, relative error at most 900 * 2^-24 = 5.4e-5,
    which scales to at most 255 * 5.4e-5 = 0.014; exp / atan2 / sqrt add ~1e-6 relative."""
    c = describe_cases[shape]
    got, u = c["got"], c["u"]
    n_kp = c["kp"].shape[1]
    err = np.abs(got["desc_f32"].astype(np.float64) - u)
    log("siftdesc_vs_model", shape=shape, n_kp=n_kp, max_abs_err=err.max(), u_max=u.max(),
        desc_mismatch=int((got["desc"] != c["desc"]).sum()), desc_max_diff=int(np.abs(got["desc"].astype(int) - c["desc"]).max()))
    print("siftdesc max |desc_f32 - u_model|", shape, err.max())
    assert err.max() <= 0.02                                                                                  # (a)
    assert np.array_equal(got["desc"], np.clip(np.rint(got["desc_f32"]), 0, 255).astype(np.uint8))            # (b)
    used = u[0].any(1)
    assert used[:n_kp - 5].sum() >= n_kp - 7 and not used[n_kp - 5:].any()           # (only the two points outside the image may be empty)
    assert not got["desc"][0, ~used].any() and not got["desc_f32"][0, ~used].any()                            # (c) NaN / inf / size <= 0
    assert not got["desc"][1].any() and not got["desc_f32"][1].any()                                          # (c) a view with count 0
    assert got["desc_f32"][0, used].any(1).all()
    assert np.abs(np.linalg.norm(got["desc_f32"][0, used].astype(np.float64), axis=1) - 512.0).max() < 0.01


def test_no_keypoints():
    img = random_blobs(np.random.RandomState(3), 32, 48, 20)[None]
    got = _describe(img, np.zeros((1, 0, 4), F), want_f32=True)
    assert got["desc"].shape == got["desc_f32"].shape == (1, 0, 128)


@pytest.mark.parametrize("step", [1, 5, 7])
def test_grid_mode_equals_explicit_keypoints_bitwise(step):
    rs = np.random.RandomState(step)
    bgr = rs.randint(0, 256, (2, 40, 70, 3)).astype(np.uint8)
    crop = (3, 5, 50, 33)
    g = M.grid_keypoints(50, 33, step)
    a = _grid(bgr, step, crop=crop, want_f32=True, want_base=True)
    b = _describe(bgr, np.stack([g, g]), crop=crop, want_f32=True, want_base=True)
    assert a["desc"].shape == (2, len(g), 128) and a["desc"].any()
    assert np.array_equal(a["desc"], b["desc"]) and np.array_equal(_bits(a["desc_f32"]), _bits(b["desc_f32"]))
    assert np.array_equal(_bits(a["base"]), _bits(b["base"]))


# ----------------------------------------------------------------------------------------------------------------- G3 reproducibility
def test_bitwise_reproducible_batch_and_slot_independent(describe_cases):
    c = describe_cases[32, 48]
    rs = np.random.RandomState(7)
    img = np.concatenate([c["img"], np.stack([random_blobs(rs, 32, 48, 40) for _ in range(3)])])
    kp = np.stack([_keypoints(32, 48, s) for s in range(1, 6)])
    a, a2 = _describe(img, kp, want_f32=True), _describe(img, kp, want_f32=True)
    assert np.array_equal(a["desc"], a2["desc"]) and np.array_equal(_bits(a["desc_f32"]), _bits(a2["desc_f32"]))
    assert np.array_equal(_bits(a["desc_f32"][0]), _bits(c["got"]["desc_f32"][0]))                # view 0 inside the batch of 2 and of 5
    for v in range(5):
        s = _describe(img[v:v + 1], kp[v:v + 1], want_f32=True)
        assert np.array_equal(s["desc"][0], a["desc"][v]) and np.array_equal(_bits(s["desc_f32"][0]), _bits(a["desc_f32"][v])), v
    perm = rs.permutation(kp.shape[1])
    p = _describe(img, kp[:, perm], want_f32=True)                                                # other slots, other neighbours
    assert np.array_equal(_bits(p["desc_f32"]), _bits(a["desc_f32"][:, perm]))
    few = _describe(img[2:3], kp[2:3, 5:8], want_f32=True)
    assert np.array_equal(_bits(few["desc_f32"][0]), _bits(a["desc_f32"][2, 5:8]))


# ----------------------------------------------------------------------------------------------------------------- G4 rank
def _rank(src, tgt, dense, pv=None):
    from relativepose_amd import descriptor
    c, t = descriptor.sift_rank_dev(src, tgt, dense, pv)
    return c.cpu().numpy(), t.cpu().numpy()


def _rank_case(E, P, seed):
    rs = np.random.RandomState(seed)
    src, tgt, dense = (rs.randint(0, 256, (3, n, 128)).astype(np.uint8) for n in (E, E, P))
    # descriptor-like neighbours, so that the counts are neither 0 nor P: some grid rows near a source row, some far
    near = rs.randint(0, E, (3, P))
    noise = rs.randint(-40, 41, (3, P, 128))
    keep = rs.rand(3, P) < 0.5
    dense = np.where(keep[:, :, None], np.clip(np.take_along_axis(src, near[:, :, None], 1).astype(int) + noise, 0, 255), dense).astype(np.uint8)
    src[0, 0, :5], src[0, 0, 5:9], dense[0, 0, :7] = 0, 255, 255                        # the extreme byte values
    dense[0, -1], tgt[2, -1] = 0, 255
    tgt[0, E // 2] = src[0, E // 2]                                                      # thr 0: nothing is closer
    dense[2, P // 2] = tgt[2, 0]                                                         # a tie with the true match: not counted
    return src, tgt, dense


@pytest.mark.parametrize("E,P", [(1, 1), (37, 182), (64, 4096), (100, 33)])
def test_rank_counts_are_exact(E, P):
    src, tgt, dense = _rank_case(E, P, E + P)
    pv = np.array([1, 0, 1], np.uint8)
    count, thr = _rank(src, tgt, dense, pv)
    rc, rt = M.rank_int(src, tgt, dense, pv)
    assert count.dtype == thr.dtype == np.int32
    assert np.array_equal(thr, rt) and np.array_equal(count, rc)
    assert (count[1] == -1).all() and (thr[1] == -1).all() and thr[0, E // 2] == 0 and count[0, E // 2] == 0
    cf, df = M.rank_f32(src[2], tgt[2], dense[2])                                        # the reference's float32 expression
    assert np.array_equal(cf, count[2]) and np.array_equal(df.astype(np.int64), thr[2])
    if P > 1:
        assert 0 < count[[0, 2]].max() and count[[0, 2]].min() < P and len(np.unique(count[[0, 2]])) > min(E, 3) - 1
    log("sift_rank_exact", E=E, P=P, count_min=count[[0, 2]].min(), count_max=count[[0, 2]].max())
    c2, t2 = _rank(src, tgt, dense, pv)                                                  # repeat
    assert np.array_equal(c2, count) and np.array_equal(t2, thr)
    ca, ta = _rank(src, tgt, dense)                                                      # no validity vector: every pair counts
    ra, _ = M.rank_int(src, tgt, dense)
    assert np.array_equal(ca, ra) and np.array_equal(ca[[0, 2]], count[[0, 2]])
    for b in (0, 2):                                                                     # a pair alone
        c1, t1 = _rank(src[b:b + 1], tgt[b:b + 1], dense[b:b + 1])
        assert np.array_equal(c1[0], count[b]) and np.array_equal(t1[0], thr[b])


# ----------------------------------------------------------------------------------------------------------------- G5 metric
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device()))


def test_eval_sift_descriptor_equals_its_composition():
    from relativepose_amd import descriptor, rputil, synth
    d = synth.make_pairs(3, 500, "suncg", h=32)
    depth = _t(d["depth"].reshape(6, 32, 128))
    dc = descriptor.dense_correspondences(depth, d["R"].reshape(6, 4, 4), "suncg", np.random.RandomState(11))
    assert dc["valid"].tolist() == [1, 1, 1]
    dc = dict(dc, valid=np.array([1, 0, 1]))
    got = descriptor.evalSiftDescriptor(d["rgb"], dc, np.random.RandomState(4))
    rng = np.random.RandomState(4)
    u8, _ = rputil.sift_images(d["rgb"], "second")
    ref = []
    for b in range(3):
        if dc["valid"][b] == 0:
            continue
        idx = rng.choice(range(2000), 100)                                               # mainPanoCompletion2view.py:360
        kp = lambda xy: np.concatenate([xy, np.full((100, 1), 5.0), np.full((100, 1), -1.0)], 1).astype(F)[None]
        sifts = rputil.sift_describe_dev(u8[2 * b:2 * b + 1], None, kp(dc["idxSrc"][b][idx]))["desc"]
        siftt = rputil.sift_describe_dev(u8[2 * b + 1:2 * b + 2], None, kp(dc["idxTgt"][b][idx]))["desc"]
        dense = rputil.sift_describe_grid_dev(u8[2 * b + 1:2 * b + 2], None, 5)["desc"]
        assert dense.shape == (1, 182, 128)
        count, thr = descriptor.sift_rank_dev(sifts, siftt, dense)
        cf, df = M.rank_f32(sifts[0].cpu().numpy(), siftt[0].cpu().numpy(), dense[0].cpu().numpy())   # :373, :378-379
        assert np.array_equal(cf, count[0].cpu().numpy())
        ratio = cf / 182                                                                 # :379
        ref.append(ratio.mean())
    assert len(got) == 2 and got == ref and all(isinstance(g, float) and 0.0 <= g <= 1.0 for g in got)
    log("eval_sift_descriptor", ratios=got)


def test_identical_views_give_ratio_zero():
    from relativepose_amd import descriptor, synth
    d = synth.make_pairs(2, 501, "suncg", h=32)
    rgb = d["rgb"].copy()
    rgb[:, 1] = rgb[:, 0]
    rs = np.random.RandomState(0)
    idx = np.stack([rs.randint(0, 128, (2, 300)), rs.randint(0, 32, (2, 300))], -1).astype(np.float64)
    got = descriptor.evalSiftDescriptor(rgb, {"idxSrc": idx, "idxTgt": idx, "valid": np.ones(2, np.int64)}, np.random.RandomState(1))
    assert got == [0.0, 0.0]


def test_shifted_view_gives_ratio_zero():
    """The target is the source moved by whole pixels (dx, dy) = (4, -3); both end points of every correspondence lie >= 40 px from every
    border, further than the descriptor's reach (radius 27 + 1 gradient pixel + 6 blur taps): the two descriptors are bitwise equal."""
    from relativepose_amd import descriptor, rputil
    rs = np.random.RandomState(5)
    g = random_blobs(rs, 96, 160, 300).astype(np.float32) / 255.0
    src = np.stack([g, np.roll(g, 1, 0), np.roll(g, 2, 1)])                              # three different channels
    tgt = np.roll(src, (-3, 4), (1, 2))
    rgb = np.stack([src, tgt])[None]                                                     # [1, 2, 3, 96, 160]
    xs, ys = rs.randint(40, 116, 400), rs.randint(43, 56, 400)
    dc = {"idxSrc": np.stack([xs, ys], -1)[None].astype(np.float64), "idxTgt": np.stack([xs + 4, ys - 3], -1)[None].astype(np.float64),
          "valid": np.ones(1, np.int64)}
    assert min(dc["idxTgt"][0, :, 0].min(), dc["idxTgt"][0, :, 1].min(), 159 - dc["idxTgt"][0, :, 0].max(), 95 - dc["idxTgt"][0, :, 1].max()) >= 40
    u8, _ = rputil.sift_images(rgb, "second")
    kp = lambda xy: np.concatenate([xy, np.full((400, 1), 5.0), np.full((400, 1), -1.0)], 1).astype(F)[None]
    a = rputil.sift_describe_dev(u8[0:1], None, kp(dc["idxSrc"][0]), want_f32=True)
    b = rputil.sift_describe_dev(u8[1:2], None, kp(dc["idxTgt"][0]), want_f32=True)
    assert bool(a["desc"].any()) and np.array_equal(_bits(a["desc_f32"].cpu().numpy()), _bits(b["desc_f32"].cpu().numpy()))
    assert descriptor.evalSiftDescriptor(rgb, dc, np.random.RandomState(2)) == [0.0]


# ----------------------------------------------------------------------------------------------------------------- G6 operators and CLI
def test_torch_ops_match_the_python_api_and_meta_shapes():
    import torch
    from relativepose_amd import descriptor, ops, rputil  # noqa: F401
    rs = np.random.RandomState(9)
    img = _t(rs.randint(0, 256, (2, 40, 70, 3)).astype(np.uint8))
    kp = _t(np.stack([_keypoints(33, 50, 1), _keypoints(33, 50, 2)]))
    cnt = _t(np.array([20, 7], np.int32))
    crop = [3, 5, 50, 33]
    d, f = torch.ops.relpose.sift_describe(img, crop, kp, cnt)
    r = rputil.sift_describe_dev(img, crop, kp, cnt, want_f32=True)
    assert torch.equal(d, r["desc"]) and torch.equal(f.view(torch.int32), r["desc_f32"].view(torch.int32)) and bool(d.any())
    d, f = torch.ops.relpose.sift_describe(img, [], kp.new_empty(0), None, 5)
    r = rputil.sift_describe_grid_dev(img, None, 5, want_f32=True)
    assert d.shape == (2, 14 * 8, 128) and torch.equal(d, r["desc"]) and torch.equal(f.view(torch.int32), r["desc_f32"].view(torch.int32))
    src, tgt, dense = (_t(x) for x in _rank_case(37, 182, 3))
    pv = _t(np.array([1, 1, 0], np.uint8))
    a, b = torch.ops.relpose.sift_rank(src, tgt, dense, pv), descriptor.sift_rank_dev(src, tgt, dense, pv)
    assert len(a) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    m = lambda t: torch.empty_like(t, device="meta")
    md, mf = torch.ops.relpose.sift_describe(m(img), crop, m(kp), m(cnt))
    assert md.shape == mf.shape == (2, kp.shape[1], 128) and (md.dtype, mf.dtype) == (torch.uint8, torch.float32)
    md, _ = torch.ops.relpose.sift_describe(m(img), [], m(kp.new_empty(0)), None, 5)
    assert md.shape == (2, 112, 128)
    mc, mt = torch.ops.relpose.sift_rank(m(src), m(tgt), m(dense), m(pv))
    assert mc.shape == mt.shape == (3, 37) and mc.dtype == mt.dtype == torch.int32


def test_evaluation_sift_baseline_adds_ratio_sift(capsys):
    from relativepose_amd import evaluation
    argv = ["--descriptor-eval", "--dataset", "suncg", "--pairs", "4", "--batch", "4"]
    evaluation.main(argv + ["--sift-baseline"])
    evaluation.main(argv)
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2
    with_sift, plain = lines
    assert set(with_sift) == set(plain) | {"ratio_sift"} and "ratio_sift" not in plain
    assert np.isfinite(with_sift["ratio_sift"]) and 0.0 <= with_sift["ratio_sift"] <= 1.0
    assert with_sift["ratio_obs"] == plain["ratio_obs"] and with_sift["ratio_unobs"] == plain["ratio_unobs"]
    assert with_sift["valid_pairs"] == plain["valid_pairs"] > 0
    log("descriptor_eval_sift_baseline", **with_sift)


# ----------------------------------------------------------------------------------------------------------------- G7 cv2
def test_compare_with_cv2_when_installed():
    """Agreement with cv2's descriptors is not part of the contract (DESIGN.md §4.10 lists the known differences): the mean absolute
    element difference is logged."""
    cv2 = pytest.importorskip("cv2")
    rs = np.random.RandomState(0)
    img = random_blobs(rs, 96, 160, 300)
    xy = rs.uniform((30, 30), (130, 66), (50, 2)).astype(F)
    kps = [cv2.KeyPoint(float(x), float(y), 5.0, 0.0) for x, y in xy]
    try:
        sift = cv2.xfeatures2d.SIFT_create()
    except AttributeError:
        sift = cv2.SIFT_create()
    _, ref = sift.compute(img, kps)
    kp = np.concatenate([xy, np.full((50, 1), 5, F), np.zeros((50, 1), F)], 1)[None]
    got = _describe(img[None], kp)["desc"][0].astype(np.float64)
    diff = np.abs(got - ref.astype(np.float64)).mean()
    print("mean |desc - cv2|", diff)
    log("siftdesc_vs_cv2", mean_abs_diff=diff)
