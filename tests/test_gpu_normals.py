"""GPU: relpose_depth_normals (csrc/normals.hip) against the numpy statements of its contract (tests/normals_model.py) --
count and the nine moments bit for bit, validity and the normal within the backward error of an fp32 Jacobi -- and its uses: the torch
operator, util.depth_normals_dev / depth_normals, and RelativePosePipeline.prepare(rgb, None, depth, ...)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import normals_model as M
from gpu_util import log
from relativepose_amd import synth, weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MIN_NEIGHBORS = 6


def _views(kind, dataset, h, seed):
    if kind == "holes":
        return M.room(dataset, h, seed, hole_frac=0.05)[0]
    if kind == "sparse":
        return M.sparse_scannet_view(h, seed)[0]
    return np.zeros((1, h, 4 * h), np.float32)


# name -> (dataset, h, r, [(kind, seed, number of views taken)]): the shapes at which the kernel can still go wrong
CASES = {
    # 4h = 80 is no multiple of the tile width and the halo of the second tile wraps around the ring inside it
    "suncg_h20_r4": ("suncg", 20, 4, [("holes", 21, 1)]),
    "matterport_h32_r1": ("matterport", 32, 1, [("holes", 22, 2), ("zero", 0, 1)]),
    "scannet_h32_r2": ("scannet", 32, 2, [("holes", 23, 2), ("sparse", 24, 1)]),
    "suncg_h32_r2": ("suncg", 32, 2, [("holes", 25, 2), ("zero", 0, 1)]),
    "matterport_h48_r3": ("matterport", 48, 3, [("holes", 26, 2)]),
    "scannet_h48_r3": ("scannet", 48, 3, [("sparse", 27, 2)]),
}


def _abi(depth_dev, dataset, r, gate_scale=3.0, min_neighbors=MIN_NEIGHBORS):
    """The C ABI called directly, every stage output requested."""
    import torch
    from relativepose_amd import _lib, util
    n, h, w = depth_dev.shape
    dev = depth_dev.device
    out = {"normal": torch.full((n, 3, h, w), 7.0, dtype=torch.float32, device=dev), "valid": torch.full((n, h, w), 9, dtype=torch.uint8, device=dev),
           "count": torch.full((n, h, w), -1, dtype=torch.int32, device=dev), "moments": torch.full((n, 9, h, w), 7.0, dtype=torch.float32, device=dev)}
    a = _lib.DepthNormalsArgs()
    a.struct_size = C.sizeof(a)
    a.n_views, a.h, a.dataset, a.radius, a.min_neighbors, a.gate_scale = n, h, util.dataset_id(dataset), r, min_neighbors, gate_scale
    a.depth = _lib.ptr(depth_dev)
    a.normal, a.valid, a.count, a.moments = (_lib.ptr(out[k]) for k in ("normal", "valid", "count", "moments"))
    a.stream = _lib.stream_ptr()
    assert _lib.lib().relpose_depth_normals(C.byref(a)) == 0
    torch.cuda.synchronize()
    return out


_cache = {}


def _case(name):
    """(depth numpy, depth on the device, model32, model64, the C ABI's outputs), computed once per case and never modified."""
    import torch
    if name not in _cache:
        dataset, h, r, parts = CASES[name]
        dep = np.ascontiguousarray(np.concatenate([_views(kind, dataset, h, seed)[:k] for kind, seed, k in parts]))
        m32 = M.model32(dep, dataset, r)
        m64 = M.model64(m32, MIN_NEIGHBORS)
        dd = torch.from_numpy(dep).cuda()
        _cache[name] = (dep, dd, m32, m64, _abi(dd, dataset, r))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_count_and_moments_equal_the_model_bitwise(name):
    dep, _, m32, _, got = _case(name)
    assert np.array_equal(got["count"].cpu().numpy(), m32["count"])
    mo = got["moments"].cpu().numpy()
    for k in range(9):
        assert np.array_equal(mo[:, k].view(np.uint32), m32["moments"][:, k].view(np.uint32)), k
    assert m32["count"].max() > MIN_NEIGHBORS and (m32["count"][dep == 0] == 0).all() and np.abs(m32["moments"]).max() > 0


@pytest.mark.parametrize("name", CASES)
def test_valid_and_normals_agree_with_float64(name):
    """valid: equal to model64's except where l1 - 1e-6 l2 lies within 64 * 2^-24 * l2 of zero (at most 0.5 % of the pixels).
    normal: within 64 * 2^-24 * l2 / (l1 - l0) + 1e-6 rad of model64's -- the backward error of an fp32 Jacobi with margin, the moments
    being the model's bit for bit; pixels whose bound exceeds 0.05 rad are left out (at most 1 % of the valid pixels)."""
    dep, _, m32, m64, got = _case(name)
    lam = m64["lam"]
    decided = (dep != 0) & (m32["count"] >= MIN_NEIGHBORS)              # elsewhere valid is 0 whatever the eigenvalues are
    close = decided & (np.abs(lam[..., 1] - 1e-6 * lam[..., 2]) <= 64 * U * lam[..., 2])
    share = close.mean()
    valid = got["valid"].cpu().numpy()
    assert set(np.unique(valid)) <= {0, 1}
    valid = valid.astype(bool)
    assert share <= 0.005
    assert np.array_equal(valid[~close], m64["valid"][~close])
    nrm = got["normal"].cpu().numpy()
    assert (nrm[:, 0][~valid] == 0).all() and (nrm[:, 1][~valid] == 0).all() and (nrm[:, 2][~valid] == 0).all()
    both = valid & m64["valid"]
    assert both.sum() > 100
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = lam[..., 1] - lam[..., 0]
        bound = np.where(gap > 0, 64 * U * lam[..., 2] / gap, np.inf) + 1e-6
    out = both & ~(bound <= 0.05)
    assert out.sum() <= 0.01 * both.sum()
    sel = both & ~out
    ang = M.angle(nrm, m64["normal"])
    worst = float((ang[sel] / bound[sel]).max())
    cond = float((lam[..., 2][sel] / gap[sel]).max())
    print(f"{name}: share near the collinearity threshold {share:.2e}, {int(sel.sum())} normals, {int(out.sum())} left out, "
          f"max angle / bound {worst:.3f}, max l2 / (l1 - l0) {cond:.1f}")
    log("depth_normals_vs_float64", case=name, near_threshold_share=share, checked=int(sel.sum()), left_out=int(out.sum()), worst_ratio=worst)
    assert (ang[sel] <= bound[sel]).all()
    ln = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert np.abs(ln[valid] - 1).max() <= 1e-6
    assert ((np.moveaxis(nrm, 1, -1).astype(np.float64) * m32["P"]).sum(-1)[valid] < 0).all()


@pytest.mark.parametrize("name", CASES)
def test_results_do_not_depend_on_the_batch(name):
    import torch
    dataset, h, r, _ = CASES[name]
    _, dd, _, _, got = _case(name)
    for i in range(dd.shape[0]):
        alone = _abi(dd[i:i + 1].contiguous(), dataset, r)
        for k in alone:
            assert torch.equal(alone[k][0], got[k][i]), (i, k)


@pytest.mark.parametrize("name", ["suncg_h20_r4", "scannet_h32_r2"])
def test_operator_and_shims_return_what_the_abi_wrote(name):
    import torch
    from relativepose_amd import ops, util  # noqa: F401
    dataset, h, r, _ = CASES[name]
    dep, dd, _, _, got = _case(name)
    nrm, valid = torch.ops.relpose.depth_normals(dd, util.dataset_id(dataset), r, 3.0, MIN_NEIGHBORS)
    assert torch.equal(nrm, got["normal"]) and torch.equal(valid, got["valid"]) and valid.dtype == torch.uint8
    res = util.depth_normals_dev(dd, dataset, radius=r, stages=True)
    assert len(res) == 4 and all(torch.equal(a, got[k]) for a, k in zip(res, ("normal", "valid", "count", "moments")))
    assert res[2].dtype == torch.int32 and res[3].shape == (dd.shape[0], 9, h, 4 * h)
    buf = torch.zeros_like(got["normal"])
    two = util.depth_normals_dev(dd, dataset, radius=r, out=buf)
    assert len(two) == 2 and two[0] is buf and torch.equal(buf, got["normal"])
    # the host shim: numpy [h,4h] and [B,2,h,4h] in, the dataset dict's `norm` layout out
    one = util.depth_normals(dep[0], dataset, radius=r)
    assert one.shape == (3, h, 4 * h) and one.dtype == np.float32 and np.array_equal(one, got["normal"][0].cpu().numpy())
    two_views = np.stack([dep[0], dep[-1]])[None]
    pair = util.depth_normals(two_views, dataset, radius=r)
    assert pair.shape == (1, 2, 3, h, 4 * h) and np.array_equal(pair[0], got["normal"][[0, -1]].cpu().numpy())
    with pytest.raises(ValueError):
        util.depth_normals(dep, dataset)                                        # [n,h,4h] is neither layout
    # other thresholds reach the kernel: a stricter neighbour count can only take pixels away
    strict = _abi(dd, dataset, r, min_neighbors=(2 * r + 1) ** 2 - 1)
    assert torch.equal(strict["count"], got["count"]) and (strict["valid"] <= got["valid"]).all() and strict["valid"].sum() < got["valid"].sum()
    tight = _abi(dd, dataset, r, gate_scale=0.5)                                # a gate of half the window's reach: the outer ring is gone
    assert np.array_equal(tight["count"].cpu().numpy(), M.model32(dep, dataset, r, 0.5)["count"])
    assert (tight["count"] <= got["count"]).all() and tight["count"].sum() < got["count"].sum()


def test_pipeline_estimates_the_normals_it_is_not_given():
    """B = 2 suncg pairs at 160x640: prepare(rgb, None, depth, ...) holds the estimated normals, its poses are those of a run prepared with that
    array passed as `norm`, also through keep_host + upload_inputs (which uploads no normals); a given `norm` is used as uploaded."""
    import torch
    from cases import E2E_WEIGHT_SEED
    from relativepose_amd import rputil, util
    from relativepose_amd.model import SCNet
    from relativepose_amd.pipeline import RelativePosePipeline
    dev = torch.device("cuda:0")
    ds, mm, S, tanh = "suncg", "second", 15, 1
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=tanh, skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(weights.make_state_dict(E2E_WEIGHT_SEED, S))
    pipe = RelativePosePipeline(net, ds, mm)
    d = synth.make_pairs(2, 1700, ds)
    pts, ptw = synth.make_keypoints(2, 60, 1700, mm)
    B, h, w = 2, 160, 640
    est, est_valid = util.depth_normals_dev(torch.from_numpy(d["depth"].reshape(2 * B, h, w)).to(dev), ds)
    assert est_valid.float().mean() > 0.9

    st = pipe.prepare(d["rgb"], None, d["depth"], pts, ptw, dev)
    assert torch.equal(st["norm"], est)
    pose, status, _ = pipe.run(st)
    given = est.cpu().numpy().reshape(B, 2, 3, h, w)
    st_g = pipe.prepare(d["rgb"], given, d["depth"], pts, ptw, dev, keep_host=True)
    # a given array is what the state holds and what upload_inputs uploads: the parent commit's code path, no estimate is read
    assert "normals_dataset" not in st_g and torch.equal(st_g["norm"], est) and set(st_g["host"]) == {"rgb", "norm", "depth", "pts"}
    assert torch.equal(st_g["host"]["norm"], est.cpu())
    pose_g, status_g, _ = pipe.run(st_g)
    assert torch.equal(pose, pose_g) and torch.equal(status, status_g)
    other = (0.5 * given + 0.1).astype(np.float32)
    st_o = pipe.prepare(d["rgb"], other, d["depth"], pts, ptw, dev)
    assert "normals_dataset" not in st_o and torch.equal(st_o["norm"], torch.from_numpy(other.reshape(2 * B, 3, h, w)).to(dev))

    st_h = pipe.prepare(d["rgb"], None, d["depth"], pts, ptw, dev, keep_host=True)
    assert set(st_h["host"]) == {"rgb", "depth", "pts"}                  # 3/7 fewer panorama bytes cross PCIe
    for copy_stream in (None, torch.cuda.Stream()):
        torch.cuda.synchronize()
        for k in ("rgb", "depth", "pts", "norm"):                        # whatever is on the device now must not matter
            st_h[k].zero_()
        pipe.upload_inputs(st_h, copy_stream)
        pose_h, status_h, _ = pipe.run(st_h)
        assert torch.equal(st_h["norm"], est)
        assert torch.equal(pose_h, pose) and torch.equal(status_h, status)

    # keypoints="reference" takes the same route
    pipe_r = RelativePosePipeline(net, ds, mm, keypoints="reference")
    dets = synth.make_sift_detections(B, 40, 5, mm, h)
    sift = [(rputil.map_detections(a, mm, h), rputil.map_detections(c, mm, h)) for a, c in dets]
    st_r = pipe_r.prepare(d["rgb"], None, d["depth"], None, None, dev, sift=sift, keep_host=True)
    assert torch.equal(st_r["norm"], est) and set(st_r["host"]) == {"rgb", "depth"} and st_r["normals_dataset"] == ds
