"""CPU: the numpy model of the SIFT descriptor contract (tests/siftdesc_model.py) against properties that follow from the
contract, the integer rank expression against the reference's float32 one, and the C ABI / host plumbing of relpose_sift_describe and
relpose_sift_rank without a device.  Reference: mainPanoCompletion2view.py:353-381."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import siftdesc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _texture(h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w)).astype(np.uint8)


def _base(gray):
    return M.base_image(gray[None])[0]


# ----------------------------------------------------------------------------------------------------------------- the model
def test_flat_image_gives_zeros():
    u, desc, base = M.describe(np.full((1, 40, 40), 93, np.uint8), np.array([[[20, 20, 5, -1], [3.3, 7.5, 12.3, 40]]], np.float32))
    assert not u.any() and not desc.any()
    assert (base == base[0, 0, 0]).all()


def test_normalisation_properties():
    g = _texture(48, 64, 1)
    base = _base(g)
    for kp in ([30, 20, 5, -1], [10.4, 11.5, 2, 0], [33, 25, 12.3, 77.7], [2, 2, 5, 359.9]):
        hist = M.histogram(base, np.array(kp, np.float32)).reshape(128)
        assert hist.any() and (hist >= 0).all()
        u, desc = M.normalise(hist)
        assert abs(np.linalg.norm(u) - 512.0) < 1e-9
        v = np.minimum(hist, 0.2 * np.linalg.norm(hist))
        assert u.max() <= 0.2 * 512.0 * (np.linalg.norm(hist) / np.linalg.norm(v)) * (1 + 1e-12)
        assert np.array_equal(desc, np.clip(np.rint(u), 0, 255).astype(np.uint8))


def test_unused_slots_read_zeros():
    g = _texture(32, 48, 2)
    kp = np.array([[[20, 15, 5, -1], [np.nan, 15, 5, -1], [20, np.inf, 5, -1], [20, 15, 0, -1], [20, 15, -3, -1], [20, 15, np.nan, -1],
                    [21, 15, 5, -1]]], np.float32)
    u, desc, _ = M.describe(g[None], kp)
    assert u[0, 0].any() and u[0, 6].any() and not u[0, 1:6].any() and not desc[0, 1:6].any()
    u2, _, _ = M.describe(g[None], kp, count=[1])
    assert np.array_equal(u2[0, 0], u[0, 0]) and not u2[0, 1:].any()


def test_horizontal_ramp_fills_one_orientation_bin_pair():
    """I = 2 x: dx = 4, dy = 0 everywhere (the blur keeps a ramp away from the border), orientation 0 deg; with angle -1 the descriptor
    frame is turned by a = 1 deg, so obin = -1 * 8 / 360 = -0.0222: all mass in orientation bins 7 (weight 0.0222) and 0."""
    x = np.arange(120)
    g = np.broadcast_to((x * 2).astype(np.uint8), (120, 120)).copy()
    base = _base(g)
    hist = M.histogram(base, np.array([60, 60, 5, -1], np.float32))
    per_o = hist.sum((0, 1))
    assert per_o[0] > 0 and per_o[7] > 0 and np.abs(per_o[1:7]).max() <= 1e-9 * per_o[0]
    assert abs(per_o[7] / (per_o[0] + per_o[7]) - 8.0 / 360.0) < 1e-6
    # angle 0: the frame is the image's, obin = 0 exactly: bin 0 alone
    per_o = M.histogram(base, np.array([60, 60, 5, 0], np.float32)).sum((0, 1))
    assert per_o[0] > 0 and np.abs(per_o[1:]).max() <= 1e-9 * per_o[0]


def test_rotating_image_and_angle_by_90_degrees_keeps_the_descriptor():
    """np.rot90 (counter-clockwise on the screen) maps pixel (r, c) of an N x N image to (N - 1 - c, r).  With `a` = 360 - angle measured
    like the gradient orientation (y up), the rotated patch in a frame turned by +90 deg is the same patch: angle -> angle - 90 gives
    the same 4 x 4 x 8 histogram cell for cell.  Keeping the angle instead turns the cells: cell (row, col) -> (3 - col, row) and
    orientation bin o -> o + 2.  (The float64 part of the model is exact to ~1e-12; the base image is blurred once and rotated with it.)"""
    N = 81
    base = _base(_texture(N, N, 3))
    rot = np.ascontiguousarray(np.rot90(base))
    r, c = 37, 44
    for size, angle in ((5, 200.0), (5, 91.0), (8, 300.5)):
        h0 = M.histogram(base, np.array([c, r, size, angle], np.float32))
        h1 = M.histogram(rot, np.array([r, N - 1 - c, size, angle - 90.0], np.float32))
        assert np.abs(h1 - h0).max() <= 1e-9 * h0.max()
        h2 = M.histogram(rot, np.array([r, N - 1 - c, size, angle], np.float32))
        pred = np.zeros_like(h0)
        for row in range(4):
            for col in range(4):
                for o in range(8):
                    pred[3 - col, row, (o + 2) % 8] = h0[row, col, o]
        assert np.abs(h2 - pred).max() <= 1e-9 * h0.max()


def test_radius_larger_than_the_image_uses_interior_pixels_only():
    g = _texture(20, 24, 4)
    base = _base(g)
    hist, info = M.histogram(base, np.array([11, 9, 40, -1], np.float32), want_samples=True)
    assert info["radius"] == int(np.sqrt(24 * 24 + 20 * 20)) == 31            # round(60 * 1.414 * 2.5) = 212, clipped to the diagonal
    assert info["n"] == 18 * 22                                               # every interior pixel lies in the support (hw = 60)
    assert info["r"].min() == 1 and info["r"].max() == 18 and info["c"].min() == 1 and info["c"].max() == 22
    assert hist.any()
    # a keypoint outside the image whose support still reaches it, and one whose support does not
    assert M.histogram(base, np.array([-3, 9, 5, -1], np.float32)).any()
    assert not M.histogram(base, np.array([-40, 9, 5, -1], np.float32)).any()


def test_geometry_of_the_reference_keypoints():
    ptx, pty, a, hw, radius = M.geometry(np.array([10.5, 11.5, 5, -1], np.float32), 160, 640)
    assert (ptx, pty, float(a), float(hw), radius) == (10, 12, 1.0, 7.5, 27)   # round half to even; 360 + 1 - 360; 55 x 55 samples
    assert M.geometry(np.array([0, 0, 5, 0], np.float32), 160, 640)[2] == 0.0
    assert M.geometry(np.array([0, 0, 2, 0], np.float32), 160, 640)[4] == 11
    assert M.geometry(np.array([0, 0, 12.3, 0], np.float32), 160, 640)[4] == 65


def test_grid_order_and_count():
    from relativepose_amd import rputil
    g = M.grid_keypoints(128, 32, 5)
    assert g.shape == (182, 4) and tuple(g[0]) == (0, 0, 5, -1) and tuple(g[1]) == (5, 0, 5, -1) and tuple(g[26]) == (0, 5, 5, -1)
    assert tuple(g[-1]) == (125, 30, 5, -1)
    assert len(M.grid_keypoints(640, 160, 5)) == 4096
    for w, h, s in ((128, 32, 5), (640, 160, 5), (48, 32, 1), (50, 33, 7)):
        assert np.array_equal(rputil.sift_grid_keypoints(w, h, s), M.grid_keypoints(w, h, s))


def test_float32_rank_expression_equals_the_integer_one():
    """128 * 255^2 < 2^24: every partial sum of the reference's float32 expression is an integer below 2^24, hence exact."""
    rs = np.random.RandomState(5)
    src, tgt, dense = rs.randint(0, 256, (40, 128)), rs.randint(0, 256, (40, 128)), rs.randint(0, 256, (300, 128))
    src[0], tgt[0] = 0, 255                                       # the largest distance: 128 * 255^2 = 8 323 200
    dense[:40] = tgt                                              # ties: not counted
    dense[40:60] = src[:20] + rs.randint(-1, 2, (20, 128))
    src, tgt, dense = (np.clip(x, 0, 255).astype(np.uint8) for x in (src, tgt, dense))
    cf, df = M.rank_f32(src, tgt, dense)
    ci, ti = M.rank_int(src[None], tgt[None], dense[None])
    assert df.dtype == np.float32 and np.array_equal(df.astype(np.int64), ti[0]) and np.array_equal(cf, ci[0])
    assert ti[0, 0] == 128 * 255 * 255 < 2 ** 24 and ci[0].max() > 0
    c2, t2 = M.rank_int(src[None].repeat(2, 0), tgt[None].repeat(2, 0), dense[None].repeat(2, 0), pair_valid=[1, 0])
    assert np.array_equal(c2[0], ci[0]) and (c2[1] == -1).all() and (t2[1] == -1).all()


# ----------------------------------------------------------------------------------------------------------------- ABI and plumbing
def test_header_declares_the_siftdesc_symbols():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    from relativepose_amd import _lib, build
    for sym in ("relpose_sift_describe_workspace_bytes", "relpose_sift_describe", "relpose_sift_rank"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
        assert sym in _lib.SIGNATURES
    assert "typedef struct RelposeSiftDescArgs" in h and "typedef struct RelposeSiftRankArgs" in h
    for cite in ("mainPanoCompletion2view.py:353-381", "mainPanoCompletion2view.py:373, :378-379", "UNTESTED"):
        assert cite in h, cite
    assert ("siftdesc.hip", ["-ffp-contract=off"]) in build.SOURCES


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
@pytest.mark.parametrize("name", ["SiftDescArgs", "SiftRankArgs"])
def test_args_layout_matches_ctypes(tmp_path, name):
    from relativepose_amd import _lib
    cls = getattr(_lib, name)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof(Relpose{name}));\n' +
                   "".join(f'  printf(" %zu", offsetof(Relpose{name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]


def test_invalid_arguments_return_einval_without_a_device():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_double * 64)()                      # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)

    def describe(**kw):
        a = _lib.SiftDescArgs()
        a.struct_size = C.sizeof(a)
        a.n_views, a.img_h, a.img_w, a.channels = 1, 32, 48, 3
        a.crop_x, a.crop_y, a.crop_w, a.crop_h, a.n_kp = 0, 0, 48, 32, 4
        for k in ("images", "kp", "desc", "workspace"):
            setattr(a, k, p)
        a.workspace_bytes = 1 << 20
        for k, v in kw.items():
            setattr(a, k, v)
        return L.relpose_sift_describe(C.byref(a))

    assert L.relpose_sift_describe(None) == -1
    for bad in (dict(images=None), dict(kp=None), dict(desc=None), dict(workspace=None), dict(n_views=0), dict(channels=2), dict(img_h=0),
                dict(crop_w=0), dict(crop_h=4096), dict(crop_x=-1), dict(crop_x=1), dict(crop_y=1), dict(n_kp=-1), dict(grid_step=-1),
                dict(grid_step=5), dict(grid_step=5, kp=None, n_kp=69), dict(grid_step=5, kp=None, n_kp=70, kp_count=p), dict(kp=p + 2),
                dict(desc_f32=p + 1), dict(base=p + 2), dict(struct_size=8)):
        assert describe(**bad) == -1, bad
    assert describe(workspace_bytes=16) == -2      # RELPOSE_ENOMEM: still before any launch
    assert L.relpose_sift_describe_workspace_bytes(3, 32, 48) >= 3 * 32 * 48 * 4
    assert L.relpose_sift_describe_workspace_bytes(0, 32, 48) == 0 and L.relpose_sift_describe_workspace_bytes(1, 4096, 48) == 0

    def rank(**kw):
        a = _lib.SiftRankArgs()
        a.struct_size = C.sizeof(a)
        a.n_pairs, a.n_slots, a.n_points = 1, 4, 4
        for k in ("src", "tgt", "dense", "thr", "count"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.relpose_sift_rank(C.byref(a))

    assert L.relpose_sift_rank(None) == -1
    for bad in (dict(src=None), dict(tgt=None), dict(dense=None), dict(thr=None), dict(count=None), dict(n_pairs=0), dict(n_slots=0),
                dict(n_points=0), dict(src=p + 8), dict(dense=p + 4), dict(thr=p + 2), dict(struct_size=8)):
        assert rank(**bad) == -1, bad


def test_host_functions_need_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from relativepose_amd import descriptor, rputil
    img = np.zeros((1, 32, 48), np.uint8)
    z = np.zeros((1, 4, 128), np.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        rputil.sift_describe_dev(img, None, np.zeros((1, 2, 4), np.float32))
    with pytest.raises(RuntimeError, match="GPU"):
        rputil.sift_describe_grid_dev(img, None, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        descriptor.sift_rank_dev(z, z, z)
    with pytest.raises(RuntimeError, match="GPU"):
        descriptor.evalSiftDescriptor(np.zeros((1, 2, 3, 32, 128), np.float32),
                                      {"idxSrc": np.zeros((1, 8, 2)), "idxTgt": np.zeros((1, 8, 2)), "valid": np.ones(1)}, np.random.RandomState(0))


def test_meta_kernel_shapes():
    import torch
    from relativepose_amd import ops
    assert "sift_describe" in ops.OPS and "sift_rank" in ops.OPS
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    d, f = torch.ops.relpose.sift_describe(e(64, 160, 640, 3, dt=torch.uint8), [], e(64, 100, 4))
    assert d.shape == f.shape == (64, 100, 128) and (d.dtype, f.dtype) == (torch.uint8, torch.float32)
    d, f = torch.ops.relpose.sift_describe(e(64, 160, 640, 3, dt=torch.uint8), [], e(0), None, 5)
    assert d.shape == f.shape == (64, 4096, 128)
    d, _ = torch.ops.relpose.sift_describe(e(2, 64, 256, dt=torch.uint8), [32, 0, 128, 32], e(0), None, 5)
    assert d.shape == (2, 182, 128)
    u = lambda *s: e(*s, dt=torch.uint8)
    c, t = torch.ops.relpose.sift_rank(u(32, 100, 128), u(32, 100, 128), u(32, 4096, 128))
    assert c.shape == t.shape == (32, 100) and c.dtype == t.dtype == torch.int32


def test_cli_defaults_are_unchanged_without_the_flag():
    from relativepose_amd import evaluation
    d = vars(evaluation._cli_parser().parse_args([]))
    assert d.pop("sift_baseline") is False
    assert d == {"gpus": 1, "dataset": "scannet", "pairs": 2048, "batch": 256, "keypoints": 200, "exp": None, "rm": False, "round_batches": None,
                 "seed": 4000, "keypoint_mode": "given", "sift": 120, "sift_detector": "synthetic", "precision": "f32", "completion": 1,
                 "method": "ours", "descriptor_eval": False}
    a = evaluation._cli_parser().parse_args(["--descriptor-eval", "--sift-baseline"])
    assert a.descriptor_eval and a.sift_baseline
