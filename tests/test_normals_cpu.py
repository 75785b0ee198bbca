"""CPU: the depth-normals contract (tests/normals_model.py) against the analytic normals of the synthetic rooms, its gate,
its behaviour on holes and sparse views, and the C ABI / operator plumbing of relpose_depth_normals."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import normals_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATASETS = ("suncg", "matterport", "scannet")
SIZES = ((32, 2), (48, 3))                 # (h, r)
U = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------- ABI and plumbing
def test_header_declares_the_symbol():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    assert re.search(r"\brelpose_depth_normals\s*\(", h) and "typedef struct RelposeDepthNormalsArgs" in h
    assert "datasets/SUNCG.py:300-313" in h
    from relativepose_amd import _lib, build
    assert ("normals.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert "relpose_depth_normals" in _lib.SIGNATURES


@pytest.fixture(scope="module")
def lib():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_library_exports_the_symbol(lib):
    assert hasattr(lib, "relpose_depth_normals")


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_args_layout_matches_ctypes(tmp_path):
    from relativepose_amd import _lib
    cls = _lib.DepthNormalsArgs
    fields = [f for f, _ in cls._fields_]
    assert fields[0] == "struct_size" and fields[-1] == "stream"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(RelposeDepthNormalsArgs));\n' +
                   "".join(f'  printf(" %zu", offsetof(RelposeDepthNormalsArgs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]


def test_invalid_arguments_return_einval_without_a_device(lib):
    from relativepose_amd import _lib
    EINVAL = -1
    assert lib.relpose_depth_normals(None) == EINVAL
    buf = (C.c_float * 64)()                       # host memory: a valid call would fault, an invalid one must not touch it
    p = C.addressof(buf)

    def call(**kw):
        a = _lib.DepthNormalsArgs()
        a.struct_size = C.sizeof(a)
        a.n_views, a.h, a.dataset, a.radius, a.min_neighbors, a.gate_scale = 2, 32, 0, 3, 6, 3.0
        a.depth = a.normal = a.valid = p
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.relpose_depth_normals(C.byref(a))

    assert call(struct_size=16) == EINVAL
    assert call(struct_size=C.sizeof(_lib.DepthNormalsArgs) - 8) == EINVAL      # the stream field is cut off
    assert call(depth=None) == EINVAL
    assert call(normal=None) == EINVAL
    assert call(n_views=0) == EINVAL
    assert call(h=6) == EINVAL and call(h=8, radius=4) == EINVAL                # h < 2r + 1
    assert call(radius=0) == EINVAL and call(radius=5) == EINVAL
    assert call(min_neighbors=2) == EINVAL
    assert call(min_neighbors=49) == EINVAL                                     # (2 * 3 + 1)^2 - 1 = 48 is the most
    assert call(radius=1, min_neighbors=9) == EINVAL
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert call(gate_scale=g) == EINVAL, g
    assert call(dataset=3) == EINVAL and call(dataset=-1) == EINVAL


def test_operator_is_registered_with_a_meta_kernel():
    import torch
    from relativepose_amd import ops
    assert "depth_normals" in ops.OPS
    d = torch.empty(3, 20, 80, dtype=torch.float32, device="meta")
    nrm, valid = torch.ops.relpose.depth_normals(d, 1, 4, 3.0, 6)
    assert nrm.shape == (3, 3, 20, 80) and nrm.dtype == torch.float32 and valid.shape == (3, 20, 80) and valid.dtype == torch.uint8
    nrm, valid = torch.ops.relpose.depth_normals(d, 0)                          # the defaults
    assert nrm.shape == (3, 3, 20, 80)
    with pytest.raises(Exception):                                              # no CPU kernel: loud failure, no fallback
        torch.ops.relpose.depth_normals(torch.zeros(1, 20, 80), 0)


def test_host_shims_exist():
    import inspect
    from relativepose_amd import util
    sig = inspect.signature(util.depth_normals_dev)
    assert [sig.parameters[k].default for k in ("radius", "gate_scale", "min_neighbors", "stages")] == [3, 3.0, 6, False]
    assert list(inspect.signature(util.depth_normals).parameters)[:2] == ["depth", "dataList"]


def test_evaluation_cli_takes_normals_and_measures_their_error():
    import torch
    from relativepose_amd import evaluation as E
    ap = E._cli_parser_completion()
    assert ap.parse_args([]).normals == "given" and ap.parse_args(["--normals", "estimated"]).normals == "estimated"
    for argv in (["--method", "fgs"], ["--descriptor-eval"], ["--completion-eval"]):
        with pytest.raises(SystemExit):
            E.main(argv + ["--normals", "estimated", "--dataset", "suncg"])
    with pytest.raises(ValueError):
        E._prepare_batch(None, {"norm": None}, None, normals="computed")
    # the angle histogram: 0.01 degree bins over the pixels that are non-zero in both maps
    est = torch.zeros(1, 3, 2, 4)
    given = torch.zeros(1, 3, 2, 4)
    est[0, 2] = 1.0
    est[0, :, 1, 3] = 0.0                                                   # one pixel invalid in the estimate
    for k, deg in enumerate((0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0)):
        given[0, 1].view(-1)[k], given[0, 2].view(-1)[k] = 2 * np.sin(np.radians(deg)), 2 * np.cos(np.radians(deg))      # (not unit length)
    hist = E.normal_error_hist(est, given)
    assert hist.shape == (E.NORMAL_ERR_BINS,) and float(hist.sum()) == 7          # the eighth pixel is zero in both
    assert E.hist_quantile(hist.numpy(), 0.5) == pytest.approx(30.0, abs=0.011)
    assert E.hist_quantile(hist.numpy(), 0.9) == pytest.approx(60.0, abs=0.011)
    assert np.isnan(E.hist_quantile(np.zeros(8), 0.5))


# ----------------------------------------------------------------------------------------------------------------- the model
def _bound(m32, m64, r, gate_scale=3.0):
    """The per-pixel Davis-Kahan bound of the issue: 2 * 16 * 2^-24 * m * (rho + g) * g / (l1 - l0), in radians (inf without a gap)."""
    h = m32["depth"].shape[1]
    g = gate_scale * r * (2.0 / h) * m32["depth"].astype(np.float64)
    rho = np.linalg.norm(m32["P"].astype(np.float64), axis=-1)
    m = m32["count"] + 1.0
    gap = m64["lam"][..., 1] - m64["lam"][..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gap > 0, 2 * 16 * U * m * (rho + g) * g / gap, np.inf)


def _check_against_truth(dep, nrm_true, dataset, r, select, gate_scale=3.0):
    """model64's normals on the pixels `select` (interior and valid) against the analytic ones, within the per-pixel bound; pixels whose
    bound exceeds 0.05 rad are left out and may be at most 1 % of the valid pixels.  Returns (checked mask, angles)."""
    m32 = M.model32(dep, dataset, r, gate_scale)
    m64 = M.model64(m32)
    sel = select & m64["valid"]
    bound = _bound(m32, m64, r, gate_scale)
    out = sel & ~(bound <= 0.05)
    assert out.sum() <= 0.01 * m64["valid"].sum(), (int(out.sum()), int(m64["valid"].sum()))
    sel &= ~out
    ang = M.angle(m64["normal"], nrm_true)
    print(f"{dataset} r={r}: {int(sel.sum())} pixels, {int(out.sum())} left out, median bound {np.median(bound[sel]):.2e}, "
          f"max angle/bound {np.max(ang[sel] / bound[sel]):.3f}")
    assert (ang[sel] <= bound[sel]).all(), float(np.max(ang[sel] / bound[sel]))
    return sel, ang, m32, m64


@pytest.mark.parametrize("h,r", SIZES)
@pytest.mark.parametrize("dataset", DATASETS)
def test_model_matches_the_analytic_normals(dataset, h, r):
    dep, nrm_true = M.room(dataset, h, 100 + h)
    inter = M.interior(nrm_true, dep, r)
    sel, _, _, m64 = _check_against_truth(dep, nrm_true, dataset, r, inter)
    assert sel.sum() > 0.3 * dep.size
    w = 4 * h
    for k in range(4):                              # pixels on every seam, column 4h-1 | 0 among them: their windows cross it
        for col in ((k * h - 1) % w, k * h):
            assert sel[:, :, col].any(), (k, col)


@pytest.mark.parametrize("h,r", SIZES)
@pytest.mark.parametrize("dataset", DATASETS)
def test_gate_separates_foreground_from_background(dataset, h, r):
    """A rectangle spanning the seam between slots 0 and 1 has its depth scaled by 0.4: the same plane normal, 0.6 |P| nearer.  The pixels
    within r of the rectangle's border, inside and outside, keep the wall's normal under the default gate; with the gate wide open
    (gate_scale = 1e6) the two surfaces mix in their windows and every one of them is off by more than 0.1 rad."""
    dep, nrm_true, rect = M.gate_case(dataset, h)
    y0, y1, x0, x1 = rect
    assert x0 < h < x1
    near = np.zeros(dep.shape, bool)
    near[:, y0 - r:y1 + r, x0 - r:x1 + r] = True
    near[:, y0 + r:y1 - r, x0 + r:x1 - r] = False
    inter = M.interior(nrm_true, dep, r) & near
    sel, ang, m32, _ = _check_against_truth(dep, nrm_true, dataset, r, inter)
    assert (m32["count"][sel] >= 6).all() and (m32["count"][sel] < (2 * r + 1) ** 2 - 1).all()      # the gate rejected the other surface
    inside = np.zeros(dep.shape, bool)
    inside[:, y0:y1, x0:x1] = True
    assert (sel & inside).sum() > 20 and (sel & ~inside).sum() > 20
    assert (sel & inside)[:, :, h - 1].any() and (sel & inside)[:, :, h].any()                      # both sides of the seam
    open64 = M.model64(M.model32(dep, dataset, r, 1e6))
    off = M.angle(open64["normal"], nrm_true)
    assert open64["valid"][sel].all()
    print(f"gate open: min angle {off[sel].min():.3f} rad")
    assert (off[sel] > 0.1).all()


def _check_properties(dep, dataset, r):
    m32 = M.model32(dep, dataset, r)
    m64 = M.model64(m32)
    n, v = m64["normal"], m64["valid"]
    assert not v[dep == 0].any()
    assert (n[:, 0][~v] == 0).all() and (n[:, 1][~v] == 0).all() and (n[:, 2][~v] == 0).all()
    ln = np.linalg.norm(n, axis=1)
    assert np.abs(ln[v] - 1).max(initial=0) <= 1e-6
    assert ((np.moveaxis(n, 1, -1) * m32["P"]).sum(-1)[v] < 0).all()
    return m32, m64


@pytest.mark.parametrize("dataset", DATASETS)
def test_rooms_with_holes(dataset):
    h, r = 32, 2
    dep, nrm_true = M.room(dataset, h, 7, hole_frac=0.05)
    assert 0.03 < (dep == 0).mean() < 0.07
    _, m64 = _check_properties(dep, dataset, r)
    assert m64["valid"].mean() > 0.85
    _check_against_truth(dep, nrm_true, dataset, r, M.interior(nrm_true, dep, r))


def test_sparse_scannet_view():
    h, r = 48, 3
    dep, nrm_true = M.sparse_scannet_view(h, 11)
    m32, m64 = _check_properties(dep, "scannet", r)
    assert 0 < m64["valid"].sum() <= (dep != 0).sum()
    assert not m64["valid"][:, :, :h].any() and not m64["valid"][:, :, 2 * h:].any()
    sel, _, _, _ = _check_against_truth(dep, nrm_true, "scannet", r, M.interior(nrm_true, dep, r))
    assert sel.sum() > 100


def test_all_zero_view_gives_zeros():
    dep = np.zeros((1, 20, 80), np.float32)
    m32, m64 = _check_properties(dep, "suncg", 4)
    assert not m32["count"].any() and not m32["moments"].any() and not m64["valid"].any() and not m64["normal"].any()
