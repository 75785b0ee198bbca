"""CPU: the coloured ICP contract's numpy model (tests/cicp_model.py) and the C ABI of relpose_cicp."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cicp_model as M
import cicp_scenes as S
import fgr_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the model, seeds 0-5 of cicp_scenes.planted_pair started from the truth perturbed by 3 degrees and 2 cm (4.4-5.5 cm at the
# origin): 0.006-0.049 degrees and 0.11-0.44 mm after the three levels; the bounds leave a third on top.
MAX_DEG, MAX_T = 0.065, 0.0006
SEEDS = (0, 1, 2)
PLANE_SHIFT = (0.012, -0.009)


@pytest.fixture(scope="module")
def planted():
    out = {}
    for s in SEEDS:
        p = S.planted_pair(s)
        out[s] = (p, M.register(p[0], p[2], p[1], p[3], S.perturbed(p[4], s)))
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_model_recovers_planted_motion(planted, seed):
    p, r = planted[seed]
    d0, t0 = S.pose_error(S.perturbed(p[4], seed), p[4])
    assert d0 > 2.9 and t0 > 0.04
    assert r["status"] == M.STATUS_OK
    deg, dt = S.pose_error(r["pose"], p[4])
    assert deg < MAX_DEG and dt < MAX_T, (deg, dt)
    assert np.array_equal(r["pose"], r["level_pose"][2]) and (r["n_iterations"] >= 1).all()
    assert (r["levels"][2]["ncnt"] >= 4).mean() > 0.95           # the sampling is dense enough for the 1 cm level's gradients


def _in_plane_error(T_hat, T, src):
    d = (src @ T_hat[:3, :3].T + T_hat[:3, 3]) - (src @ T[:3, :3].T + T[:3, 3])
    return float(np.sqrt((d[:, :2] ** 2).sum(1)).mean())


def test_colour_term_removes_an_in_plane_offset_and_geometry_alone_does_not():
    src, tgt, cs, ct, T = S.textured_plane(0, PLANE_SHIFT)
    planted_off = float(np.hypot(*PLANE_SHIFT))
    assert abs(_in_plane_error(np.eye(4), T, src) - planted_off) < 1e-12
    r = M.register(src, cs, tgt, ct, None, lam=M.LAMBDA_GEOMETRIC)
    e = _in_plane_error(r["pose"], T, src)
    assert r["status"] == M.STATUS_OK and e < 0.05 * planted_off, e
    g = M.register(src, cs, tgt, ct, None, lam=1.0)
    eg = _in_plane_error(g["pose"], T, src)
    assert eg >= 0.5 * planted_off, eg


def test_gradient_of_a_linear_intensity_on_a_plane_is_its_in_plane_slope():
    rs = np.random.RandomState(3)
    uv = rs.uniform(-0.2, 0.2, (1500, 2))
    slope3 = np.r_[0.7, -1.3, 2.1]
    # a plane of constant z: its normal comes out exactly, so the in-plane slope is (0.7, -1.3, 0)
    pts = np.c_[uv, np.zeros(len(uv))] + np.r_[0.1, -0.2, -1.0]
    idx, cnt = M.neighbors(pts, 0.04)
    nrm = M.normals(pts, idx, cnt)
    assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
    g = M.gradients(pts, pts @ slope3 + 0.25, nrm, idx, cnt)
    full = cnt >= 4
    assert full.sum() > 1400
    assert np.abs(g[full] - np.r_[0.7, -1.3, 0.0]).max() <= 1e-12
    assert np.array_equal(g[~full], np.zeros((int((~full).sum()), 3)))
    # a tilted plane: the sampled field is linear only up to the rounding of the intensities (eps |I|), which a neighbour at distance d
    # turns into a slope error of eps |I| / d; 64 of those for the closest neighbour of the cloud bound the error of the solve
    R = S.rotation([0.3, -0.5, 0.8], 25.0)
    pts = np.c_[uv, np.zeros(len(uv))] @ R.T + np.r_[0.1, -0.2, -1.0]
    n_true = R[:, 2] if R[:, 2] @ (-pts[0]) >= 0 else -R[:, 2]
    inten = pts @ slope3 + 0.25
    idx, cnt = M.neighbors(pts, 0.04)
    nrm = M.normals(pts, idx, cnt)
    assert np.abs(nrm - n_true).max() < 1e-9
    g = M.gradients(pts, inten, nrm, idx, cnt)
    d_min = np.sqrt(((pts[idx[:, 1]] - pts) ** 2).sum(1)).min()
    bound = 64 * np.finfo(np.float64).eps * np.abs(inten).max() / d_min
    assert bound < 1e-9 and np.abs(g - (slope3 - (slope3 @ n_true) * n_true)).max() <= bound
    # nn < 4 and a non-positive pivot (a degenerate neighbourhood: all rows parallel) give zero
    line = np.c_[np.linspace(0, 0.03, 6), np.zeros(6), np.zeros(6)] + np.r_[0, 0, -1.0]
    li, lc = M.neighbors(line, 0.04)
    gl = M.gradients(line, np.arange(6.0), np.tile([0.0, 1.0, 0.0], (6, 1)), li, lc)
    assert (lc >= 4).all() and np.array_equal(gl, np.zeros((6, 3)))


def test_searches_match_brute_force():
    rs = np.random.RandomState(5)
    tgt = rs.uniform(0, 0.3, (2500, 3))
    q = rs.uniform(-0.05, 0.35, (3000, 3))
    q[:3] = (np.nan, 0.1, 0.1), (np.inf, 0.1, 0.1), (50.0, 0.1, 0.1)
    d = tgt[None] - q[:, None]
    with np.errstate(invalid="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        hit = np.nan_to_num(d2, nan=np.inf).min(1) < 0.02 ** 2
    corr, best = M.nearest(tgt, q, 0.02)
    assert np.array_equal(corr >= 0, hit) and 100 < hit.sum() < 2900 and not hit[:3].any()
    assert np.array_equal(corr[hit], np.argmin(d2[hit], 1)) and np.array_equal(best[hit], d2[hit].min(1)) and (best[~hit] == 0).all()
    dup = np.concatenate([tgt[:50], tgt[:50]])                                     # ties go to the lower index
    assert np.array_equal(M.nearest(dup, tgt[:50] + 1e-4, 0.02)[0], np.arange(50))
    idx, cnt = M.neighbors(tgt, 0.04)
    dd = tgt[None, :, :] - tgt[:300, None, :]
    dd2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
    for i in range(300):
        c = np.flatnonzero(dd2[i] < 0.04 ** 2)
        c = c[np.lexsort((c, dd2[i][c]))][:M.MAX_NN]
        assert cnt[i] == len(c) and np.array_equal(idx[i, :len(c)], c) and (idx[i, len(c):] == -1).all() and idx[i, 0] == i
    assert cnt.max() == M.MAX_NN and cnt.min() < M.MAX_NN


def test_voxel_grid_averages_colours_like_points():
    rs = np.random.RandomState(6)
    pts = rs.uniform(0, 0.2, (4000, 3))
    col = rs.uniform(0, 1, (4000, 3))
    for v in M.RADII:
        p, c = M.voxel_down(pts, col, v)
        mb = pts.min(0) - 0.5 * v
        key = np.floor((pts - mb) / v).astype(np.int64)
        uk, inv = np.unique(key, axis=0, return_inverse=True)
        assert len(p) == len(uk)
        for j in (0, len(uk) // 2, len(uk) - 1):
            m = np.flatnonzero(inv.reshape(-1) == j)
            sp, sc = np.zeros(3), np.zeros(3)
            for i in m:
                sp, sc = sp + pts[i], sc + col[i]
            assert np.array_equal(p[j], sp / len(m)) and np.array_equal(c[j], sc / len(m))
    p5, _ = M.voxel_down(pts, col, F.VOXEL)
    assert np.array_equal(p5, F.voxel_down(pts)[0])                                # §4.6 stage 1 is the voxel = 0.05 case


def test_stop_rule_and_level_without_correspondences():
    src, tgt, cs, ct, T = S.planted_pair(0)
    lv = M.prepare_level(src, cs, tgt, ct, 0.04)
    T0 = S.perturbed(T, 0)
    s0 = M.step(lv, T0, 0.04)
    assert not s0["ended"] and s0["x"] is not None and s0["ncorr"] > 100
    # the same evaluation twice in a row meets the stop rule; a first evaluation never does
    s1 = M.step(lv, T0, 0.04, prev=(s0["fitness"], s0["rmse"]))
    assert s1["ended"] and s1["x"] is None and np.array_equal(s1["T_next"], T0)
    s2 = M.step(lv, T0, 0.04, prev=(s0["fitness"] + 2e-6, s0["rmse"]))
    assert not s2["ended"] and np.array_equal(s2["T_next"], s0["T_next"])
    s3 = M.step(lv, T0, 0.04, prev=(s0["fitness"], s0["rmse"] + 2e-6))
    assert not s3["ended"]
    _, fit, rmse, nit, trace = M.run_level(lv, T0, 0.04, 50)
    assert 2 <= nit < 50 and trace[-1]["ended"] and not any(t["ended"] for t in trace[:-1])
    assert M.run_level(lv, T0, 0.04, 3)[3] == 3                                    # the cap
    # no correspondence: not an error, the level ends at once with the pose unchanged and the next level still runs
    far = np.eye(4)
    far[:3, 3] = (5.0, 0.0, 0.0)
    r = M.register(src, cs, tgt, ct, far @ T)
    assert r["status"] == M.STATUS_OK and r["n_iterations"].tolist() == [1, 1, 1] and r["fitness"].tolist() == [0, 0, 0]
    assert r["inlier_rmse"].tolist() == [0, 0, 0] and np.array_equal(r["pose"], far @ T)


def test_too_few_points_and_overflow_status():
    src, tgt, cs, ct, T = S.planted_pair(0)
    r = M.register(src[:2], cs[:2], tgt, ct)
    assert r["status"] == M.STATUS_FEW_POINTS and np.array_equal(r["pose"], np.eye(4))
    assert M.register(np.zeros((0, 3)), np.zeros((0, 3)), tgt, ct)["status"] == M.STATUS_FEW_POINTS
    r = M.register(src, cs, tgt, ct, max_points=4096)                               # only the 1 cm level has more voxels than that
    n = [len(lv["ps"]) for lv in r["levels"]]
    assert n[0] < n[1] <= 4096 < n[2] and r["status"] == M.STATUS_OVERFLOW and np.array_equal(r["pose"], np.eye(4))


def test_solves_agree_with_numpy():
    rs = np.random.RandomState(7)
    for k in (3, 6):
        B = rs.randn(40, k, k)
        A = B @ B.transpose(0, 2, 1) + k * np.eye(k)
        b = rs.randn(40, k)
        x, ok = M.chol_solve_batch(A, b)
        assert ok.all()
        for i in range(40):
            ref = np.linalg.solve(A[i], b[i])
            assert np.abs(x[i] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
            assert np.array_equal(x[i].view(np.uint64), F.cholesky_solve(A[i], b[i]).view(np.uint64))      # the same expression order
            assert M.pivots_positive(A[i])
    bad = np.diag([1.0, 2.0, 0.0, 1.0, 1.0, 1.0])
    x, ok = M.chol_solve_batch(bad[None], np.ones((1, 6)))
    assert not ok[0] and not x.any() and not M.pivots_positive(bad) and not M.pivots_positive(-np.eye(3))
    A, r = M.unpack_system(np.arange(27.0))
    assert np.array_equal(A, A.T) and A[0].tolist() == [0, 1, 2, 3, 4, 5] and A[1, 1] == 6 and A[5, 5] == 20 and r.tolist() == [21, 22, 23, 24, 25, 26]


def test_system_matches_a_direct_restatement():
    src, tgt, cs, ct, T = S.planted_pair(1)
    lv = M.prepare_level(src, cs, tgt, ct, 0.04)
    T0 = S.perturbed(T, 1)
    q, corr, ncorr, fit, rmse = M.evaluate(lv["ps"], lv["pt"], T0, 0.04)
    lam = 0.9
    tot = M.build_system(q, M.intensity(lv["cs"]), corr, lv["pt"], M.intensity(lv["ct"]), lv["normals"], lv["gradient"], lam)
    JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
    for i in np.flatnonzero(corr >= 0):
        j = corr[i]
        vs, vt, nt, dit = q[i], lv["pt"][j], lv["normals"][j], lv["gradient"][j]
        rG = np.sqrt(lam) * (vs - vt) @ nt
        JG = np.sqrt(lam) * np.r_[np.cross(vs, nt), nt]
        vp = vs - ((vs - vt) @ nt) * nt
        ip = dit @ (vp - vt) + M.intensity(lv["ct"][j])
        dm = -(dit - (dit @ nt) * nt)
        rI = np.sqrt(1 - lam) * (M.intensity(lv["cs"][i]) - ip)
        JI = np.sqrt(1 - lam) * np.r_[np.cross(vs, dm), dm]
        JTJ += np.outer(JG, JG) + np.outer(JI, JI)
        JTr += JG * rG + JI * rI
    A, r = M.unpack_system(tot)
    assert np.allclose(A, JTJ, rtol=1e-10, atol=1e-12) and np.allclose(r, JTr, rtol=1e-10, atol=1e-12)
    assert fit == ncorr / len(lv["ps"]) and abs(rmse - np.sqrt(M.nearest(lv["pt"], q, 0.04)[1].sum() / ncorr)) < 1e-15


def test_header_declares_the_cicp_symbols():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    for sym in ("relpose_cicp_workspace_bytes", "relpose_cicp"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "typedef struct RelposeCicpArgs" in h and "baselines.py:110-168" in h
    from relativepose_amd import _lib, baselines, build, ops
    assert int(re.search(r"#define RELPOSE_CICP_OVERFLOW \((-\d+)\)", h).group(1)) == _lib.CICP_OVERFLOW
    assert _lib.CICP_OVERFLOW not in (_lib.FGR_OVERFLOW, _lib.RANSAC_OVERFLOW, _lib.SIFT_OVERFLOW)
    assert int(re.search(r"#define RELPOSE_CICP_LEVELS (\d+)", h).group(1)) == _lib.CICP_LEVELS == len(M.RADII) == 3
    assert int(re.search(r"#define RELPOSE_CICP_TRACE_SLOTS (\d+)", h).group(1)) == _lib.CICP_TRACE_SLOTS == M.SLOTS == sum(M.MAX_ITER)
    assert float(re.search(r"#define RELPOSE_CICP_LAMBDA_GEOMETRIC ([\d.]+)", h).group(1)) == _lib.CICP_LAMBDA_GEOMETRIC == M.LAMBDA_GEOMETRIC
    assert list(M.SLOT_OFF) == [0, M.MAX_ITER[0], M.MAX_ITER[0] + M.MAX_ITER[1]]
    assert ("cicp.hip", ["-ffp-contract=off"]) in build.SOURCES
    for sym in ("relpose_cicp_workspace_bytes", "relpose_cicp"):
        assert sym in _lib.SIGNATURES
    assert "colored_icp" in ops.OPS and "color_registration" in ops.OPS
    assert baselines.STATUS[1] == "too few points" and baselines.STATUS[3] == "overflow"
    for fn in ("colored_icp_dev", "color_registration_dev", "open3d_color_registration"):
        assert callable(getattr(baselines, fn)) and fn in baselines.__doc__


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_cicp_args_layout_matches_ctypes(tmp_path):
    from relativepose_amd import _lib
    fields = [f for f, _ in _lib.CicpArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(RelposeCicpArgs));\n' +
                   "".join(f'  printf(" %zu", offsetof(RelposeCicpArgs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.CicpArgs)
    assert got[1:] == [getattr(_lib.CicpArgs, f).offset for f in fields]
    assert fields[0] == "struct_size" and fields[4:8] == ["pc", "valid", "color", "init"] and fields[-3:] == ["workspace", "workspace_bytes", "stream"]


def test_workspace_sizes_and_invalid_arguments():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    w1, w32 = L.relpose_cicp_workspace_bytes(1, 25600, 32768), L.relpose_cicp_workspace_bytes(32, 25600, 32768)
    assert w32 > 16 * w1 > 0
    assert L.relpose_cicp_workspace_bytes(1, 25600, 16384) < w1 < L.relpose_cicp_workspace_bytes(1, 51200, 32768)
    for bad in ((0, 100, 100), (1, 0, 100), (1, 100, 0), (1, 100, 65537), (-1, 100, 100)):
        assert L.relpose_cicp_workspace_bytes(*bad) == 0, bad
    a = _lib.CicpArgs()
    a.struct_size = C.sizeof(a)
    assert L.relpose_cicp(C.byref(a)) == -1                         # no clouds / outputs: RELPOSE_EINVAL before touching a device
    assert L.relpose_cicp(None) == -1
    a.struct_size = 4
    assert L.relpose_cicp(C.byref(a)) == -1
    # every pointer set but lambda_geometric outside 0 .. 1 (or NaN): still RELPOSE_EINVAL, before any device call
    buf = (C.c_double * 64)()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_points, a.max_points = 1, 4, 4
    for f in ("pc", "valid", "color", "pose", "status", "workspace"):
        setattr(a, f, C.addressof(buf))
    a.workspace_bytes = 1 << 40
    for lam in (-0.1, 1.5, float("nan")):
        a.lambda_geometric = lam
        assert L.relpose_cicp(C.byref(a)) == -1, lam


def test_meta_kernel_shapes():
    import torch
    from relativepose_amd import ops  # noqa: F401
    pc = torch.empty(64, 25600, 3, dtype=torch.float64, device="meta")
    valid = torch.empty(64, 25600, dtype=torch.uint8, device="meta")
    init = torch.empty(32, 4, 4, dtype=torch.float64, device="meta")
    for pose, status in (torch.ops.relpose.colored_icp(pc, pc, valid, init), torch.ops.relpose.color_registration(pc, pc, valid)):
        assert pose.shape == (32, 4, 4) and pose.dtype == torch.float64 and status.shape == (32,) and status.dtype == torch.int32


def test_evaluation_refuses_what_cgs_cannot_run():
    from relativepose_amd import evaluation
    with pytest.raises(SystemExit, match="one GPU"):
        evaluation.main(["--method", "cgs", "--gpus", "2", "--dataset", "suncg"])
    with pytest.raises(SystemExit, match="full-resolution"):
        evaluation.main(["--method", "cgs", "--dataset", "scannet"])


def test_observed_colors_follow_the_reference_quantisation():
    from relativepose_amd import evaluation
    rs = np.random.RandomState(8)
    rgb = rs.uniform(-0.1, 1.1, (2, 3, 8, 32)).astype(np.float32)
    c = evaluation.observed_colors(rgb)
    assert c.shape == (2, 64, 3) and c.dtype == np.float64 and c.min() == 0.0 and c.max() == 1.0
    v, u = 5, 3
    want = (rgb[1, :, v, 8 + u] * 255).clip(0, 255).astype('uint8') / 255.
    assert np.array_equal(c[1, v * 8 + u], want)
