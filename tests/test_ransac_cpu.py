"""CPU: the RANSAC feature-registration contract's numpy model (tests/ransac_model.py) and the C ABI of relpose_ransac."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fgr_model as F
import fgr_scenes as S
import ransac_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the model, seeds 0-5 of planted_pair: 2.9-4.8 degrees and 1.9-7.4 cm with 50 validations, 0.7-3.9 degrees and 1.6-7.3 cm
# with the default 500 (there is no refit after the loop: the pose is one 4-point estimate); the bounds leave a third on top.
MAX_DEG, MAX_T = 6.5, 0.10
SEEDS = (0, 1, 2)
FEW_VALIDATIONS = 50


@pytest.fixture(scope="module")
def planted():
    return {s: S.planted_pair(s) for s in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_model_recovers_planted_motion(planted, seed):
    src, tgt, T = planted[seed]
    r = M.register(src, tgt, max_validations=FEW_VALIDATIONS)
    assert r["status"] == M.STATUS_OK and r["n_validations"] == FEW_VALIDATIONS
    deg, dt = S.pose_error(r["pose"], T)
    assert deg < MAX_DEG and dt < MAX_T, (deg, dt)
    assert r["val_inliers"][r["best_index"]] == round(r["fitness"] * len(r["down_src"]))


def test_draws_are_a_counter_hash():
    a = M.draw(5, np.arange(1000), 0, 37)
    assert np.array_equal(a, M.draw(5, np.arange(1000), 0, 37))
    assert not np.array_equal(a, M.draw(6, np.arange(1000), 0, 37))
    assert a.min() >= 0 and a.max() < 37 and len(np.unique(a)) == 37
    x = (0x9E3779B97F4A7C15 * 5 + 4 * 17 + 3) & F.M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & F.M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & F.M64
    x ^= x >> 31
    assert int(M.draw(5, np.array([17]), 3, 1000003)[0]) == x % 1000003


def _small_case(seed=3, density=500.0):
    src, tgt, T = S.planted_pair(seed, density=density)
    ds, dt = F.voxel_down(src)[0], F.voxel_down(tgt)[0]
    nn = F.nn_f32(F.features(ds)["fpfh"].astype(np.float32), F.features(dt)["fpfh"].astype(np.float32))
    return ds, dt, nn


def test_validated_set_is_the_first_passing_iterations():
    ds, dt, nn = _small_case()
    t = np.arange(200000)
    ok, _, _ = M.hypotheses(ds, dt, nn, t, 7)
    passing = t[ok]
    assert 10 < len(passing) < 200000
    vi, nit = M.screen(ds, dt, nn, 7, max_iterations=200000, max_validations=10, chunk=4096)
    assert np.array_equal(vi, passing[:10]) and nit == passing[9] + 1
    vi, nit = M.screen(ds, dt, nn, 7, max_iterations=200000, max_validations=len(passing) + 5)
    assert np.array_equal(vi, passing) and nit == 200000              # fewer pass than max_validations: n_iterations = the cap


def test_checkers_match_a_direct_restatement():
    ds, dt, nn = _small_case()
    t = np.arange(3000)
    idx = np.stack([M.draw(1, t, k, len(ds)) for k in range(4)], 1)
    s, q = ds[idx], dt[nn[idx]]
    edge = M.edge_ok(s, q)
    R, tr = M.estimate(s, q)
    dist = M.distance_ok(R, tr, s, q)
    n3 = lambda v: math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    for h in range(len(t)):
        e = True
        for j in range(4):
            for k in range(j + 1, 4):
                a, b = n3(s[h, j] - s[h, k]), n3(q[h, j] - q[h, k])
                e = e and not (a < 0.9 * b or b < 0.9 * a)
        assert e == edge[h], h
        d = True
        for k in range(4):
            p = [((R[h, a, 0] * s[h, k, 0] + R[h, a, 1] * s[h, k, 1]) + R[h, a, 2] * s[h, k, 2]) + tr[h, a] for a in range(3)]
            d = d and not n3(np.array(p) - q[h, k]) > 0.075
        assert d == dist[h], h
    assert edge.sum() > 0 and (edge & dist).sum() > 0


SHIM = r'''
#include "rp_math.h"
extern "C" void t_horn(const double* M, double* R, int n) {
    for (int h = 0; h < n; ++h) { double m[3][3], r[3][3]; for (int i = 0; i < 9; ++i) m[i / 3][i % 3] = M[9 * h + i];
        rp_horn_rotation(m, r); for (int i = 0; i < 9; ++i) R[9 * h + i] = r[i / 3][i % 3]; }
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_model_horn_equals_rp_horn_rotation_bitwise(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM)
    so = tmp_path / "shim.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "relativepose_amd", "csrc"), str(src),
                           "-o", str(so)])
    lib = C.CDLL(str(so))
    ds, dt, nn = _small_case()
    t = np.arange(4000)
    idx = np.stack([M.draw(2, t, k, len(ds)) for k in range(4)], 1)
    s, q = ds[idx], dt[nn[idx]]
    cs, ct = (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]) / 4.0, (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]) / 4.0
    Ms = sum((s[:, k] - cs)[:, :, None] * (q[:, k] - ct)[:, None, :] for k in range(4))
    rs = np.random.RandomState(0)
    Ms = np.concatenate([Ms, rs.randn(500, 3, 3), np.zeros((1, 3, 3)), np.eye(3)[None]])
    got = np.ascontiguousarray(M.horn(Ms))
    ref = np.zeros_like(got)
    Mc = np.ascontiguousarray(Ms)
    lib.t_horn(Mc.ctypes.data_as(C.POINTER(C.c_double)), ref.ctypes.data_as(C.POINTER(C.c_double)), len(Mc))
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    # and Horn recovers a planted rotation (t ~ R s)
    R0 = S.rotation([0.2, 0.5, -0.3], 33.0)
    p = rs.randn(4, 3)
    c = p - (((p[0] + p[1]) + p[2]) + p[3]) / 4.0
    assert np.abs(M.horn(sum(c[k][:, None] * (R0 @ c[k])[None, :] for k in range(4))[None])[0] - R0).max() < 1e-12


def test_validation_grid_and_reduction_order():
    rs = np.random.RandomState(4)
    tgt = rs.uniform(0, 1.0, (3000, 3))
    q = rs.uniform(-0.1, 1.1, (4000, 3))
    g = M.CellGrid(tgt)
    got = g.min_d2(q)
    d = tgt[None, :, :] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ref = np.where(d2.min(1) < 0.075 ** 2, d2.min(1), np.inf)
    assert np.array_equal(got, ref) and np.isfinite(got).sum() > 100
    x = rs.rand(3, 1000)
    s = M.reduce_sum(x)
    assert np.allclose(s, x.sum(1), rtol=1e-13, atol=0)
    assert M.select(np.array([0, 5, 5, 7, 7]), np.array([0.0, 0.01, 0.005, 0.02, 0.02])) == 3
    assert M.select(np.array([0, 0]), np.array([0.0, 0.0])) == -1


def test_too_few_points_and_overflow_status():
    assert M.register(np.zeros((0, 3)), np.random.rand(100, 3))["status"] == M.STATUS_FEW_POINTS
    src, tgt, _ = S.planted_pair(0, density=300.0)
    r = M.register(src, tgt, max_points=50)
    assert r["status"] == M.STATUS_OVERFLOW and len(r["down_src"]) > 50 and np.array_equal(r["pose"], np.eye(4))


def test_header_declares_the_ransac_symbols():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    for sym in ("relpose_ransac_workspace_bytes", "relpose_ransac"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "typedef struct RelposeRansacArgs" in h and "baselines.py:52-81" in h
    from relativepose_amd import _lib, baselines, build
    assert int(re.search(r"#define RELPOSE_RANSAC_OVERFLOW \((-\d+)\)", h).group(1)) == _lib.RANSAC_OVERFLOW
    assert int(re.search(r"#define RELPOSE_RANSAC_MAX_ITERATIONS (\d+)", h).group(1)) == _lib.RANSAC_MAX_ITERATIONS == M.MAX_ITERATIONS
    assert int(re.search(r"#define RELPOSE_RANSAC_MAX_VALIDATIONS (\d+)", h).group(1)) == _lib.RANSAC_MAX_VALIDATIONS == M.MAX_VALIDATIONS
    assert int(re.search(r"#define RELPOSE_RANSAC_MAX_ITERATIONS_LIMIT (\d+)", h).group(1)) == _lib.RANSAC_MAX_ITERATIONS_LIMIT
    assert int(re.search(r"#define RELPOSE_RANSAC_MAX_VALIDATIONS_LIMIT (\d+)", h).group(1)) == _lib.RANSAC_MAX_VALIDATIONS_LIMIT
    assert ("ransac.hip", ["-ffp-contract=off"]) in build.SOURCES
    for sym in ("relpose_ransac_workspace_bytes", "relpose_ransac"):
        assert sym in _lib.SIGNATURES
    assert baselines.STATUS[4] == "no hypothesis" and baselines.STATUS[3] == "overflow"


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_ransac_args_layout_matches_ctypes(tmp_path):
    from relativepose_amd import _lib
    fields = [f for f, _ in _lib.RansacArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(RelposeRansacArgs));\n' +
                   "".join(f'  printf(" %zu", offsetof(RelposeRansacArgs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.RansacArgs)
    assert got[1:] == [getattr(_lib.RansacArgs, f).offset for f in fields]


def test_workspace_sizes_and_invalid_arguments():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    w1, w32 = L.relpose_ransac_workspace_bytes(1, 25600, 32768, 0, 0), L.relpose_ransac_workspace_bytes(32, 25600, 32768, 0, 0)
    assert w32 > w1 > L.relpose_fgr_workspace_bytes(1, 25600, 32768) // 2 > 0
    assert L.relpose_ransac_workspace_bytes(1, 25600, 32768, 4000000, 500) == w1          # 0 = the reference's values
    assert L.relpose_ransac_workspace_bytes(1, 25600, 32768, 8000000, 500) > w1           # the pass bits grow with max_iterations
    assert L.relpose_ransac_workspace_bytes(1, 25600, 32768, 4000000, 1000) > w1
    for bad in ((0, 100, 100, 0, 0), (1, 0, 100, 0, 0), (1, 100, 0, 0, 0), (1, 100, 65537, 0, 0), (1, 100, 100, -1, 0),
                (1, 100, 100, _lib.RANSAC_MAX_ITERATIONS_LIMIT + 1, 0), (1, 100, 100, 0, _lib.RANSAC_MAX_VALIDATIONS_LIMIT + 1)):
        assert L.relpose_ransac_workspace_bytes(*bad) == 0, bad
    a = _lib.RansacArgs()
    a.struct_size = C.sizeof(a)
    assert L.relpose_ransac(C.byref(a)) == -1                       # no clouds / outputs: RELPOSE_EINVAL before touching a device
    assert L.relpose_ransac(None) == -1
    a.struct_size = 4
    assert L.relpose_ransac(C.byref(a)) == -1


def test_meta_kernel_shapes():
    import torch
    from relativepose_amd import ops
    assert "global_registration" in ops.OPS
    pose, status = torch.ops.relpose.global_registration(torch.empty(64, 102400, 3, dtype=torch.float64, device="meta"),
                                                         torch.empty(64, 102400, dtype=torch.uint8, device="meta"))
    assert pose.shape == (32, 4, 4) and pose.dtype == torch.float64 and status.shape == (32,) and status.dtype == torch.int32


def test_evaluation_refuses_what_gs_cannot_run():
    from relativepose_amd import evaluation
    with pytest.raises(SystemExit, match="one GPU"):
        evaluation.main(["--method", "gs", "--gpus", "2", "--dataset", "suncg"])
    with pytest.raises(SystemExit, match="full-resolution"):
        evaluation.main(["--method", "gs", "--dataset", "scannet"])
