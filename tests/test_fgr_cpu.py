"""CPU: the FPFH + fast global registration contract's numpy model (tests/fgr_model.py) and the C ABI of relpose_fgr."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fgr_model as M
import fgr_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the model: seeds 0-5 of planted_pair give 0.61-3.03 degrees and 1.1-2.8 cm; the bounds leave a third on top.
MAX_DEG, MAX_T = 4.0, 0.04
SEEDS = (0, 1, 2)


@pytest.mark.parametrize("seed", SEEDS)
def test_model_recovers_planted_motion(seed):
    src, tgt, T = S.planted_pair(seed)
    r = M.register(src, tgt)
    assert r["status"] == M.STATUS_OK
    deg, dt = S.pose_error(r["pose"], T)
    assert deg < MAX_DEG and dt < MAX_T, (deg, dt)


def test_voxel_means_equal_a_direct_computation():
    rs = np.random.RandomState(3)
    pts = rs.uniform(-1.0, 1.0, (4000, 3)) * np.r_[1.0, 0.5, 0.3]
    down, ix, keys = M.voxel_down(pts)
    mb = pts.min(0) - 0.5 * M.VOXEL
    acc = {}
    for p in pts:                                        # plain sequential sums, input order
        k = tuple(int(v) for v in np.floor((p - mb) / M.VOXEL))
        s = acc.setdefault(k, [0.0, 0.0, 0.0, 0])
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += 1
    ref = np.array([[s[0] / s[3], s[1] / s[3], s[2] / s[3]] for _, s in sorted(acc.items())])
    assert down.shape == ref.shape
    assert np.array_equal(down, ref)
    assert np.array_equal(ix, np.array([k[0] for k in sorted(acc)]))
    assert (np.diff(keys) > 0).all()


def test_jacobi_normals_match_eigh_and_face_the_origin():
    src, _, _ = S.planted_pair(7, density=600.0)
    pts, _, _ = M.voxel_down(src)
    idx, d2, cnt = M.neighbors(pts)
    nrm = M.normals(pts, idx, d2, cnt)
    inr = (d2 < M.R_NORMAL ** 2) & (np.arange(idx.shape[1])[None] < cnt[:, None])
    m = np.minimum(np.where(inr.all(1), idx.shape[1], np.argmin(inr, 1)), M.NN_NORMAL)
    cov = M.covariances(pts, idx, m)
    ok = m >= 3
    w, v = np.linalg.eigh(cov[ok])
    gap = w[:, 1] - w[:, 0]
    sel = gap > 1e-6 * np.maximum(w[:, 2], 1e-300)        # a well-separated smallest eigenvalue
    ref = v[:, :, 0][sel]
    got = nrm[ok][sel]
    assert sel.sum() > 0.9 * ok.sum()
    assert np.abs(np.abs((ref * got).sum(1)) - 1).max() < 1e-9
    assert np.abs(np.abs(ref) - np.abs(got)).max() < 1e-9 or np.minimum(np.abs(ref - got), np.abs(ref + got)).max() < 1e-9
    assert ((nrm * (0.0 - pts)).sum(1) >= 0).all()
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0)


def test_fpfh_is_invariant_to_a_rigid_motion():
    src, _, _ = S.planted_pair(8, density=600.0)
    pts, _, _ = M.voxel_down(src)
    R = S.rotation([0.3, -0.5, 0.8], 41.0)
    t = np.r_[0.4, -0.2, 0.3]
    a = M.features(pts)
    b = M.features(pts @ R.T + t, origin=t)               # the sensor moves with the cloud
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["cnt"], b["cnt"])
    assert np.abs(a["normal"] @ R.T - b["normal"]).max() < 1e-9
    # a pair feature on a bin edge may round to the other side after the motion and moves 100/k of one block of one SPFH; FPFH
    # spreads it over that point's neighbours with a small weight.  Measured: median 2e-16, 99th percentile 1.3e-3 (relative L1)
    l1 = np.abs(a["fpfh"] - b["fpfh"]).sum(1) / np.abs(a["fpfh"]).sum(1)
    assert np.median(l1) < 1e-12 and np.percentile(l1, 99) < 1e-2
    assert (M.nn_f32(a["fpfh"], b["fpfh"]) == np.arange(len(pts))).mean() > 0.99      # every point still finds itself
    assert np.abs(a["fpfh"][:, :11].sum(1)[a["cnt"] > 1] - 200).max() < 1e-9      # each block: SPFH 100 + weighted neighbours 100


def test_angle_bins_follow_atan2_away_from_the_edges():
    rs = np.random.RandomState(0)
    th = rs.uniform(-np.pi, np.pi, 20000)
    r = rs.uniform(0.1, 2.0, th.size)
    ref = np.clip(np.floor(11 * (th + np.pi) / (2 * np.pi)), 0, 10).astype(int)
    got = M.angle_bin(r * np.cos(th), r * np.sin(th))
    edge = np.abs((11 * (th + np.pi) / (2 * np.pi)) - np.round(11 * (th + np.pi) / (2 * np.pi))) < 1e-9
    assert np.array_equal(got[~edge], ref[~edge])
    assert np.allclose(M.EDGE_COS, np.cos(-np.pi + 2 * np.pi * np.arange(1, 11) / 11), atol=1e-15)
    assert np.allclose(M.EDGE_SIN, np.sin(-np.pi + 2 * np.pi * np.arange(1, 11) / 11), atol=1e-15)


def test_the_kernel_and_the_model_share_the_edge_literals():
    src = open(os.path.join(ROOT, "relativepose_amd", "csrc", "fgr.hip")).read()
    for name, arr in (("kEdgeCos", M.EDGE_COS), ("kEdgeSin", M.EDGE_SIN)):
        body = re.search(name + r"\[10\] = \{([^}]*)\}", src).group(1)
        assert np.array_equal(np.array([float(x) for x in body.split(",")]), arr)


def test_tuple_draws_are_a_counter_hash():
    a = M.tuple_draw(5, np.arange(1000), 0, 37)
    assert np.array_equal(a, M.tuple_draw(5, np.arange(1000), 0, 37))
    assert not np.array_equal(a, M.tuple_draw(6, np.arange(1000), 0, 37))
    assert a.min() >= 0 and a.max() < 37 and len(np.unique(a)) == 37
    x = 0x9E3779B97F4A7C15 * 5 + 3 * 17 + 2
    x &= M.M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M.M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M.M64
    x ^= x >> 31
    assert int(M.tuple_draw(5, np.array([17]), 2, 1000003)[0]) == x % 1000003


def test_too_few_points_and_overflow_status():
    assert M.register(np.zeros((0, 3)), np.random.rand(100, 3))["status"] == M.STATUS_FEW_POINTS
    src, tgt, _ = S.planted_pair(0, density=300.0)
    r = M.register(src, tgt, max_points=50)
    assert r["status"] == M.STATUS_OVERFLOW and len(r["down_src"]) > 50


def test_header_declares_the_fgr_symbols():
    h = open(os.path.join(ROOT, "include", "relpose.h")).read()
    for sym in ("relpose_fgr_workspace_bytes", "relpose_fgr"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "typedef struct RelposeFgrArgs" in h and "baselines.py:83-106" in h
    from relativepose_amd import _lib, build
    assert int(re.search(r"#define RELPOSE_FGR_OVERFLOW \((-\d+)\)", h).group(1)) == _lib.FGR_OVERFLOW
    assert int(re.search(r"#define RELPOSE_FGR_MAX_POINTS (\d+)", h).group(1)) == _lib.FGR_MAX_POINTS == M.MAX_POINTS
    assert ("fgr.hip", ["-ffp-contract=off"]) in build.SOURCES
    for sym in ("relpose_fgr_workspace_bytes", "relpose_fgr"):
        assert sym in _lib.SIGNATURES


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_fgr_args_layout_matches_ctypes(tmp_path):
    from relativepose_amd import _lib
    fields = [f for f, _ in _lib.FgrArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "relpose.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(RelposeFgrArgs));\n' +
                   "".join(f'  printf(" %zu", offsetof(RelposeFgrArgs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.FgrArgs)
    assert got[1:] == [getattr(_lib.FgrArgs, f).offset for f in fields]


def test_workspace_sizes_and_invalid_arguments():
    from relativepose_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    assert L.relpose_fgr_workspace_bytes(32, 102400, 16384) > L.relpose_fgr_workspace_bytes(1, 102400, 16384) > 0
    for bad in ((0, 100, 100), (1, 0, 100), (1, 100, 0), (1, 100, 65537)):
        assert L.relpose_fgr_workspace_bytes(*bad) == 0
    a = _lib.FgrArgs()
    a.struct_size = C.sizeof(a)
    assert L.relpose_fgr(C.byref(a)) == -1                          # no clouds / outputs: RELPOSE_EINVAL before touching a device
    assert L.relpose_fgr(None) == -1
    a.struct_size = 4
    assert L.relpose_fgr(C.byref(a)) == -1


def test_meta_kernel_shapes():
    import torch
    from relativepose_amd import ops
    assert "fast_global_registration" in ops.OPS
    pose, status = torch.ops.relpose.fast_global_registration(torch.empty(64, 102400, 3, dtype=torch.float64, device="meta"),
                                                              torch.empty(64, 102400, dtype=torch.uint8, device="meta"))
    assert pose.shape == (32, 4, 4) and pose.dtype == torch.float64 and status.shape == (32,) and status.dtype == torch.int32


def test_evaluation_refuses_what_fgs_cannot_run():
    from relativepose_amd import evaluation
    with pytest.raises(SystemExit, match="one GPU"):
        evaluation.main(["--method", "fgs", "--gpus", "2", "--dataset", "suncg"])
    with pytest.raises(SystemExit, match="full-resolution"):
        evaluation.main(["--method", "fgs", "--dataset", "scannet"])
