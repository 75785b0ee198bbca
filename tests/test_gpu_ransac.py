"""GPU: the batched RANSAC feature registration (csrc/ransac.hip, relpose_ransac) against the numpy model of its contract
(tests/ransac_model.py) and against relpose_fgr's front end, and its uses: baselines.open3d_global_registration,
torch.ops.relpose.global_registration and evaluation --method gs.  Reference: baselines.py:52-81."""
import numpy as np
import pytest

import fgr_scenes as S
import ransac_model as M
from gpu_util import log
from test_ransac_cpu import MAX_DEG, MAX_T, SEEDS

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _room_clouds(n, seed):
    import torch
    from relativepose_amd import synth, util
    d = synth.make_pairs(n, seed, "suncg")
    return util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(2 * n, *d["depth"].shape[2:])).to(_dev()), "suncg")


def _check_against_model(pc, valid, max_validations, tag):
    """Every stage of every pair of (pc, valid) against the model and the front end against relpose_fgr's."""
    from relativepose_amd import baselines
    pose, status, out = baselines.global_registration_dev(pc, valid, max_validations=max_validations, stages=True)
    pose, status, out = pose.cpu().numpy(), status.cpu().numpy(), _np(out)
    _, _, fst = baselines.fast_global_registration_dev(pc, valid, stages=True)
    fst = _np(fst)
    for k in ("down_count", "down_points", "fpfh"):
        assert np.array_equal(out[k], fst[k]), k
    pcn, vn = pc.cpu().numpy(), valid.cpu().numpy().astype(bool)
    for b in range(len(status)):
        r = M.register(pcn[2 * b][vn[2 * b]], pcn[2 * b + 1][vn[2 * b + 1]], max_validations=max_validations)
        assert status[b] == r["status"], (b, status[b], r["status"])
        if "nn" in r:
            ns = len(r["down_src"])
            assert np.array_equal(out["nn"][b, :ns], r["nn"])
            nv = r["n_validations"]
            assert out["n_validations"][b] == nv and out["n_iterations"][b] == r["n_iterations"]
            assert np.array_equal(out["val_iter"][b, :nv], r["val_iter"])
            assert np.array_equal(out["val_inliers"][b, :nv], r["val_inliers"])
            assert np.array_equal(out["val_err"][b, :nv].view(np.uint64), r["val_err"].view(np.uint64))
            assert out["best_index"][b] == r["best_index"]
            assert out["fitness"][b] == r["fitness"] and out["inlier_rmse"][b] == r["inlier_rmse"]
        dp = np.abs(pose[b] - r["pose"]).max()
        assert dp <= 1e-12, dp
        log(tag, pair=b, status=int(status[b]), n_iterations=int(out["n_iterations"][b]), n_validations=int(out["n_validations"][b]),
            best=int(out["best_index"][b]), fitness=float(out["fitness"][b]), pose_err=float(dp))


def test_stages_match_the_model_on_planted_pairs():
    import torch
    from relativepose_amd import baselines
    pairs = [S.planted_pair(s, density=800.0) for s in (10, 11)]
    pc, valid = baselines.pack_clouds([c for s, t, _ in pairs for c in (s, t)])
    _check_against_model(torch.from_numpy(pc).to(_dev()), torch.from_numpy(valid).to(_dev()), 40, "ransac_planted")


def test_stages_match_the_model_on_room_clouds():
    # pairs 0 and 1 of this batch: the symmetric box rooms mostly give no hypothesis with an inlier (status 4, pair 0); pair 1 registers
    pc, valid = _room_clouds(2, 500)
    _check_against_model(pc, valid, 12, "ransac_room")


def test_batch_of_32_equals_single_calls_and_repeats_bitwise():
    from relativepose_amd import baselines
    pc, valid = _room_clouds(32, 500)
    p1, s1, o1 = baselines.global_registration_dev(pc, valid, stages=True)
    p2, s2, o2 = baselines.global_registration_dev(pc, valid, stages=True)
    assert np.array_equal(p1.cpu().numpy(), p2.cpu().numpy()) and np.array_equal(s1.cpu().numpy(), s2.cpu().numpy())
    for k in o1:
        assert np.array_equal(o1[k].cpu().numpy(), o2[k].cpu().numpy()), k
    o1 = _np(o1)
    for b in range(32):
        pb, sb, ob = baselines.global_registration_dev(pc[2 * b:2 * b + 2], valid[2 * b:2 * b + 2], stages=True)
        assert np.array_equal(pb.cpu().numpy()[0], p1.cpu().numpy()[b]), b
        assert int(sb[0]) == int(s1[b])
        for k, v in _np(ob).items():
            big = o1[k]
            sl = big[2 * b:2 * b + 2] if big.shape[0] == 64 else big[b:b + 1]
            assert np.array_equal(v, sl), (b, k)
    log("ransac_batch32", status=s1.cpu().numpy(), n_iterations=o1["n_iterations"], fitness=o1["fitness"])


def test_overflow_returns_true_counts():
    import ctypes as C
    import torch
    from relativepose_amd import _lib, baselines
    import fgr_model as F
    a_, b_, _ = S.planted_pair(0, density=300.0)
    c_, d_, _ = S.planted_pair(1, density=300.0)
    pc, valid = baselines.pack_clouds([a_, b_, c_[:40], d_[:40]])
    pcd, vd = torch.from_numpy(pc).to(_dev()), torch.from_numpy(valid).to(_dev())
    pose, status, out = baselines.global_registration_dev(pcd, vd, max_points=64, max_iterations=100000, max_validations=20, stages=True)
    ns, nt = len(F.voxel_down(a_)[0]), len(F.voxel_down(b_)[0])
    assert ns > 64 and nt > 64
    assert out["down_count"].cpu().numpy()[:2].tolist() == [ns, nt]
    assert int(status[0]) == M.STATUS_OVERFLOW and np.array_equal(pose[0].cpu().numpy(), np.eye(4))
    assert out["down_points"].shape[1] == 64
    r = M.register(c_[:40], d_[:40], max_points=64, max_iterations=100000, max_validations=20)        # the other pair is complete
    assert int(status[1]) == r["status"] and np.abs(pose[1].cpu().numpy() - r["pose"]).max() <= 1e-12
    assert int(out["n_validations"][1]) == r["n_validations"] and int(out["n_iterations"][1]) == r["n_iterations"]
    a = _lib.RansacArgs()                                            # the raw return code
    a.struct_size = C.sizeof(a)
    wsb = _lib.lib().relpose_ransac_workspace_bytes(2, pc.shape[1], 64, 100000, 20)
    ws = torch.empty(wsb, dtype=torch.uint8, device=_dev())
    a.n_pairs, a.n_points, a.max_points, a.max_iterations, a.max_validations = 2, pc.shape[1], 64, 100000, 20
    a.pc, a.valid, a.pose, a.status = pcd.data_ptr(), vd.data_ptr(), pose.data_ptr(), status.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), wsb, _lib.stream_ptr()
    assert _lib.lib().relpose_ransac(C.byref(a)) == _lib.RANSAC_OVERFLOW


@pytest.mark.parametrize("seed", SEEDS)
def test_planted_motion_on_the_gpu(seed):
    from relativepose_amd import baselines
    src, tgt, T = S.planted_pair(seed)
    T_hat = baselines.open3d_global_registration(src, tgt)
    deg, dt = S.pose_error(T_hat, T)
    log("ransac_planted_gpu", seed=seed, deg=deg, t=dt)
    assert deg < MAX_DEG and dt < MAX_T, (deg, dt)


def test_torch_op_matches_the_direct_call():
    import torch
    from relativepose_amd import baselines, ops  # noqa: F401
    pc, valid = _room_clouds(4, 77)
    p1, s1 = torch.ops.relpose.global_registration(pc, valid)
    p2, s2, _ = baselines.global_registration_dev(pc, valid)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    assert p1.shape == (4, 4, 4) and s1.dtype == torch.int32


def test_evaluation_method_gs_writes_reference_records(tmp_path, capsys):
    from relativepose_amd import evaluation
    exp = str(tmp_path / "gs")
    evaluation.main(["--method", "gs", "--dataset", "suncg", "--pairs", "64", "--batch", "32", "--exp", exp])
    recs = evaluation.load_results(exp + ".result.npy")
    keys = {'img_src', 'img_tgt', 'err_ad', 'err_t', 'err_blind', 'err_t_blind', 'overlap', 'pc_dist', 'cam_dist', 'pc_nearest', 'R_gt',
            'R_pred_44', 'status'}
    assert 0 < len(recs) <= 64
    assert all(set(r) == keys for r in recs)
    assert all(r['overlap'] >= 0.1 for r in recs)
    out = capsys.readouterr().out
    assert '"method": "gs"' in out
    log("ransac_evaluation", records=len(recs), stats=evaluation.summarize(recs))
