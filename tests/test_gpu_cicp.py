"""GPU: the batched coloured ICP (csrc/cicp.hip, relpose_cicp) against the numpy model of its contract (tests/cicp_model.py, DESIGN.md
§4.8), layered and teacher-forced -- every stage of the model is fed the GPU's own upstream results, so a one-ulp difference upstream
cannot flip a correspondence downstream -- and its uses: baselines.color_registration_dev / open3d_color_registration,
torch.ops.relpose.colored_icp / color_registration and evaluation --method cgs.  Reference: baselines.py:110-168."""
import numpy as np
import pytest

import cicp_model as M
import cicp_scenes as S
from gpu_util import log
from test_cicp_cpu import MAX_DEG, MAX_T, SEEDS

pytestmark = pytest.mark.gpu

CAP = 16384          # the planted clouds have about 8000 voxels at the 1 cm level
GS_SCALE = 1.5       # the scene of the tests that start from RANSAC: FPFH (radius 0.25 m) needs more than a 1 m scene; about 19000 voxels at 1 cm


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _pack(pairs):
    """[(src, tgt, col_src, col_tgt, ...)] -> pc, color, valid CUDA tensors."""
    import torch
    from relativepose_amd import baselines
    pc, valid = baselines.pack_clouds([c for p in pairs for c in (p[0], p[1])])
    col, _ = baselines.pack_clouds([c for p in pairs for c in (p[2], p[3])])
    return torch.from_numpy(pc).to(_dev()), torch.from_numpy(col).to(_dev()), torch.from_numpy(valid).to(_dev())


def _run(pairs, inits, lam=M.LAMBDA_GEOMETRIC, cap=CAP):
    import torch
    from relativepose_amd import baselines
    pc, col, valid = _pack(pairs)
    init = None if inits is None else torch.from_numpy(np.stack(inits)).to(_dev())
    pose, status, out = baselines.colored_icp_dev(pc, col, valid, init=init, lambda_geometric=lam, max_points=cap, stages=True)
    return pose.cpu().numpy(), status.cpu().numpy(), _np(out)


@pytest.fixture(scope="module")
def planted():
    """Two planted pairs from a perturbed truth at the default lambda, and the textured plane at lambda = 1 (its level never meets the stop
    rule early, so every level runs to its iteration cap), each with the free-running model."""
    pairs = [S.planted_pair(s) for s in SEEDS[:2]]
    inits = [S.perturbed(p[4], s) for p, s in zip(pairs, SEEDS)]
    plane = S.textured_plane(0)
    runs = [(pairs, inits, M.LAMBDA_GEOMETRIC), ([plane], [np.eye(4)], 1.0)]
    out = []
    for prs, ini, lam in runs:
        models = [M.register(p[0], p[2], p[1], p[3], T0, lam=lam, max_points=CAP) for p, T0 in zip(prs, ini)]
        out.append({"pairs": prs, "inits": ini, "lam": lam, "gpu": _run(prs, ini, lam), "model": models})
    return out


def test_voxels_colours_and_normals_match_the_model(planted):
    for run in planted:
        _, status, out = run["gpu"]
        for b, m in enumerate(run["model"]):
            assert status[b] == m["status"] == M.STATUS_OK
            for l, lv in enumerate(m["levels"]):
                for c, (kp, kc) in ((2 * b, ("ps", "cs")), (2 * b + 1, ("pt", "ct"))):
                    n = len(lv[kp])
                    assert out["down_count"][c, l] == n
                    assert np.array_equal(out["down_points"][c, l, :n].view(np.uint64), lv[kp].view(np.uint64)), (b, l, c)
                    assert np.array_equal(out["down_colors"][c, l, :n].view(np.uint64), lv[kc].view(np.uint64)), (b, l, c)
                nt = len(lv["pt"])
                dn = np.abs(out["normals"][b, l, :nt] - lv["normals"]).max()
                log("cicp_normals", pair=b, level=l, voxels=nt, max_diff=float(dn), fallback=int((lv["ncnt"] < 3).sum()))
                assert dn <= 1e-9, (b, l, dn)


def test_gradients_match_the_model_fed_the_gpu_normals(planted):
    for run in planted:
        out = run["gpu"][2]
        for b, m in enumerate(run["model"]):
            for l, lv in enumerate(m["levels"]):
                nt = len(lv["pt"])
                g = M.gradients(lv["pt"], M.intensity(lv["ct"]), out["normals"][b, l, :nt], lv["nbr"], lv["ncnt"])
                got = out["gradient"][b, l, :nt]
                scale = np.abs(g).max()
                d = np.abs(got - g).max()
                log("cicp_gradient", pair=b, level=l, scale=float(scale), max_diff=float(d), zero=int((np.abs(g).sum(1) == 0).sum()))
                assert scale > 0 and d <= 1e-12 * scale, (b, l, d, scale)


def test_every_iteration_matches_the_model_from_the_gpu_pose(planted):
    for r, run in enumerate(planted):
        _, _, out = run["gpu"]
        for b, m in enumerate(run["model"]):
            T_carry = run["inits"][b]
            for l, (radius, cap_it) in enumerate(zip(M.RADII, M.MAX_ITER)):
                ns, nt = out["down_count"][2 * b, l], out["down_count"][2 * b + 1, l]
                lv = {"ps": out["down_points"][2 * b, l, :ns], "cs": out["down_colors"][2 * b, l, :ns],
                      "pt": out["down_points"][2 * b + 1, l, :nt], "ct": out["down_colors"][2 * b + 1, l, :nt],
                      "normals": out["normals"][b, l, :nt], "gradient": out["gradient"][b, l, :nt]}
                nit = int(out["n_iterations"][b, l])
                assert 1 <= nit <= cap_it
                # the level starts from the pose the previous one ended with, bit for bit
                assert np.array_equal(out["iter_pose"][b, M.SLOT_OFF[l]], T_carry), (b, l)
                prev = None
                for k in range(nit):
                    slot = M.SLOT_OFF[l] + k
                    T = out["iter_pose"][b, slot]
                    s = M.step(lv, T, radius, run["lam"], prev)
                    assert np.array_equal(out["iter_corr"][b, slot, :ns], s["corr"]), (b, l, k)
                    assert out["iter_ncorr"][b, slot] == s["ncorr"]
                    assert np.array_equal(out["iter_rmse"][b, slot:slot + 1].view(np.uint64), np.array([s["rmse"]]).view(np.uint64)), (b, l, k)
                    T_next = out["iter_pose"][b, slot + 1] if k + 1 < nit else out["level_pose"][b, l]
                    dx = 0.0
                    if s["x"] is not None:
                        dx = float(np.abs(out["iter_x"][b, slot] - s["x"]).max() / np.abs(s["x"]).max())
                        assert dx <= 1e-12, (b, l, k, dx)
                    dT = float(np.abs(T_next - s["T_next"]).max())
                    assert dT <= 1e-12, (b, l, k, dT)
                    if k + 1 < cap_it:                        # the stop decision: the level ended here iff the model says so
                        assert s["ended"] == (k + 1 == nit), (b, l, k)
                    prev = (s["fitness"], s["rmse"])
                    log("cicp_iteration", run=r, pair=b, level=l, k=k, ncorr=s["ncorr"], rmse=s["rmse"], ended=bool(s["ended"]), x_rel=dx, pose_diff=dT)
                assert out["fitness"][b, l] == prev[0] and out["inlier_rmse"][b, l] == prev[1]
                T_carry = out["level_pose"][b, l]
            assert np.array_equal(run["gpu"][0][b], T_carry)
    assert planted[1]["gpu"][2]["n_iterations"][0].tolist() == list(M.MAX_ITER)        # the plane at lambda 1 ran every level to its cap


def test_final_pose_recovers_the_planted_motion(planted):
    run = planted[0]
    pose = run["gpu"][0]
    for b, (p, m) in enumerate(zip(run["pairs"], run["model"])):
        deg, dt = S.pose_error(pose[b], p[4])
        log("cicp_planted_gpu", pair=b, deg=deg, t=dt, n_iterations=run["gpu"][2]["n_iterations"][b], model_n_iterations=m["n_iterations"],
            free_running_diff=float(np.abs(pose[b] - m["pose"]).max()))
        assert deg < MAX_DEG and dt < MAX_T, (deg, dt)


@pytest.mark.parametrize("seed", SEEDS)
def test_cgs_improves_on_gs_for_planted_pairs(seed):
    from relativepose_amd import baselines
    p = S.planted_pair(seed, scale=GS_SCALE)
    pc, col, valid = _pack([p])
    pose, status, out = baselines.color_registration_dev(pc, col, valid, seed=0)
    e_gs = S.pose_error(out["ransac_pose"][0].cpu().numpy(), p[4])
    e_cgs = S.pose_error(pose[0].cpu().numpy(), p[4])
    log("cicp_cgs_vs_gs", seed=seed, gs=e_gs, cgs=e_cgs, ransac_status=int(out["ransac_status"][0]), status=int(status[0]),
        n_iterations=out["n_iterations"][0].cpu().numpy())
    assert int(status[0]) == 0
    assert e_cgs[0] < e_gs[0] and e_cgs[1] < e_gs[1], (e_gs, e_cgs)
    assert e_cgs[0] < MAX_DEG and e_cgs[1] < MAX_T, e_cgs


def _room_batch(n, seed):
    import torch
    from relativepose_amd import evaluation, synth, util
    d = synth.make_pairs(n, seed, "suncg")
    pc, valid = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(2 * n, *d["depth"].shape[2:])).to(_dev()), "suncg")
    col = torch.from_numpy(evaluation.observed_colors(d["rgb"].reshape(2 * n, *d["rgb"].shape[2:]))).to(_dev())
    return pc, col, valid


def test_batch_of_32_equals_single_calls_and_repeats_bitwise():
    from relativepose_amd import baselines
    pc, col, valid = _room_batch(32, 500)
    p1, s1, o1 = baselines.colored_icp_dev(pc, col, valid, stages=True)
    p2, s2, o2 = baselines.colored_icp_dev(pc, col, valid, stages=True)
    assert np.array_equal(p1.cpu().numpy(), p2.cpu().numpy()) and np.array_equal(s1.cpu().numpy(), s2.cpu().numpy())
    for k in o1:
        assert np.array_equal(o1[k].cpu().numpy(), o2[k].cpu().numpy()), k
    del o2
    o1, p1 = _np(o1), p1.cpu().numpy()
    for b in range(32):
        pb, sb, ob = baselines.colored_icp_dev(pc[2 * b:2 * b + 2], col[2 * b:2 * b + 2], valid[2 * b:2 * b + 2], stages=True)
        assert np.array_equal(pb.cpu().numpy()[0], p1[b]), b
        assert int(sb[0]) == int(s1[b])
        for k, v in _np(ob).items():
            big = o1[k]
            sl = big[2 * b:2 * b + 2] if big.shape[0] == 64 else big[b:b + 1]
            assert np.array_equal(v, sl), (b, k)
    log("cicp_batch32", status=s1.cpu().numpy(), n_iterations=o1["n_iterations"], fitness=o1["fitness"])
    assert (o1["n_iterations"] >= 1).all() and (o1["fitness"][:, 2] > 0).any()


def test_overflow_at_one_level_returns_true_counts():
    import ctypes as C
    import torch
    from relativepose_amd import _lib, baselines
    big = S.planted_pair(0)
    small = tuple(a[:400] for a in S.planted_pair(1)[:4])
    m = M.register(big[0], big[2], big[1], big[3], max_points=4096)
    counts = [[len(lv["ps"]), len(lv["pt"])] for lv in m["levels"]]
    assert max(counts[0] + counts[1]) <= 4096 < min(counts[2]) and m["status"] == M.STATUS_OVERFLOW      # only the 1 cm level overflows
    pc, col, valid = _pack([big, small])
    pose, status, out = baselines.colored_icp_dev(pc, col, valid, max_points=4096, stages=True)
    assert out["down_count"].cpu().numpy()[:2].T.tolist() == counts
    assert int(status[0]) == M.STATUS_OVERFLOW and np.array_equal(pose[0].cpu().numpy(), np.eye(4))
    assert np.array_equal(out["level_pose"][0].cpu().numpy(), np.tile(np.eye(4), (3, 1, 1))) and out["n_iterations"][0].tolist() == [0, 0, 0]
    assert out["down_points"].shape[2] == 4096
    ms = M.register(small[0], small[2], small[1], small[3], max_points=4096)          # the other pair is complete
    assert int(status[1]) == ms["status"] == M.STATUS_OK and (out["n_iterations"][1] >= 1).all()
    p1, s1, o1 = baselines.colored_icp_dev(pc[2:4], col[2:4], valid[2:4], max_points=4096, stages=True)
    assert torch.equal(p1[0], pose[1]) and torch.equal(o1["iter_corr"][0], out["iter_corr"][1]) and torch.equal(o1["fitness"][0], out["fitness"][1])
    a = _lib.CicpArgs()                                              # the raw return code
    a.struct_size = C.sizeof(a)
    wsb = _lib.lib().relpose_cicp_workspace_bytes(2, pc.shape[1], 4096)
    ws = torch.empty(wsb, dtype=torch.uint8, device=_dev())
    a.n_pairs, a.n_points, a.max_points, a.lambda_geometric = 2, pc.shape[1], 4096, M.LAMBDA_GEOMETRIC
    a.pc, a.valid, a.color, a.pose, a.status = pc.data_ptr(), valid.data_ptr(), col.data_ptr(), pose.data_ptr(), status.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), wsb, _lib.stream_ptr()
    assert _lib.lib().relpose_cicp(C.byref(a)) == _lib.CICP_OVERFLOW


def test_voxel_edge_cases_match_the_model_bitwise():
    """The shared scan, compaction and sort (csrc/cloud_prims.h) where they can go wrong, at the three voxel sizes:
    fgr_scenes.voxel_edge_clouds, with max_points below the voxel count of the sparse clouds (the first max_points voxels in key order are
    kept, the count is the true one)."""
    import torch
    import fgr_scenes
    from relativepose_amd import baselines
    cap = 1024
    names, pc, valid, col = fgr_scenes.voxel_edge_clouds(M.RADII[0])
    dev = _dev()
    pose, status, out = baselines.colored_icp_dev(torch.from_numpy(pc).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(valid).to(dev),
                                                  max_points=cap, stages=True)
    out = _np(out)
    bits, over = {}, {}
    for c, name in enumerate(names):
        m = valid[c] != 0
        for l, vox in enumerate(M.RADII):
            dp, dc = M.voxel_down(pc[c][m], col[c][m], vox)
            n = len(dp)
            bits[name, l], over[name, l] = (fgr_scenes.key_bits(pc[c][m], vox) if m.any() else -1), n > cap
            log("cicp_voxel_edge", cloud=name, level=l, valid=int(m.sum()), bits=bits[name, l], voxels=n)
            assert out["down_count"][c, l] == n, (name, l)
            assert np.array_equal(out["down_points"][c, l, :min(n, cap)].view(np.uint64), dp[:cap].view(np.uint64)), (name, l)
            assert np.array_equal(out["down_colors"][c, l, :min(n, cap)].view(np.uint64), dc[:cap].view(np.uint64)), (name, l)
    # the cases reach what they are meant to
    assert all(bits["empty", l] == -1 and bits["one_cell", l] == 0 and over["sparse", l] for l in range(3))
    assert bits["sparse", 0] % 4 and bits["sparse", 1] % 4 and bits["sparse", 2] % 4 == 0 and bits["dense", 0] % 4 and not over["dense", 1]
    assert status.cpu().numpy().tolist() == [M.STATUS_FEW_POINTS, M.STATUS_OVERFLOW, M.STATUS_OVERFLOW]
    assert np.array_equal(pose.cpu().numpy(), np.tile(np.eye(4), (3, 1, 1)))


def test_too_few_points_gives_the_identity():
    import torch
    from relativepose_amd import baselines
    p = S.planted_pair(0)
    tiny = (p[0][:2], p[1][:300], p[2][:2], p[3][:300])
    pc, col, valid = _pack([tiny])
    init = torch.from_numpy(S.perturbed(p[4], 0)[None]).to(_dev())
    pose, status, out = baselines.colored_icp_dev(pc, col, valid, init=init, max_points=4096)
    assert int(status[0]) == M.STATUS_FEW_POINTS and np.array_equal(pose[0].cpu().numpy(), np.eye(4))


def test_init_none_equals_the_identity_bitwise():
    import torch
    from relativepose_amd import baselines
    pc, col, valid = _room_batch(2, 77)
    eye = torch.eye(4, dtype=torch.float64, device=_dev()).repeat(2, 1, 1)
    p1, s1, o1 = baselines.colored_icp_dev(pc, col, valid, stages=True)
    p2, s2, o2 = baselines.colored_icp_dev(pc, col, valid, init=eye, stages=True)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k


def test_torch_ops_match_the_direct_calls():
    import torch
    from relativepose_amd import baselines, ops  # noqa: F401
    pc, col, valid = _room_batch(2, 78)
    init = torch.eye(4, dtype=torch.float64, device=_dev()).repeat(2, 1, 1)
    init[:, 0, 3] = 0.01
    p1, s1 = torch.ops.relpose.colored_icp(pc, col, valid, init)
    p2, s2, _ = baselines.colored_icp_dev(pc, col, valid, init=init)
    assert torch.equal(p1, p2) and torch.equal(s1, s2) and p1.shape == (2, 4, 4) and s1.dtype == torch.int32
    p3, s3 = torch.ops.relpose.color_registration(pc, col, valid)
    p4, s4, _ = baselines.color_registration_dev(pc, col, valid)
    assert torch.equal(p3, p4) and torch.equal(s3, s4)


def test_open3d_color_registration_recovers_the_planted_motion():
    from relativepose_amd import baselines
    src, tgt, cs, ct, T = S.planted_pair(SEEDS[1], scale=GS_SCALE)
    T_hat = baselines.open3d_color_registration(src, tgt, cs, ct)
    deg, dt = S.pose_error(T_hat, T)
    log("cicp_open3d_call", deg=deg, t=dt)
    assert T_hat.shape == (4, 4) and deg < MAX_DEG and dt < MAX_T, (deg, dt)


def test_evaluation_method_cgs_writes_reference_records(tmp_path, capsys):
    from relativepose_amd import evaluation
    exp = str(tmp_path / "cgs")
    evaluation.main(["--method", "cgs", "--dataset", "suncg", "--pairs", "64", "--batch", "32", "--exp", exp])
    recs = evaluation.load_results(exp + ".result.npy")
    keys = {'img_src', 'img_tgt', 'err_ad', 'err_t', 'err_blind', 'err_t_blind', 'overlap', 'pc_dist', 'cam_dist', 'pc_nearest', 'R_gt',
            'R_pred_44', 'status'}
    assert 0 < len(recs) <= 64
    assert all(set(r) == keys for r in recs)
    assert all(r['overlap'] >= 0.1 for r in recs)
    out = capsys.readouterr().out
    assert '"method": "cgs"' in out
    log("cicp_evaluation", records=len(recs), stats=evaluation.summarize(recs))
