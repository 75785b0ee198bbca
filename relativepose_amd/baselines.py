"""The point-cloud registration baselines of the reference (baselines.py), on the GPU.

  open3d_fast_global_registration   baselines.py:83-106 (`--method fgs`): FPFH features + fast global registration, csrc/fgr.hip
  fast_global_registration_dev      the same for a batch of pairs on the device (relpose_fgr)
  open3d_global_registration        baselines.py:52-81 (`--method gs`): the same FPFH front end + RANSAC over feature matches, csrc/ransac.hip
  global_registration_dev           the same for a batch of pairs on the device (relpose_ransac)
  open3d_color_registration         baselines.py:110-168 (`--method cgs`): the gs RANSAC result refined by three levels of coloured ICP, csrc/cicp.hip
  color_registration_dev            the same for a batch of pairs on the device (relpose_ransac, then relpose_cicp)
  colored_icp_dev                   the coloured ICP alone, from any initial pose (relpose_cicp)

The remaining baseline (super4pcs) shells out to a third-party binary and is not implemented.
The contracts are the project's own; Open3D is not a dependency and agreement with it is not tested."""
import ctypes as C

import numpy as np

from . import _lib

STATUS = {0: "ok", 1: "too few points", 2: "too few correspondences", 3: "overflow", 4: "no hypothesis"}


def fast_global_registration_dev(pc, valid, max_points=_lib.FGR_MAX_POINTS, seed=0, stages=False):
    """pc [2B, P, 3] f64 / valid [2B, P] u8 CUDA tensors (util.depth2pc_dev's layout; cloud 2b = the source of pair b, 2b+1 its target)
    -> (pose [B,4,4] f64 with T p_src ~ p_tgt, status [B] i32, stages).  stages=True: a dict of every per-stage output (down_points,
    down_count, nbr_index, nbr_count, normals, fpfh, corr, n_corr, tuple_corr, n_tuples); else an empty dict.
    Raises on an invalid call; a cloud with more than max_points voxels gives its pair status 3 (overflow) and identity."""
    import torch
    _lib.require_gpu()
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.shape[0] % 2 or valid.shape != pc.shape[:2]:
        raise ValueError("pc must be [2B, P, 3] and valid [2B, P]")
    pc = pc.to(torch.float64).contiguous()
    valid = valid.to(torch.uint8).contiguous()
    C2, P = int(pc.shape[0]), int(pc.shape[1])
    B, N, dev = C2 // 2, int(max_points), pc.device
    L = _lib.lib()
    wsb = L.relpose_fgr_workspace_bytes(B, P, N)
    if wsb == 0:
        raise ValueError(f"relpose_fgr: unsupported sizes (pairs {B}, points {P}, max_points {N})")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    pose = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    st = {}
    if stages:
        st = {"down_points": torch.zeros(C2, N, 3, dtype=torch.float64, device=dev), "down_count": torch.zeros(C2, dtype=torch.int32, device=dev),
              "nbr_index": torch.full((C2, N, 100), -1, dtype=torch.int32, device=dev), "nbr_count": torch.zeros(C2, N, dtype=torch.int32, device=dev),
              "normals": torch.zeros(C2, N, 3, dtype=torch.float64, device=dev), "fpfh": torch.zeros(C2, N, 33, dtype=torch.float64, device=dev),
              "corr": torch.zeros(B, N, 2, dtype=torch.int32, device=dev), "n_corr": torch.zeros(B, dtype=torch.int32, device=dev),
              "tuple_corr": torch.zeros(B, 3 * _lib.FGR_MAX_TUPLES, 2, dtype=torch.int32, device=dev),
              "n_tuples": torch.zeros(B, dtype=torch.int32, device=dev)}
    a = _lib.FgrArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_points, a.max_points, a.seed = B, P, N, int(seed)
    a.pc, a.valid, a.pose, a.status = pc.data_ptr(), valid.data_ptr(), pose.data_ptr(), status.data_ptr()
    for k, v in st.items():
        setattr(a, k, v.data_ptr())
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), wsb, _lib.stream_ptr()
    rc = L.relpose_fgr(C.byref(a))
    if rc not in (0, _lib.FGR_OVERFLOW):
        _lib.check(rc, "relpose_fgr")
    return pose, status, st


def pack_clouds(clouds):
    """[pc_0, pc_1, ...] numpy [n_i, 3] -> (pc [len, P, 3] f64, valid [len, P] u8) numpy, P = the largest n_i (at least 1)."""
    P = max(1, max(len(c) for c in clouds))
    pc = np.zeros((len(clouds), P, 3))
    valid = np.zeros((len(clouds), P), np.uint8)
    for i, c in enumerate(clouds):
        pc[i, :len(c)] = c
        valid[i, :len(c)] = 1
    return pc, valid


def open3d_fast_global_registration(pc_src, pc_tgt):
    """baselines.py:83-106: pc_src [n1,3], pc_tgt [n2,3] numpy -> R_hat [4,4] numpy (T p_src ~ p_tgt; identity when the pair has too
    few points or correspondences, or more voxels than RELPOSE_FGR_MAX_POINTS)."""
    import torch
    dev = _lib.require_gpu()
    pc, valid = pack_clouds([np.asarray(pc_src, np.float64).reshape(-1, 3), np.asarray(pc_tgt, np.float64).reshape(-1, 3)])
    pose, _, _ = fast_global_registration_dev(torch.from_numpy(pc).to(dev), torch.from_numpy(valid).to(dev))
    return pose[0].cpu().numpy()


def global_registration_dev(pc, valid, max_points=_lib.FGR_MAX_POINTS, seed=0, max_iterations=_lib.RANSAC_MAX_ITERATIONS,
                            max_validations=_lib.RANSAC_MAX_VALIDATIONS, stages=False):
    """pc [2B, P, 3] f64 / valid [2B, P] u8 CUDA tensors (cloud 2b = the source of pair b, 2b+1 its target) -> (pose [B,4,4] f64 with
    T p_src ~ p_tgt, status [B] i32, out).  out always holds the per-pair fitness, inlier_rmse, n_iterations, n_validations and
    best_index; stages=True adds down_points, down_count, fpfh, nn (source -> target feature match), val_iter, val_inliers and val_err.
    Raises on an invalid call; a cloud with more than max_points voxels gives its pair status 3 (overflow) and identity."""
    import torch
    _lib.require_gpu()
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.shape[0] % 2 or valid.shape != pc.shape[:2]:
        raise ValueError("pc must be [2B, P, 3] and valid [2B, P]")
    pc = pc.to(torch.float64).contiguous()
    valid = valid.to(torch.uint8).contiguous()
    C2, P = int(pc.shape[0]), int(pc.shape[1])
    B, N, dev = C2 // 2, int(max_points), pc.device
    MI, MV = int(max_iterations), int(max_validations)
    L = _lib.lib()
    wsb = L.relpose_ransac_workspace_bytes(B, P, N, MI, MV)
    if wsb == 0 or MI <= 0 or MV <= 0:
        raise ValueError(f"relpose_ransac: unsupported sizes (pairs {B}, points {P}, max_points {N}, max_iterations {MI}, max_validations {MV})")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    pose = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    out = {"fitness": f64(B), "inlier_rmse": f64(B), "n_iterations": i32(B), "n_validations": i32(B), "best_index": i32(B)}
    if stages:
        out.update(down_points=f64(C2, N, 3), down_count=i32(C2), fpfh=f64(C2, N, 33), nn=torch.full((B, N), -1, dtype=torch.int32, device=dev),
                   val_iter=torch.full((B, MV), -1, dtype=torch.int32, device=dev), val_inliers=i32(B, MV), val_err=f64(B, MV))
    a = _lib.RansacArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_points, a.max_points, a.seed = B, P, N, int(seed)
    a.max_iterations, a.max_validations = MI, MV
    a.pc, a.valid, a.pose, a.status = pc.data_ptr(), valid.data_ptr(), pose.data_ptr(), status.data_ptr()
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), wsb, _lib.stream_ptr()
    rc = L.relpose_ransac(C.byref(a))
    if rc not in (0, _lib.RANSAC_OVERFLOW):
        _lib.check(rc, "relpose_ransac")
    return pose, status, out


def open3d_global_registration(pc_src, pc_tgt):
    """baselines.py:52-81: pc_src [n1,3], pc_tgt [n2,3] numpy -> R_hat [4,4] numpy (T p_src ~ p_tgt; identity when the pair has too
    few points, more voxels than RELPOSE_FGR_MAX_POINTS, or no hypothesis with an inlier)."""
    import torch
    dev = _lib.require_gpu()
    pc, valid = pack_clouds([np.asarray(pc_src, np.float64).reshape(-1, 3), np.asarray(pc_tgt, np.float64).reshape(-1, 3)])
    pose, _, _ = global_registration_dev(torch.from_numpy(pc).to(dev), torch.from_numpy(valid).to(dev))
    return pose[0].cpu().numpy()


def colored_icp_dev(pc, color, valid, init=None, lambda_geometric=_lib.CICP_LAMBDA_GEOMETRIC, max_points=_lib.FGR_MAX_POINTS, stages=False):
    """pc, color [2B, P, 3] f64 / valid [2B, P] u8 CUDA tensors (cloud 2b = the source of pair b, 2b+1 its target), init [B,4,4] f64 or
    None (the identity) -> (pose [B,4,4] f64 with T p_src ~ p_tgt, status [B] i32, out): the three coloured ICP levels of
    baselines.py:141-166 from `init`.  out always holds fitness, inlier_rmse, n_iterations [B,3] and level_pose [B,3,4,4]; stages=True
    adds down_points, down_colors [2B,3,N,3], down_count [2B,3], the target's normals and gradient [B,3,N,3] and the per-iteration
    trace iter_pose [B,94,4,4], iter_ncorr, iter_rmse [B,94], iter_corr [B,94,N] (-1 = no correspondence or not evaluated), iter_x [B,94,6].
    Raises on an invalid call; a cloud with more than max_points voxels at some level gives its pair status 3 (overflow) and identity."""
    import torch
    _lib.require_gpu()
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.shape[0] % 2 or valid.shape != pc.shape[:2] or color.shape != pc.shape:
        raise ValueError("pc and color must be [2B, P, 3] and valid [2B, P]")
    pc = pc.to(torch.float64).contiguous()
    color = color.to(torch.float64).contiguous()
    valid = valid.to(torch.uint8).contiguous()
    C2, P = int(pc.shape[0]), int(pc.shape[1])
    B, N, dev = C2 // 2, int(max_points), pc.device
    if init is not None:
        if tuple(init.shape) != (B, 4, 4):
            raise ValueError("init must be [B, 4, 4]")
        init = init.to(device=dev, dtype=torch.float64).contiguous()
    lam = float(lambda_geometric)
    L = _lib.lib()
    wsb = L.relpose_cicp_workspace_bytes(B, P, N)
    if wsb == 0 or not 0.0 <= lam <= 1.0:
        raise ValueError(f"relpose_cicp: unsupported arguments (pairs {B}, points {P}, max_points {N}, lambda_geometric {lam})")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    pose = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    NL, NS = _lib.CICP_LEVELS, _lib.CICP_TRACE_SLOTS
    out = {"fitness": f64(B, NL), "inlier_rmse": f64(B, NL), "n_iterations": i32(B, NL), "level_pose": f64(B, NL, 4, 4)}
    if stages:
        out.update(down_points=f64(C2, NL, N, 3), down_colors=f64(C2, NL, N, 3), down_count=i32(C2, NL), normals=f64(B, NL, N, 3),
                   gradient=f64(B, NL, N, 3), iter_pose=f64(B, NS, 4, 4), iter_ncorr=i32(B, NS), iter_rmse=f64(B, NS),
                   iter_corr=torch.full((B, NS, N), -1, dtype=torch.int32, device=dev), iter_x=f64(B, NS, 6))
    a = _lib.CicpArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_points, a.max_points, a.lambda_geometric = B, P, N, lam
    a.pc, a.valid, a.color, a.pose, a.status = pc.data_ptr(), valid.data_ptr(), color.data_ptr(), pose.data_ptr(), status.data_ptr()
    a.init = init.data_ptr() if init is not None else None
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), wsb, _lib.stream_ptr()
    rc = L.relpose_cicp(C.byref(a))
    if rc not in (0, _lib.CICP_OVERFLOW):
        _lib.check(rc, "relpose_cicp")
    return pose, status, out


def color_registration_dev(pc, color, valid, seed=0, lambda_geometric=_lib.CICP_LAMBDA_GEOMETRIC, max_points=_lib.FGR_MAX_POINTS,
                           max_iterations=_lib.RANSAC_MAX_ITERATIONS, max_validations=_lib.RANSAC_MAX_VALIDATIONS, stages=False):
    """The whole `cgs` baseline for a batch of pairs: global_registration_dev, then colored_icp_dev from its pose whatever the RANSAC
    status (the reference passes result.transformation on unconditionally, baselines.py:144) -> (pose, status, out).  status is the
    ICP's; out is colored_icp_dev's plus ransac_pose, ransac_status, ransac_fitness and ransac_inlier_rmse."""
    p0, s0, o0 = global_registration_dev(pc, valid, max_points=max_points, seed=seed, max_iterations=max_iterations,
                                         max_validations=max_validations)
    pose, status, out = colored_icp_dev(pc, color, valid, init=p0, lambda_geometric=lambda_geometric, max_points=max_points, stages=stages)
    out.update(ransac_pose=p0, ransac_status=s0, ransac_fitness=o0["fitness"], ransac_inlier_rmse=o0["inlier_rmse"])
    return pose, status, out


def open3d_color_registration(pc_src, pc_tgt, color_src, color_tgt):
    """baselines.py:110-168: pc_src, color_src [n1,3], pc_tgt, color_tgt [n2,3] numpy -> R_hat [4,4] numpy (T p_src ~ p_tgt; identity when
    a cloud has too few points or more voxels than RELPOSE_FGR_MAX_POINTS at some level)."""
    import torch
    dev = _lib.require_gpu()
    f = lambda x: np.asarray(x, np.float64).reshape(-1, 3)
    pc, valid = pack_clouds([f(pc_src), f(pc_tgt)])
    col, _ = pack_clouds([f(color_src), f(color_tgt)])
    pose, _, _ = color_registration_dev(torch.from_numpy(pc).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(valid).to(dev))
    return pose[0].cpu().numpy()
