"""Descriptor evaluation: the reference's feature-quality metric on the GPU (csrc/descriptor.hip).

  dense_nn_dev             relpose_dense_nn: batched nearest neighbour with index (the KDTree query of datasets/SUNCG.py:323-332)
  descriptor_rank_dev      relpose_descriptor_rank: per correspondence, the number of target pixels whose descriptor is closer to the
                           source descriptor than the true match (mainPanoCompletion2view.py:401-405)
  dense_correspondences    the loaders' `denseCorres` branch for a batch (datasets/SUNCG.py:315-341)
  evalDLDescriptor         mainPanoCompletion2view.py:383-414 with the classes of :535-542
  sift_rank_dev            relpose_sift_rank (csrc/siftdesc.hip): the same count over 128-byte SIFT descriptors, in integers
  evalSiftDescriptor       mainPanoCompletion2view.py:353-381, the SIFT baseline of the metric (descriptors: rputil.sift_describe_dev)

contrast_loss on these correspondences is completion.py; out of scope: the training scripts.
There is no CPU path: every function needs the GPU."""
import ctypes as C

import numpy as np

from . import _lib, util

MAX_DIST = 0.08             # datasets/SUNCG.py:328


def dense_nn_dev(pc, valid, to_world, query, max_dist=MAX_DIST):
    """pc [2B,3,P] f64 and valid [2B,P] u8 as util.pano2pc_dev returns them (cloud 2b = the source of pair b, 2b+1 its target; P = 4 h h),
    to_world [2B,4,4] f64 (applied to every cloud), query [B,nq] i32 point indices into the source cloud (-1 = unused)
    -> (nn_index [B,nq] i32, nn_dist [B,nq] f64, hit [B,nq] u8, idx_src, idx_tgt [B,nq,2] i32 (x, y) panorama pixels).
    The nearest VALID target point of every query in world coordinates, ties to the lowest index; hit = nn_dist < max_dist.  A slot
    that is unused, whose source point is invalid or whose target cloud has no valid point reads -1, -1, 0 and pixels 0."""
    import torch
    _lib.require_gpu()
    if pc.dim() != 3 or pc.shape[1] != 3 or pc.shape[0] % 2 or tuple(valid.shape) != (pc.shape[0], pc.shape[2]):
        raise ValueError("pc must be [2B, 3, P] and valid [2B, P]")
    C2, P = int(pc.shape[0]), int(pc.shape[2])
    B, h = C2 // 2, int(round((P / 4) ** 0.5))
    if tuple(to_world.shape) != (C2, 4, 4) or query.dim() != 2 or query.shape[0] != B:
        raise ValueError("to_world must be [2B, 4, 4] and query [B, nq]")
    dev = pc.device
    pc = pc.to(torch.float64).contiguous()
    valid = valid.to(torch.uint8).contiguous()
    to_world = to_world.to(device=dev, dtype=torch.float64).contiguous()
    query = query.to(device=dev, dtype=torch.int32).contiguous()
    nq = int(query.shape[1])
    out = (torch.empty(B, nq, dtype=torch.int32, device=dev), torch.empty(B, nq, dtype=torch.float64, device=dev),
           torch.empty(B, nq, dtype=torch.uint8, device=dev), torch.empty(B, nq, 2, dtype=torch.int32, device=dev),
           torch.empty(B, nq, 2, dtype=torch.int32, device=dev))
    a = _lib.DenseNnArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_points, a.n_query, a.h, a.max_dist = B, P, nq, h, float(max_dist)
    a.pc, a.valid, a.to_world, a.query = pc.data_ptr(), valid.data_ptr(), to_world.data_ptr(), query.data_ptr()
    a.nn_index, a.nn_dist, a.hit, a.idx_src, a.idx_tgt = (t.data_ptr() for t in out)
    a.stream = _lib.stream_ptr()
    _lib.check(_lib.lib().relpose_dense_nn(C.byref(a)), "relpose_dense_nn")
    return out


def descriptor_rank_dev(f, feat_off, C_, idx_src, idx_tgt, sel=None, pair_valid=None, mask=None):
    """f [2B,Ct,h,4h] f32 (the network output, read in place: image 2b = the source of pair b), descriptor = channels feat_off : feat_off + C_;
    idx_src, idx_tgt [B,K,2] i32 (x, y) pixels; sel [B,E] i32 indices into K (-1 = unused; None = all K); pair_valid [B] u8 or None;
    mask [2B,1,h,4h] or [2B,h,4h] f32 or None (nonzero = observed) -> (count [B,E] i32, thr [B,E] f32, type [B,E] i32).
    count = the number of target pixels with a squared descriptor distance strictly below the true match's (thr); -1 for unused slots
    and invalid pairs.  type = observed end points of the correspondence (0, 1 or 2), -1 without a mask."""
    import torch
    _lib.require_gpu()
    if f.dim() != 4 or f.shape[0] % 2 or f.shape[3] != 4 * f.shape[2] or f.dtype != torch.float32 or not f.is_contiguous():
        raise ValueError("f must be a contiguous float32 [2B, Ct, h, 4h]")
    B, Ct, h = int(f.shape[0]) // 2, int(f.shape[1]), int(f.shape[2])
    dev = f.device
    if idx_src.dim() != 3 or idx_src.shape[0] != B or idx_src.shape[2] != 2 or idx_tgt.shape != idx_src.shape:
        raise ValueError("idx_src and idx_tgt must be [B, K, 2]")
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    idx_src, idx_tgt = i32(idx_src), i32(idx_tgt)
    K = int(idx_src.shape[1])
    if sel is not None:
        sel = i32(sel)
        if sel.dim() != 2 or sel.shape[0] != B:
            raise ValueError("sel must be [B, E]")
    E = K if sel is None else int(sel.shape[1])
    if pair_valid is not None:
        pair_valid = pair_valid.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(pair_valid.shape) != (B,):
            raise ValueError("pair_valid must be [B]")
    if mask is not None:
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        if mask.numel() != 2 * B * h * 4 * h:
            raise ValueError("mask must be [2B, h, 4h]")
    count = torch.empty(B, E, dtype=torch.int32, device=dev)
    thr = torch.empty(B, E, dtype=torch.float32, device=dev)
    typ = torch.empty(B, E, dtype=torch.int32, device=dev)
    a = _lib.DescRankArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.h, a.total_channels, a.feat_off, a.n_channels, a.n_corres, a.n_slots = B, h, Ct, int(feat_off), int(C_), K, E
    a.f, a.idx_src, a.idx_tgt = f.data_ptr(), idx_src.data_ptr(), idx_tgt.data_ptr()
    a.sel = sel.data_ptr() if sel is not None else None
    a.pair_valid = pair_valid.data_ptr() if pair_valid is not None else None
    a.mask = mask.data_ptr() if mask is not None else None
    a.count, a.thr, a.type = count.data_ptr(), thr.data_ptr(), typ.data_ptr()
    a.stream = _lib.stream_ptr()
    _lib.check(_lib.lib().relpose_descriptor_rank(C.byref(a)), "relpose_descriptor_rank")
    return count, thr, typ


def dense_correspondences(depth, to_world, dataset, rng, n_query=5000, n_keep=2000, min_corres=500, max_dist=MAX_DIST):
    """The loaders' dense ground-truth correspondences (datasets/SUNCG.py:315-341) for a batch: depth [2B,h,4h] f32 CUDA (image 2b = the
    source of pair b), to_world [2B,4,4] (the transform applied to each panorama's cloud: the reference passes inv(R) of its
    world-to-camera poses; synth.make_pairs' R is camera-to-world and is passed as is), rng a np.random.RandomState
    -> {'idxSrc', 'idxTgt': [B,n_keep,2] float64 (x, y) pixels, 'valid': [B] int64} (host numpy, the reference's key names).
    Draw order: per pair in order rng.choice(range(4 h h), n_query); then ONE nearest-neighbour call for the batch; then per pair in
    order, if it has at least min_corres hits, rng.choice(range(hits), n_keep) over its hits in query order (a pair with fewer makes no
    draw and returns zeros and valid 0).  For B = 1 that is the reference's order; for B > 1 all first draws precede all second draws."""
    import torch
    n2, h, _ = depth.shape
    B, P = n2 // 2, 4 * h * h
    pc, valid = util.pano2pc_dev(depth, dataset)
    query = np.stack([rng.choice(range(P), n_query) for _ in range(B)]).astype(np.int32)
    tw = torch.as_tensor(np.ascontiguousarray(to_world), dtype=torch.float64) if not torch.is_tensor(to_world) else to_world
    _, _, hit, isrc, itgt = dense_nn_dev(pc, valid, tw.to(depth.device), torch.from_numpy(query).to(depth.device), max_dist)
    hit, isrc, itgt = hit.cpu().numpy().astype(bool), isrc.cpu().numpy(), itgt.cpu().numpy()
    out = {"idxSrc": np.zeros((B, n_keep, 2)), "idxTgt": np.zeros((B, n_keep, 2)), "valid": np.zeros(B, np.int64)}
    for b in range(B):
        n = int(hit[b].sum())
        if n < min_corres:
            continue
        pick = rng.choice(range(n), n_keep)
        out["idxSrc"][b] = isrc[b][hit[b]][pick]
        out["idxTgt"][b] = itgt[b][hit[b]][pick]
        out["valid"][b] = 1
    return out


def evalDLDescriptor(f, feat_off, C_, denseCorres, mask, rng, n_eval=100):
    """mainPanoCompletion2view.py:383-414 for a batch: f [2B,Ct,h,4h] f32 CUDA, denseCorres as dense_correspondences returns it, mask
    [2B,1,h,4h] f32 (nonzero = observed), rng a np.random.RandomState -> (ratiosObs, ratiosUnobs): per valid pair in order,
    rng.choice(range(K), n_eval) correspondences (n_eval=None: all K, no draw); ratio = count.astype(float32) / (4 h h); the float32 mean
    over the correspondences with both end points observed is appended to the first list and the mean over the others to the second,
    each only when its class is non-empty."""
    import torch
    B, h = int(f.shape[0]) // 2, int(f.shape[2])
    K = denseCorres["idxSrc"].shape[1]
    pv = np.asarray(denseCorres["valid"]).reshape(B) != 0
    E = K if n_eval is None else int(n_eval)
    sel = None
    if n_eval is not None:
        sel = np.full((B, E), -1, np.int32)
        for b in range(B):
            if pv[b]:
                sel[b] = rng.choice(range(K), E)
        sel = torch.from_numpy(sel)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))
    count, _, typ = descriptor_rank_dev(f, feat_off, C_, t(denseCorres["idxSrc"]), t(denseCorres["idxTgt"]), sel,
                                        torch.from_numpy(pv.astype(np.uint8)), mask)
    count, typ = count.cpu().numpy(), typ.cpu().numpy()
    ratiosObs, ratiosUnobs = [], []
    for b in range(B):
        if not pv[b]:
            continue
        ratio = count[b].astype(np.float32) / np.float32(4 * h * h)
        if (typ[b] == 2).sum() > 0:
            ratiosObs.append(ratio[typ[b] == 2].mean())
        if (typ[b] < 2).sum() > 0:
            ratiosUnobs.append(ratio[typ[b] < 2].mean())
    return ratiosObs, ratiosUnobs


def sift_rank_dev(src, tgt, dense, pair_valid=None):
    """src, tgt [B,E,128] u8 (the SIFT descriptors of E correspondences in the source and the target), dense [B,P,128] u8 (the target's grid
    descriptors), pair_valid [B] u8 or None -> (count [B,E] i32, thr [B,E] i32): thr = sum (src - tgt)^2 and count = the number of grid
    descriptors with sum (src - dense)^2 strictly below it (mainPanoCompletion2view.py:373, :378-379), exact; -1 for invalid pairs."""
    import torch
    dev = _lib.require_gpu()
    u8 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.uint8).contiguous()
    src, tgt, dense = u8(src), u8(tgt), u8(dense)
    if src.dim() != 3 or src.shape[2] != 128 or src.shape[1] < 1 or tgt.shape != src.shape:
        raise ValueError("src and tgt must be [B, E, 128] with E >= 1")
    if dense.dim() != 3 or dense.shape[0] != src.shape[0] or dense.shape[2] != 128 or dense.shape[1] < 1:
        raise ValueError("dense must be [B, P, 128] with P >= 1")
    B, E, P = int(src.shape[0]), int(src.shape[1]), int(dense.shape[1])
    if pair_valid is not None:
        pair_valid = u8(pair_valid)
        if tuple(pair_valid.shape) != (B,):
            raise ValueError("pair_valid must be [B]")
    count = torch.empty(B, E, dtype=torch.int32, device=dev)
    thr = torch.empty(B, E, dtype=torch.int32, device=dev)
    a = _lib.SiftRankArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.n_slots, a.n_points = B, E, P
    a.src, a.tgt, a.dense = src.data_ptr(), tgt.data_ptr(), dense.data_ptr()
    a.pair_valid = pair_valid.data_ptr() if pair_valid is not None else None
    a.thr, a.count = thr.data_ptr(), count.data_ptr()
    a.stream = _lib.stream_ptr()
    _lib.check(_lib.lib().relpose_sift_rank(C.byref(a)), "relpose_sift_rank")
    return count, thr


def evalSiftDescriptor(rgb, denseCorres, rng, n_eval=100, step_size=5):
    """mainPanoCompletion2view.py:353-381 for a batch: rgb [B,2,3,h,4h] float (numpy or torch; channel 0 is weighted as cv2's B, like the
    reference's cvtColor call on it), denseCorres as dense_correspondences returns it, rng a np.random.RandomState -> ratios: per valid
    pair in order, rng.choice(range(K), n_eval) correspondences; SIFT descriptors (size step_size, angle -1) at their source pixels in
    the source panorama, at their target pixels in the target panorama and on the target's grid range(0, 4h, step_size) x
    range(0, h, step_size) -- ONE describe call for the batch -- then ONE rank call; ratio = count / P in float64 and its mean over the
    n_eval correspondences is appended.  The images are rputil.sift_images(rgb, 'second'): trunc(clip(rgb * 255, 0, 255)); the reference's
    unclipped astype('uint8') differs only for values outside [0, 1]."""
    import torch
    from . import rputil
    u8, _ = rputil.sift_images(rgb, "second")            # [2B, h, 4h, 3]; the metric describes the whole panorama: no crop
    dev = u8.device
    B, h, w = int(u8.shape[0]) // 2, int(u8.shape[1]), int(u8.shape[2])
    K = denseCorres["idxSrc"].shape[1]
    pv = np.asarray(denseCorres["valid"]).reshape(B) != 0
    E = int(n_eval)
    grid = rputil.sift_grid_keypoints(w, h, step_size)
    P = len(grid)
    kp = np.zeros((2 * B, E + P, 4), np.float32)
    kp[:, :, 2], kp[:, :, 3] = step_size, -1
    kp[1::2, E:] = grid
    cnt = np.zeros(2 * B, np.int32)
    for b in range(B):
        if not pv[b]:
            continue
        idx = rng.choice(range(K), E)
        kp[2 * b, :E, :2] = np.asarray(denseCorres["idxSrc"][b])[idx]
        kp[2 * b + 1, :E, :2] = np.asarray(denseCorres["idxTgt"][b])[idx]
        cnt[2 * b], cnt[2 * b + 1] = E, E + P
    desc = rputil.sift_describe_dev(u8, None, torch.from_numpy(kp).to(dev), torch.from_numpy(cnt).to(dev))["desc"]
    count, _ = sift_rank_dev(desc[0::2, :E], desc[1::2, :E], desc[1::2, E:], torch.from_numpy(pv.astype(np.uint8)))
    count = count.cpu().numpy()
    return [(count[b].astype(np.float64) / P).mean() for b in range(B) if pv[b]]
