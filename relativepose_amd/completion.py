"""Completion quality: the losses of the reference's validation pass, learner.step(mode='val') (mainPanoCompletion2view.py:457-602), on the
GPU (csrc/completion.hip).  Forward only: no backward, no optimiser, no trainer.

  completion_loss_dev      relpose_completion_loss: dataMask-weighted L1 on rgb / normal / depth (:553-561) and the cross-entropy of the
                           semantic head (:565-567) in one pass over the network output, as float64 sums per image and region
  completion_scalars       the reference's errG_rgb / errG_n / errG_d / errG_s and their splits from those sums (host)
  contrast_loss_dev        relpose_contrast_loss: the sums behind contrast_loss (:429-455), per pair
  contrast_loss            contrast_loss for a batch: the negatives in the reference's draw order, then (loss_fl, loss_fl_pos, loss_fl_neg)
  perturbed_poses          the loaders' pose perturbation (datasets/SUNCG.py:358-364, :405-410, util.randomRotation, util.py:234-240)
  geometric_weight         the `geow` of mainPanoCompletion2view.apply_mask (:59-75), for --GeometricWeight (off by default there and here)

Not built: util.pnlayer (--pnloss; it raises for any batch larger than 1) and loss_fc (needs the Resnet18_8s teacher).
There is no CPU path: the *_dev functions need the GPU."""
import ctypes as C

import numpy as np

from . import _lib

ROWS = ("rgb", "n", "d", "ce", "w")         # rows of `sums`
MARGIN = 0.5                                # the reference's --D


def completion_loss_dev(f, complete, label, mask, weight=None, S=None, with_cross=True):
    """f [N,Ct,H,W] f32 (the network output, read in place; channels >= 7 + S are never read), complete [N,7,H,W] f32 (rgb, normal,
    depth), label [N,H,W] u8 or None, mask [N,1,H,W] or [N,H,W] f32 (nonzero = observed), weight [N,H,W] f32 or None, S classes
    -> (sums [N,5,2] f64, ce_mag [N] f64, ce_cross [1] f64, n_bad_label [N] i32): rows ROWS, regions (unobserved, observed); the
    contract is include/relpose.h.  ce_cross is 0 without a label or with with_cross=False."""
    import torch
    _lib.require_gpu()
    if f.dim() != 4 or f.dtype != torch.float32 or not f.is_contiguous():
        raise ValueError("f must be a contiguous float32 [N, Ct, H, W]")
    if S is None:
        raise ValueError("S (the number of semantic classes) is required")
    N, Ct, H, W = (int(v) for v in f.shape)
    dev = f.device
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    complete, mask = f32(complete), f32(mask)
    if tuple(complete.shape) != (N, 7, H, W) or mask.numel() != N * H * W:
        raise ValueError("complete must be [N, 7, H, W] and mask [N, 1, H, W]")
    if label is not None:
        label = label.to(device=dev, dtype=torch.uint8).contiguous()
        if label.numel() != N * H * W:
            raise ValueError("label must be [N, H, W]")
    if weight is not None:
        weight = f32(weight)
        if weight.numel() != N * H * W:
            raise ValueError("weight must be [N, H, W]")
    cross = bool(with_cross) and label is not None
    L = _lib.lib()
    nbytes = L.relpose_completion_loss_workspace_bytes(N, H, W, int(cross))
    if nbytes == 0:
        raise ValueError("relpose_completion_loss: unsupported shape (H * W must be a multiple of 4)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sums = torch.empty(N, 5, 2, dtype=torch.float64, device=dev)
    ce_mag = torch.empty(N, dtype=torch.float64, device=dev)
    ce_cross = torch.zeros(1, dtype=torch.float64, device=dev)
    n_bad = torch.empty(N, dtype=torch.int32, device=dev)
    a = _lib.CompletionLossArgs()
    a.struct_size = C.sizeof(a)
    a.n_images, a.H, a.W, a.total_channels, a.n_classes = N, H, W, Ct, int(S)
    a.f, a.complete, a.mask = f.data_ptr(), complete.data_ptr(), mask.data_ptr()
    a.label = label.data_ptr() if label is not None else None
    a.weight = weight.data_ptr() if weight is not None else None
    a.sums, a.ce_mag, a.n_bad_label = sums.data_ptr(), ce_mag.data_ptr(), n_bad.data_ptr()
    a.ce_cross = ce_cross.data_ptr() if cross else None
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    _lib.check(L.relpose_completion_loss(C.byref(a)), "relpose_completion_loss")
    return sums, ce_mag, ce_cross, n_bad


def completion_scalars(sums, ce_cross, H, W):
    """sums [N,5,2], ce_cross [1] (host float64) -> the reference's scalars and the project's splits:
    errG_rgb, errG_n = sum / (N 3 H W), errG_d = sum / (N H W) (the .mean() of :554-560), errG_s = 0.1 ce_cross / (N N H W) (:566 and
    its [N,N,H,W] broadcast); `<name>_obs` / `<name>_unobs` = a region's sum / (N channels H W): per-pixel means whose sum is the
    scalar; ce_diag = sum_i sum_p CE_i(p) w_i(p) / (N H W), the per-image form of the cross-entropy (not x 0.1)."""
    sums = np.asarray(sums, np.float64)
    N = sums.shape[0]
    px = float(N * H * W)
    out = {}
    for r, (name, ch) in enumerate((("errG_rgb", 3), ("errG_n", 3), ("errG_d", 1))):
        out[name] = float(sums[:, r, :].sum() / (px * ch))
        out[name + "_unobs"] = float(sums[:, r, 0].sum() / (px * ch))
        out[name + "_obs"] = float(sums[:, r, 1].sum() / (px * ch))
    out["errG_s"] = float(0.1 * np.asarray(ce_cross, np.float64).reshape(-1)[0] / (N * px))
    out["ce_diag"] = float(sums[:, 3, :].sum() / px)
    out["ce_diag_unobs"] = float(sums[:, 3, 0].sum() / px)
    out["ce_diag_obs"] = float(sums[:, 3, 1].sum() / px)
    return out


def contrast_loss_dev(f, feat_off, C_, idx_src, idx_tgt, pair_valid, neg, margin=MARGIN):
    """f [2B,Ct,h,4h] f32 (image 2b = the source of pair b), descriptor = channels feat_off : feat_off + C_; idx_src, idx_tgt [B,K,2] i32
    (x, y) pixels; pair_valid [B] u8 or None; neg [B,K,M,2] i32 (x, y) pixels of the target map
    -> (pos_sum [B] f64, neg_sum [B] f64, n_active [B] i32, n_skipped [B] i32), the contract of include/relpose.h."""
    import torch
    _lib.require_gpu()
    if f.dim() != 4 or f.shape[0] % 2 or f.shape[3] != 4 * f.shape[2] or f.dtype != torch.float32 or not f.is_contiguous():
        raise ValueError("f must be a contiguous float32 [2B, Ct, h, 4h]")
    B, Ct, h = int(f.shape[0]) // 2, int(f.shape[1]), int(f.shape[2])
    dev = f.device
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    idx_src, idx_tgt, neg = i32(idx_src), i32(idx_tgt), i32(neg)
    if idx_src.dim() != 3 or idx_src.shape[0] != B or idx_src.shape[2] != 2 or idx_tgt.shape != idx_src.shape:
        raise ValueError("idx_src and idx_tgt must be [B, K, 2]")
    K = int(idx_src.shape[1])
    if neg.dim() != 4 or tuple(neg.shape[:2]) != (B, K) or neg.shape[3] != 2:
        raise ValueError("neg must be [B, K, M, 2]")
    M = int(neg.shape[2])
    if pair_valid is not None:
        pair_valid = pair_valid.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(pair_valid.shape) != (B,):
            raise ValueError("pair_valid must be [B]")
    L = _lib.lib()
    nbytes = L.relpose_contrast_loss_workspace_bytes(B, K)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    pos = torch.empty(B, dtype=torch.float64, device=dev)
    ngs = torch.empty(B, dtype=torch.float64, device=dev)
    act = torch.empty(B, dtype=torch.int32, device=dev)
    skp = torch.empty(B, dtype=torch.int32, device=dev)
    a = _lib.ContrastLossArgs()
    a.struct_size = C.sizeof(a)
    a.n_pairs, a.h, a.total_channels, a.feat_off, a.n_channels, a.n_corres, a.n_neg = B, h, Ct, int(feat_off), int(C_), K, M
    a.margin = float(margin)
    a.f, a.idx_src, a.idx_tgt, a.neg = f.data_ptr(), idx_src.data_ptr(), idx_tgt.data_ptr(), neg.data_ptr()
    a.pair_valid = pair_valid.data_ptr() if pair_valid is not None else None
    a.pos_sum, a.neg_sum, a.n_active, a.n_skipped = pos.data_ptr(), ngs.data_ptr(), act.data_ptr(), skp.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.stream = _lib.stream_ptr()
    _lib.check(L.relpose_contrast_loss(C.byref(a)), "relpose_contrast_loss")
    return pos, ngs, act, skp


def draw_negatives(valid, K, H, W, rng, n_neg=100):
    """The negatives of contrast_loss in the reference's draw order (mainPanoCompletion2view.py:449-453): with nv valid pairs,
    ny = rng.choice(range(H), K n_neg nv), then nx = rng.choice(range(W), K n_neg nv); negative m of correspondence k of the j-th VALID
    pair is flat index j K n_neg + k n_neg + m.  -> neg [B,K,n_neg,2] int32 (x, y), zeros for the invalid pairs; no draw when nv == 0."""
    valid = np.asarray(valid).reshape(-1) != 0
    B, nv = len(valid), int(valid.sum())
    neg = np.zeros((B, K, n_neg, 2), np.int32)
    if nv:
        ny = rng.choice(range(H), K * n_neg * nv)
        nx = rng.choice(range(W), K * n_neg * nv)
        neg[valid, :, :, 0] = nx.reshape(nv, K, n_neg)
        neg[valid, :, :, 1] = ny.reshape(nv, K, n_neg)
    return neg


def contrast_loss(f, feat_off, C_, denseCorres, rng, n_neg=100, margin=MARGIN, details=None):
    """mainPanoCompletion2view.py:429-455 for a batch: f [2B,Ct,h,4h] f32 CUDA, denseCorres as descriptor.dense_correspondences returns
    it, rng a np.random.RandomState (draw_negatives' order) -> (loss_fl, loss_fl_pos, loss_fl_neg) as Python floats: loss_fl_pos = the mean
    of d over the nv K correspondences of the valid pairs, loss_fl_neg = the mean hinge over their nv K n_neg negatives, loss_fl their
    sum; zeros when no pair is valid (the reference raises there).  details: a dict that receives valid_pairs, n_active, n_skipped."""
    import torch
    B, h = int(f.shape[0]) // 2, int(f.shape[2])
    K = denseCorres["idxSrc"].shape[1]
    pv = np.asarray(denseCorres["valid"]).reshape(B) != 0
    nv = int(pv.sum())
    if details is not None:
        details.update(valid_pairs=nv, n_active=0, n_skipped=0)
    if nv == 0:
        return 0.0, 0.0, 0.0
    neg = draw_negatives(pv, K, h, 4 * h, rng, n_neg)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))
    pos, ngs, act, skp = contrast_loss_dev(f, feat_off, C_, t(denseCorres["idxSrc"]), t(denseCorres["idxTgt"]),
                                           torch.from_numpy(pv.astype(np.uint8)), torch.from_numpy(neg), margin)
    pos, ngs = pos.cpu().numpy(), ngs.cpu().numpy()
    if details is not None:
        details.update(n_active=int(act.sum().item()), n_skipped=int(skp.sum().item()))
    loss_pos = float(pos.sum() / (nv * K))
    loss_neg = float(ngs.sum() / (nv * K * n_neg))
    return loss_pos + loss_neg, loss_pos, loss_neg


def random_rotation(rng, epsilon):
    """util.randomRotation (util.py:234-240) on a given RandomState: rand(3) for the axis, randn(1) for the angle."""
    axis = rng.rand(3) - 0.5
    axis /= np.linalg.norm(axis)
    dtheta = rng.randn(1) * np.pi * epsilon
    K = np.array([0, -axis[2], axis[1], axis[2], 0, -axis[0], -axis[1], axis[0], 0]).reshape(3, 3)
    return np.eye(3) + np.sin(dtheta) * K + (1 - np.cos(dtheta)) * np.matmul(K, K)


def perturbed_poses(R_rel, rng, epsilon=0.1, sigma_t=0.1):
    """The loaders' perturbed re-projection poses (datasets/SUNCG.py:358-364, :405-410).  R_rel [B,4,4]: the pose that takes source-camera
    coordinates to target-camera coordinates -- evaluate_pairs' R_gt = batch["R"][b, 1] inv(batch["R"][b, 0]), the reference's
    R[1] inv(R[0]).  -> [B,2,4,4]: [b, 0] = the perturbed target-to-source pose (applied to the target view warped into the source
    image, :358-364), [b, 1] = the perturbed source-to-target pose (:405-410) -- the order util.warp_pairs_dev takes for images 2b, 2b + 1.
    Draws per pair, first for target-to-source, then for source-to-target: rand(3) (axis), randn(1) (angle pi epsilon), randn(3)
    (translation sigma_t); R_p[:3,:3] = dR R[:3,:3], R_p[:3,3] += t."""
    R_rel = np.asarray(R_rel, np.float64).reshape(-1, 4, 4)
    out = np.zeros((len(R_rel), 2, 4, 4))
    for b, R in enumerate(R_rel):
        for v, R_this in enumerate((np.linalg.inv(R), R)):
            R_p = R_this.copy()
            dR = random_rotation(rng, epsilon)
            R_p[:3, :3] = np.matmul(dR, R_p[:3, :3])
            R_p[:3, 3] += rng.randn(3) * sigma_t
            out[b, v] = R_p
    return out


def geometric_weight(mask_method, h):
    """The `geow` of mainPanoCompletion2view.apply_mask (:59-75) for one image -> [h, 4h] float32.  'second': exp(-d / (2 0.7^2)) with
    d = the distance in faces to the nearest vertical edge of the observed face, 0 on the face itself; 'kinect': 20 on the observed
    box, 1 elsewhere (the reference defines it at 160 x 640 only; other sizes scale the box as util.apply_mask does)."""
    w = 4 * h
    if mask_method == "second":
        ys, xs = np.meshgrid(range(h), range(w), indexing="ij")
        dist = np.stack((np.abs(xs - h), np.abs(xs - (2 * h)), np.abs(xs - w - h), np.abs(xs - w - (2 * h))), 0)
        dist = dist.min(0) / h
        sigmaGeom = 0.7
        dist = np.exp(-dist / (2 * sigmaGeom ** 2))
        dist[:, h:2 * h] = 0
        return dist.astype(np.float32)
    if mask_method == "kinect":
        from .synth import observed_box
        y0, y1, x0, x1 = observed_box("kinect", h)
        g = np.ones((h, w), np.float32)
        g[y0:y1, x0:x1] = 20
        return g
    raise ValueError(f"unknown mask method {mask_method!r}")
