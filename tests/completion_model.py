"""Numpy statement of the completion-loss contracts (include/relpose.h): relpose_completion_loss and
relpose_contrast_loss.  The fp32 terms are written exactly as the kernels evaluate them (numpy float32 arithmetic rounds every operation,
like the device code built with -ffp-contract=off); the sums are float64.  The order of a float64 sum is NOT part of the model: the
kernels' fixed order and numpy's pairwise order agree to the bounds the tests state.  Also the draw orders of the host side."""
import numpy as np

ROWS = ("rgb", "n", "d", "ce", "w")
ROW_CHANNELS = ((0, 3), (3, 6), (6, 7))


def loss_weight(complete, weight=None):
    """w(i, p) = (complete[i, 6, p] != 0 ? 1 : 0) * weight[i, p] in fp32 -> [N,H,W] float32."""
    w = (complete[:, 6] != 0).astype(np.float32)
    if weight is not None:
        w = w * np.asarray(weight, np.float32).reshape(w.shape)
    return w


def cross_entropy(z, label):
    """z [N,S,H,W] float32 logits, label [N,H,W] -> (ce, lse, z_label, ok) float64 [N,H,W]: m = max_c z_c, lse = m + log(sum_c exp(z_c - m)) in
    float64 with c ascending, CE = lse - z_label; a label >= S has CE 0 and ok False."""
    S = z.shape[1]
    z = z.astype(np.float64)
    m = z.max(1)
    s = np.zeros_like(m)
    for c in range(S):
        s = s + np.exp(z[:, c] - m)
    lse = m + np.log(s)
    ok = label < S
    zl = np.take_along_axis(z, np.minimum(label, S - 1).astype(np.int64)[:, None], 1)[:, 0]
    zl = np.where(ok, zl, 0.0)
    return np.where(ok, lse - zl, 0.0), lse, zl, ok


def completion_loss(f, complete, label, mask, weight=None, S=15):
    """-> dict(sums [N,5,2] f64, ce_mag [N] f64, ce_cross f64, ce_cross_mag f64, n_bad_label [N] i32).  ce_cross_mag is the cross
    analogue of ce_mag: sum_p (sum_i |lse_i| + |z_label_i|)(sum_j w_j), the magnitude the bound on ce_cross is stated against."""
    f, complete = np.asarray(f, np.float32), np.asarray(complete, np.float32)
    N, _, H, W = f.shape
    w = loss_weight(complete, weight)
    obs = np.asarray(mask).reshape(N, H, W) != 0
    sums = np.zeros((N, 5, 2))
    region = lambda t: np.stack([np.where(~obs, t, 0.0).sum((1, 2)), np.where(obs, t, 0.0).sum((1, 2))], -1)
    for r, (c0, c1) in enumerate(ROW_CHANNELS):
        t = np.abs((f[:, c0:c1] - complete[:, c0:c1]) * w[:, None])             # float32: subtract, multiply, abs
        assert t.dtype == np.float32
        sums[:, r] = region(t.astype(np.float64).sum(1))
    sums[:, 4] = region(w.astype(np.float64))
    out = {"sums": sums, "ce_mag": np.zeros(N), "ce_cross": 0.0, "ce_cross_mag": 0.0, "n_bad_label": np.zeros(N, np.int32)}
    if label is not None:
        label = np.asarray(label).reshape(N, H, W)
        ce, lse, zl, ok = cross_entropy(f[:, 7:7 + S], label)
        w64 = w.astype(np.float64)
        sums[:, 3] = region(ce * w64)
        mag = np.where(ok, np.abs(lse) + np.abs(zl), 0.0)
        out["ce_mag"] = (w64 * mag).sum((1, 2))
        out["ce_cross"] = float((ce.sum(0) * w64.sum(0)).sum())
        out["ce_cross_mag"] = float((mag.sum(0) * w64.sum(0)).sum())
        out["n_bad_label"] = (~ok).sum((1, 2)).astype(np.int32)
    return out


def scalars(sums, ce_cross, H, W):
    """The reference's scalars from the sums (completion.completion_scalars restated)."""
    N = sums.shape[0]
    px = float(N * H * W)
    return {"errG_rgb": sums[:, 0].sum() / (3 * px), "errG_n": sums[:, 1].sum() / (3 * px), "errG_d": sums[:, 2].sum() / px,
            "errG_s": 0.1 * ce_cross / (N * px), "ce_diag": sums[:, 3].sum() / px}


def sq_dist(a, b):
    """§4.9's expression: float32, from 0, c ascending, acc = acc + d * d (axis 0 = channels)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(np.broadcast(a[0], b[0]).shape, np.float32)
    for c in range(a.shape[0]):
        d = a[c] - b[c]
        acc = acc + d * d
    return acc


def contrast_loss(f, off, C, idx_src, idx_tgt, pair_valid, neg, margin=0.5):
    """-> (pos_sum [B] f64, neg_sum [B] f64, n_active [B] i32, n_skipped [B] i32)."""
    f = np.asarray(f, np.float32)
    B, h, w = f.shape[0] // 2, f.shape[2], f.shape[3]
    K, M = neg.shape[1], neg.shape[2]
    margin = np.float32(margin)
    pos, ngs = np.zeros(B), np.zeros(B)
    act, skp = np.zeros(B, np.int32), np.zeros(B, np.int32)
    inside = lambda xy: (xy[..., 0] >= 0) & (xy[..., 0] < w) & (xy[..., 1] >= 0) & (xy[..., 1] < h)
    for b in range(B):
        if pair_valid is not None and not pair_valid[b]:
            continue
        fs, ft = f[2 * b, off:off + C], f[2 * b + 1, off:off + C]
        s_ok, t_ok, n_ok = inside(idx_src[b]), inside(idx_tgt[b]), inside(neg[b])
        cl = lambda xy: (np.clip(xy[..., 1], 0, h - 1), np.clip(xy[..., 0], 0, w - 1))
        S = fs[(slice(None),) + cl(idx_src[b])]                     # [C, K]
        T = ft[(slice(None),) + cl(idx_tgt[b])]
        Ng = ft[(slice(None),) + cl(neg[b])]                        # [C, K, M]
        p_ok = s_ok & t_ok
        pos[b] = np.where(p_ok, sq_dist(S, T), np.float32(0)).astype(np.float64).sum()
        d = sq_dist(S[:, :, None], Ng)                               # [K, M] float32
        q_ok = s_ok[:, None] & n_ok
        hinge = np.fmax(margin - d, np.float32(0))
        assert hinge.dtype == np.float32
        ngs[b] = np.where(q_ok, hinge, np.float32(0)).astype(np.float64).sum()
        act[b] = int((q_ok & (d < margin)).sum())
        skp[b] = int((~p_ok).sum() + (~q_ok).sum())
    return pos, ngs, act, skp


def draw_negatives(valid, K, H, W, rng, n_neg=100):
    """mainPanoCompletion2view.py:449-453: ny, then nx, K n_neg nv draws each; flat index j K n_neg + k n_neg + m for the j-th valid pair."""
    valid = np.asarray(valid).reshape(-1) != 0
    nv = int(valid.sum())
    neg = np.zeros((len(valid), K, n_neg, 2), np.int32)
    if nv:
        ny = rng.choice(range(H), K * n_neg * nv)
        nx = rng.choice(range(W), K * n_neg * nv)
        j = 0
        for b in range(len(valid)):
            if valid[b]:
                neg[b, :, :, 0] = nx[j * K * n_neg:(j + 1) * K * n_neg].reshape(K, n_neg)
                neg[b, :, :, 1] = ny[j * K * n_neg:(j + 1) * K * n_neg].reshape(K, n_neg)
                j += 1
    return neg


def contrast_scalars(f, off, C, denseCorres, rng, n_neg=100, margin=0.5):
    """(loss_fl, loss_fl_pos, loss_fl_neg) as completion.contrast_loss defines them, from the model."""
    pv = np.asarray(denseCorres["valid"]).reshape(-1) != 0
    nv, K = int(pv.sum()), denseCorres["idxSrc"].shape[1]
    if nv == 0:
        return 0.0, 0.0, 0.0
    neg = draw_negatives(pv, K, f.shape[2], f.shape[3], rng, n_neg)
    i32 = lambda a: np.asarray(a).astype(np.int32)
    pos, ngs, _, _ = contrast_loss(f, off, C, i32(denseCorres["idxSrc"]), i32(denseCorres["idxTgt"]), pv, neg, margin)
    lp, ln = pos.sum() / (nv * K), ngs.sum() / (nv * K * n_neg)
    return lp + ln, lp, ln
