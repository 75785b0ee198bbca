"""Numpy restatement of the descriptor-evaluation contract (csrc/descriptor.hip, relativepose_amd/descriptor.py).
Not a test file: test_descriptor_cpu.py checks it against scipy / float64 / the reference's torch expression, test_gpu_descriptor.py
checks the kernels against it bit for bit.

  to_world             w_a = ((M_a0 x + M_a1 y) + M_a2 z) + M_a3
  dense_nn             per query the valid target point with the smallest d2 = (dx dx + dy dy) + dz dz, ties to the lowest index
  pano_idx             the reference's PanoIdx (datasets/SUNCG.py:164-174)
  dense_correspondences   the selection with its draw order (datasets/SUNCG.py:315-341)
  descriptor_rank      sequential fp32 thresholds, counts and types (mainPanoCompletion2view.py:401-405, :535-542)
  eval_dl_descriptor   the ratio lists (mainPanoCompletion2view.py:383-414)"""
import numpy as np

MAX_DIST = 0.08


def to_world(pc, M):
    """pc [3,n], M [4,4] -> [3,n] in the kernel's operation order."""
    x, y, z = pc
    return np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)])


def pano_idx(index, h):
    """Face-major point index -> [n,2] (x, y) panorama pixels."""
    index = np.asarray(index, np.int64)
    face, rest = index // (h * h), index % (h * h)
    ys, xs = np.divmod(rest, h)
    return np.stack([xs + face * h, ys], -1)


def nearest(wq, wt, valid_t, chunk=256):
    """wq [3,n] queries, wt [3,P] targets (world), valid_t [P] bool -> (index [n] (-1: no target with d2 < inf), d2 [n])."""
    n = wq.shape[1]
    idx, best = np.full(n, -1, np.int64), np.full(n, np.inf)
    for q0 in range(0, n, chunk):
        q = wq[:, q0:q0 + chunk]
        dx, dy, dz = (wt[a][None, :] - q[a][:, None] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(valid_t[None, :] & (d2 == d2), d2, np.inf)       # an invalid point or a NaN distance never wins
        i = np.argmin(d2, 1)                                           # the first minimum = the lowest index
        m = d2[np.arange(len(i)), i]
        idx[q0:q0 + chunk] = np.where(m < np.inf, i, -1)
        best[q0:q0 + chunk] = m
    return idx, best


def dense_nn(pc, valid, M, query, max_dist=MAX_DIST):
    """pc [2B,3,P] f64, valid [2B,P], M [2B,4,4], query [B,nq] -> dict of nn_index, nn_dist, hit, idx_src, idx_tgt (the kernel's outputs)."""
    C2, _, P = pc.shape
    B, nq = query.shape
    h = int(round((P / 4) ** 0.5))
    assert 4 * h * h == P
    valid = np.asarray(valid) != 0
    out = {"nn_index": np.full((B, nq), -1, np.int32), "nn_dist": np.full((B, nq), -1.0), "hit": np.zeros((B, nq), np.uint8),
           "idx_src": np.zeros((B, nq, 2), np.int32), "idx_tgt": np.zeros((B, nq, 2), np.int32)}
    for b in range(B):
        q = query[b]
        used = (q >= 0) & (q < P)
        used[used] = valid[2 * b][q[used]]
        if not used.any():
            continue
        ws = to_world(pc[2 * b][:, q[used]], M[2 * b])
        wt = to_world(pc[2 * b + 1], M[2 * b + 1])
        i, d2 = nearest(ws, wt, valid[2 * b + 1])
        found = i >= 0
        slots = np.where(used)[0][found]
        dist = np.sqrt(d2[found])
        out["nn_index"][b, slots] = i[found]
        out["nn_dist"][b, slots] = dist
        out["hit"][b, slots] = dist < max_dist
        out["idx_src"][b, slots] = pano_idx(q[slots], h)
        out["idx_tgt"][b, slots] = pano_idx(i[found], h)
    return out


def dense_correspondences(pc, valid, M, rng, n_query=5000, n_keep=2000, min_corres=500, max_dist=MAX_DIST):
    """descriptor.dense_correspondences from the clouds: all first draws (per pair in order), the search, then per pair in order the second
    draw over the hits in query order -- only for pairs with at least min_corres hits."""
    C2, _, P = pc.shape
    B = C2 // 2
    query = np.stack([rng.choice(range(P), n_query) for _ in range(B)]).astype(np.int32)
    r = dense_nn(pc, valid, M, query, max_dist)
    out = {"idxSrc": np.zeros((B, n_keep, 2)), "idxTgt": np.zeros((B, n_keep, 2)), "valid": np.zeros(B, np.int64), "hits": np.zeros(B, np.int64)}
    for b in range(B):
        hit = r["hit"][b] != 0
        out["hits"][b] = hit.sum()
        if hit.sum() < min_corres:
            continue
        pick = rng.choice(range(int(hit.sum())), n_keep)
        out["idxSrc"][b] = r["idx_src"][b][hit][pick]
        out["idxTgt"][b] = r["idx_tgt"][b][hit][pick]
        out["valid"][b] = 1
    return out


def sq_dist(a, b):
    """sum_c (a_c - b_c)^2 in fp32 from 0 with c ascending, acc = acc + d * d: a [C, ...], b [C, ...] broadcastable float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(np.broadcast(a[0], b[0]).shape, np.float32)
    for c in range(a.shape[0]):
        d = a[c] - b[c]
        acc = acc + d * d
    return acc


def descriptor_rank(f, feat_off, C, idx_src, idx_tgt, sel=None, pair_valid=None, mask=None):
    """f [2B,Ct,h,4h] f32; idx_* [B,K,2] (x, y); sel [B,E] or None; pair_valid [B] or None; mask [2B,h,4h] (or [2B,1,h,4h]) or None
    -> (count [B,E] i32, thr [B,E] f32, type [B,E] i32)."""
    f = np.asarray(f, np.float32)
    B, h = f.shape[0] // 2, f.shape[2]
    w = 4 * h
    K = idx_src.shape[1]
    if sel is None:
        sel = np.tile(np.arange(K), (B, 1))
    E = sel.shape[1]
    if mask is not None:
        mask = np.asarray(mask).reshape(2 * B, h, w)
    count, thr, typ = np.full((B, E), -1, np.int32), np.zeros((B, E), np.float32), np.full((B, E), -1, np.int32)
    for b in range(B):
        if pair_valid is not None and not pair_valid[b]:
            continue
        fs, ft = f[2 * b, feat_off:feat_off + C], f[2 * b + 1, feat_off:feat_off + C]
        flat = ft.reshape(C, -1)
        for e in range(E):
            k = sel[b, e]
            if k < 0 or k >= K:
                continue
            (xs, ys), (xt, yt) = (int(v) for v in idx_src[b, k]), (int(v) for v in idx_tgt[b, k])
            if not (0 <= xs < w and 0 <= ys < h and 0 <= xt < w and 0 <= yt < h):
                continue
            q = fs[:, ys, xs]
            t = sq_dist(q, ft[:, yt, xt])
            d = sq_dist(q[:, None], flat)
            count[b, e] = (d < t).sum()
            thr[b, e] = t
            if mask is not None:
                typ[b, e] = int(mask[2 * b, ys, xs] != 0) + int(mask[2 * b + 1, yt, xt] != 0)
    return count, thr, typ


def eval_dl_descriptor(f, feat_off, C, corres, mask, rng, n_eval=100):
    """descriptor.evalDLDescriptor: per valid pair in order rng.choice(range(K), n_eval) (n_eval None: all, no draw) -> (ratiosObs, ratiosUnobs)."""
    B, h = f.shape[0] // 2, f.shape[2]
    K = corres["idxSrc"].shape[1]
    pv = np.asarray(corres["valid"]).reshape(B) != 0
    sel = None
    if n_eval is not None:
        sel = np.full((B, n_eval), -1, np.int64)
        for b in range(B):
            if pv[b]:
                sel[b] = rng.choice(range(K), n_eval)
    count, _, typ = descriptor_rank(f, feat_off, C, corres["idxSrc"].astype(np.int32), corres["idxTgt"].astype(np.int32), sel, pv, mask)
    obs, unobs = [], []
    for b in range(B):
        if not pv[b]:
            continue
        ratio = count[b].astype(np.float32) / np.float32(4 * h * h)
        if (typ[b] == 2).sum() > 0:
            obs.append(ratio[typ[b] == 2].mean())
        if (typ[b] < 2).sum() > 0:
            unobs.append(ratio[typ[b] < 2].mean())
    return obs, unobs
