"""Numpy model of the SIFT descriptor contract, used only by the tests.

The base image runs in float32 through sift_model.blur (csrc/siftdesc.hip must agree with it bit for bit).  The discrete geometry -- the
rounded position, the angle 360 - angle and the radius -- is computed in float32 as the contract states it, so that the model and the
kernel take the same integers; everything after it (rotation, gradients, weights, histogram, normalisation) runs in float64."""
import math

import numpy as np

import sift_model as S

F = np.float32
SIGMA = math.sqrt(1.6 * 1.6 - 0.5 * 0.5)
FLT_EPSILON = float(np.finfo(np.float32).eps)


def gray_of(img):
    """uint8 [h, w, 3] (BGR) or [h, w] -> uint8 gray."""
    img = np.asarray(img)
    return S.bgr2gray(img) if img.ndim == 3 else img


def base_image(gray):
    """gray uint8 [V, h, w] -> float32 [V, h, w]: the 13-tap blur of §4.10 step 1."""
    taps = S.gaussian_taps(SIGMA)
    assert len(taps) == 13
    return S.blur(gray.astype(F), taps)


def grid_keypoints(w, h, step):
    """§4.10 step 7: x in range(0, w, step), y in range(0, h, step), y-major, size = step, angle = -1 -> [n, 4] float32."""
    return np.array([(x, y, step, -1) for y in range(0, h, step) for x in range(0, w, step)], dtype=F).reshape(-1, 4)


def geometry(kp, h, w):
    """(ptx, pty, a, hw, radius) of one keypoint, float32 arithmetic as the contract states it; None for an unused slot."""
    x, y, size, angle = (F(v) for v in kp)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(size) and np.isfinite(angle)) or not size > 0:
        return None
    ptx, pty = int(np.rint(x)), int(np.rint(y))
    a = F(360) - angle
    if a >= F(360):
        a = a - F(360)
    hw = F(3) * (size * F(0.5))
    radius = int(min(np.rint(((hw * F(1.4142135623730951)) * F(5)) * F(0.5)), F(int(math.sqrt(w * w + h * h)))))
    return ptx, pty, a, hw, radius


def histogram(base, kp, want_samples=False):
    """base float32 [h, w], kp (x, y, size, angle) -> h [4, 4, 8] float64 (before normalisation); None for an unused slot."""
    h, w = base.shape
    g = geometry(kp, h, w)
    if g is None:
        return None
    ptx, pty, a, hw, radius = g
    a, hw = float(a), float(hw)
    cos_t, sin_t = math.cos(a * math.pi / 180.0) / hw, math.sin(a * math.pi / 180.0) / hw
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    c_rot, r_rot = jj * cos_t - ii * sin_t, jj * sin_t + ii * cos_t
    rbin, cbin = r_rot + 1.5, c_rot + 1.5
    r, c = pty + ii, ptx + jj
    use = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    r, c, rbin, cbin, c_rot, r_rot = r[use], c[use], rbin[use], cbin[use], c_rot[use], r_rot[use]
    I = base.astype(np.float64)
    dx, dy = I[r, c + 1] - I[r, c - 1], I[r - 1, c] - I[r + 1, c]
    mag = np.sqrt(dx * dx + dy * dy) * np.exp(-(c_rot * c_rot + r_rot * r_rot) / 8.0)
    ori = np.degrees(np.arctan2(dy, dx))
    ori = np.where(ori < 0, ori + 360.0, ori)
    ori = np.where(ori >= 360.0, ori - 360.0, ori)
    obin = (ori - a) * (8.0 / 360.0)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(int), c0.astype(int), o0.astype(int)
    hist = np.zeros((6, 6, 8))                       # spatial bins -1 .. 4; the outer ring is discarded
    for dr, wr in ((0, 1 - fr), (1, fr)):
        for dc, wc in ((0, 1 - fc), (1, fc)):
            for do, wo in ((0, 1 - fo), (1, fo)):
                np.add.at(hist, (r0 + dr + 1, c0 + dc + 1, (o0 + do) % 8), mag * wr * wc * wo)
    out = hist[1:5, 1:5]
    if want_samples:
        return out, dict(r=r, c=c, n=int(use.sum()), radius=radius)
    return out


def normalise(hist):
    """h [128] float64 -> (u float64 [128], desc uint8 [128]), §4.10 step 5."""
    hv = hist.reshape(128)
    n = math.sqrt(float((hv * hv).sum()))
    v = np.minimum(hv, 0.2 * n)
    u = v * (512.0 / max(math.sqrt(float((v * v).sum())), FLT_EPSILON))
    return u, np.clip(np.rint(u), 0, 255).astype(np.uint8)


def describe(images, kp, count=None, crop=None):
    """images uint8 [V, ih, iw, 3] or [V, ih, iw]; kp [V, n_kp, 4]; count [V] or None; crop (x0, y0, w, h) or None
    -> (u float64 [V, n_kp, 128], desc uint8 [V, n_kp, 128], base float32 [V, h, w])."""
    images = np.asarray(images)
    gray = np.stack([gray_of(im) for im in images])
    if crop is not None:
        x0, y0, cw, ch = crop
        gray = gray[:, y0:y0 + ch, x0:x0 + cw]
    base = base_image(gray)
    kp = np.asarray(kp, dtype=F)
    V, n_kp = kp.shape[:2]
    u, desc = np.zeros((V, n_kp, 128)), np.zeros((V, n_kp, 128), np.uint8)
    for v in range(V):
        for k in range(n_kp if count is None else min(int(count[v]), n_kp)):
            hist = histogram(base[v], kp[v, k])
            if hist is not None:
                u[v, k], desc[v, k] = normalise(hist)
    return u, desc, base


def rank_int(src, tgt, dense, pair_valid=None):
    """The exact counts of relpose_sift_rank in int64: src, tgt [B, E, 128], dense [B, P, 128] uint8 -> (count, thr) [B, E] int64."""
    s, t, d = (np.asarray(x).astype(np.int64) for x in (src, tgt, dense))
    thr = ((s - t) ** 2).sum(2)
    dist = (s * s).sum(2)[:, :, None] + (d * d).sum(2)[:, None, :] - 2 * np.einsum("bek,bpk->bep", s, d)
    count = (dist < thr[:, :, None]).sum(2)
    if pair_valid is not None:
        bad = np.asarray(pair_valid) == 0
        thr[bad], count[bad] = -1, -1
    return count, thr


def rank_f32(src, tgt, dense):
    """The reference's float32 expression (mainPanoCompletion2view.py:373, :378-379; cv2 descriptors are float32) for one pair:
    src, tgt [E, 128], dense [P, 128] -> (count [E], dist [E] float32)."""
    sifts, siftt, dense_feat = (np.asarray(x).astype(np.float32) for x in (src, tgt, dense))
    dist = np.power(sifts - siftt, 2).sum(1)
    distRest = np.power(np.expand_dims(sifts, 1) - np.expand_dims(dense_feat, 0), 2).sum(2)
    return (distRest < dist[:, np.newaxis]).sum(1), dist
