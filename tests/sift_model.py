"""Vectorised numpy float32 model of the SIFT detection contract ("SIFT detector"), used only by the tests.

It is written from the contract, step by step, with the float32 operations in the order csrc/sift.hip runs them (the kernels are
compiled without FMA contraction), so the blur, the DoG pyramid, the extremum test and the refinement agree bit for bit.  The
orientation histogram uses exp / atan2, whose last bits may differ between numpy and the device: the tests allow for that (a
secondary orientation can appear or vanish when its peak lies within round-off of 0.8 max)."""
import math

import numpy as np

F = np.float32
SIGMA, LAYERS, CONTRAST, EDGE, BORDER, MAX_STEPS, NBINS = 1.6, 3, 0.02, 10.0, 5, 5, 36


def n_octaves(h, w):
    return int(math.floor(math.log2(min(h, w)) - 2.0 + 0.5)) + 1


def kernel_size(sigma):
    return int(math.floor(sigma * 8.0 + 1.0 + 0.5)) | 1


def gaussian_taps(sigma):
    """float32 taps: computed in double, normalised, rounded to float (index order sum, like the host code)."""
    ks = kernel_size(sigma)
    r = ks // 2
    w = [math.exp(-((i - r) * (i - r)) / (2.0 * sigma * sigma)) for i in range(ks)]
    s = 0.0
    for x in w:
        s += x
    return np.array([x / s for x in w], dtype=F)


def layer_sigmas():
    """[base blur, sigma_1 .. sigma_5]."""
    k = math.pow(2.0, 1.0 / LAYERS)
    return [math.sqrt(max(SIGMA * SIGMA - 1.0, 0.01))] + [SIGMA * math.pow(k, i - 1) * math.sqrt(k * k - 1.0) for i in range(1, LAYERS + 3)]


def bgr2gray(img):
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def refl101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def blur(img, t):
    """img [V, H, W] f32: rows first, then columns; taps summed in index order; reflect-101 border."""
    V, H, W = img.shape
    r = len(t) // 2
    pad = img[:, :, refl101(np.arange(-r, W + r), W)]
    acc = t[0] * pad[:, :, 0:W]
    for j in range(1, 2 * r + 1):
        acc = acc + t[j] * pad[:, :, j:j + W]
    pad = acc[:, refl101(np.arange(-r, H + r), H), :]
    out = t[0] * pad[:, 0:H, :]
    for j in range(1, 2 * r + 1):
        out = out + t[j] * pad[:, j:j + H, :]
    return out


def upsample2(gray):
    """x2 bilinear, half-pixel centres: 3/4 the nearer source pixel, 1/4 the other neighbour, edge clamped."""
    V, h, w = gray.shape
    g = gray.astype(F)
    Y, X = np.arange(2 * h), np.arange(2 * w)
    ny, nx = Y >> 1, X >> 1
    fy = np.where(Y & 1, np.minimum(ny + 1, h - 1), np.maximum(ny - 1, 0))
    fx = np.where(X & 1, np.minimum(nx + 1, w - 1), np.maximum(nx - 1, 0))
    a, b = g[:, ny][:, :, nx], g[:, ny][:, :, fx]
    c, d = g[:, fy][:, :, nx], g[:, fy][:, :, fx]
    return F(0.75) * (F(0.75) * a + F(0.25) * b) + F(0.25) * (F(0.75) * c + F(0.25) * d)


def pyramid(gray):
    """gray uint8 [V, h, w] -> lists over octaves of G [V, 6, H, W] and D [V, 5, H, W]."""
    sig = layer_sigmas()
    taps = [gaussian_taps(s) for s in sig]
    V, h, w = gray.shape
    Gs, Ds = [], []
    for o in range(n_octaves(h, w)):
        if o == 0:
            g0 = blur(upsample2(gray), taps[0])
        else:
            p = Gs[-1][:, 3]
            H, W = p.shape[1] // 2, p.shape[2] // 2
            g0 = np.ascontiguousarray(p[:, 0:2 * H:2, 0:2 * W:2])
        G = [g0]
        for i in range(1, LAYERS + 3):
            G.append(blur(G[-1], taps[i]))
        G = np.stack(G, 1)
        Gs.append(G)
        Ds.append(G[:, 1:] - G[:, :-1])
    return Gs, Ds


def extrema(D):
    """Candidates (v, layer, r, c) of one octave: DoG layers 1..3, 5-px border, |D| > 0, >= / <= all 26 neighbours."""
    V, _, H, W = D.shape
    out = []
    if H - 2 * BORDER <= 0 or W - 2 * BORDER <= 0:
        return [np.zeros(0, np.int64)] * 4
    for l in range(1, LAYERS + 1):
        c = D[:, l, BORDER:H - BORDER, BORDER:W - BORDER]
        pos, neg = c > 0, c < 0
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == 0 and dy == 0 and dx == 0:
                        continue
                    nb = D[:, l + dl, BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]
                    pos &= c >= nb
                    neg &= c <= nb
        v, r, cc = np.nonzero(pos | neg)
        out.append((v, np.full_like(v, l), r + BORDER, cc + BORDER))
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


def refine(D, o, cand):
    """Newton refinement + contrast + edge tests of one octave's candidates -> dict of the kept keypoints."""
    V, _, H, W = D.shape
    v, l, r, c = (np.array(a, dtype=np.int64) for a in cand)
    n = len(v)
    img_scale = F(1) / F(255)
    ds, ss, cs = img_scale * F(0.5), img_scale, img_scale * F(0.25)
    state = np.zeros(n, np.int8)          # 0 running, 1 converged, 2 rejected
    keep = {k: np.zeros(n, F) for k in ("val", "gx", "gy", "gs", "dxx", "dyy", "dxy", "xc", "xr", "xs")}
    for it in range(MAX_STEPS):
        idx = np.nonzero(state == 0)[0]
        if not len(idx):
            break
        vv, ll, rr, cc = v[idx], l[idx], r[idx], c[idx]
        at = lambda dl, dy, dx: D[vv, ll + dl, rr + dy, cc + dx]
        val = at(0, 0, 0)
        gx = (at(0, 0, 1) - at(0, 0, -1)) * ds
        gy = (at(0, 1, 0) - at(0, -1, 0)) * ds
        gs = (at(1, 0, 0) - at(-1, 0, 0)) * ds
        v2 = val * F(2)
        dxx = (at(0, 0, 1) + at(0, 0, -1) - v2) * ss
        dyy = (at(0, 1, 0) + at(0, -1, 0) - v2) * ss
        dss = (at(1, 0, 0) + at(-1, 0, 0) - v2) * ss
        dxy = (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1)) * cs
        dxs = (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1)) * cs
        dys = (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0)) * cs
        a, b, C, d, e, f = dxx, dxy, dxs, dyy, dys, dss
        m0, m1, m2 = d * f - e * e, b * f - e * C, b * e - d * C
        det = a * m0 - b * m1 + C * m2
        n0 = gx * m0 - b * (gy * f - e * gs) + C * (gy * e - d * gs)
        n1 = a * (gy * f - e * gs) - gx * m1 + C * (b * gs - gy * C)
        n2 = a * (d * gs - gy * e) - b * (b * gs - gy * C) + gx * m2
        with np.errstate(divide="ignore", invalid="ignore"):
            xc, xr, xs = -(n0 / det), -(n1 / det), -(n2 / det)
        for k, a_ in (("val", val), ("gx", gx), ("gy", gy), ("gs", gs), ("dxx", dxx), ("dyy", dyy), ("dxy", dxy), ("xc", xc), ("xr", xr), ("xs", xs)):
            keep[k][idx] = a_
        sing = det == 0
        conv = ~sing & (np.abs(xc) < 0.5) & (np.abs(xr) < 0.5) & (np.abs(xs) < 0.5)
        huge = ~sing & ~conv & ~((np.abs(xc) < F(1e6)) & (np.abs(xr) < F(1e6)) & (np.abs(xs) < F(1e6)))
        move = ~sing & ~conv & ~huge
        st = np.where(sing | huge, 2, np.where(conv, 1, 0)).astype(np.int8)
        mi = idx[move]
        with np.errstate(invalid="ignore"):
            c[mi] += np.rint(xc[move]).astype(np.int64)
            r[mi] += np.rint(xr[move]).astype(np.int64)
            l[mi] += np.rint(xs[move]).astype(np.int64)
        out = (l[idx] < 1) | (l[idx] > LAYERS) | (c[idx] < BORDER) | (c[idx] >= W - BORDER) | (r[idx] < BORDER) | (r[idx] >= H - BORDER)
        st = np.where(move & out, 2, st).astype(np.int8)
        state[idx] = st
    K = keep
    ok = state == 1
    # (rejected candidates carry inf / nan offsets: their arithmetic below is discarded by `ok`)
    with np.errstate(over="ignore", invalid="ignore"):
        return _finish(K, ok, v, l, r, c, o, img_scale)


def _finish(K, ok, v, l, r, c, o, img_scale):
    t = K["gx"] * K["xc"] + K["gy"] * K["xr"] + K["gs"] * K["xs"]
    contr = K["val"] * img_scale + t * F(0.5)
    tr = K["dxx"] + K["dyy"]
    det2 = K["dxx"] * K["dyy"] - K["dxy"] * K["dxy"]
    ok &= ~(np.abs(contr) * F(3) < F(CONTRAST)) & (det2 > 0) & ~(tr * tr * F(EDGE) >= F((EDGE + 1) ** 2) * det2)
    so = F(1 << o)
    sc = SIGMA * np.exp2((l.astype(np.float64) + K["xs"].astype(np.float64)) / LAYERS)
    return {"v": v[ok], "o": np.full(int(ok.sum()), o), "l": l[ok], "r": r[ok], "c": c[ok],
            "x": ((c.astype(F) + K["xc"]) * so * F(0.5))[ok], "y": ((r.astype(F) + K["xr"]) * so * F(0.5))[ok],
            "size": (sc * float(1 << o) * 2.0 * 0.5).astype(F)[ok], "scale": sc.astype(F)[ok], "response": np.abs(contr)[ok]}


def orientations(img, r, c, s):
    """Angles (degrees, [0, 360)) of one keypoint from its Gaussian layer img [H, W]: the smoothed 36-bin histogram's peaks >= 0.8 max.
    The pixel -> lane assignment and the summation order follow the kernel (pixel p of the window goes to lane p % 64)."""
    H, W = img.shape
    R = int(np.rint(F(4.5) * s))
    sw = F(1.5) * s
    escale = F(-1) / (F(2) * sw * sw)
    side = 2 * R + 1
    p = np.arange(side * side)
    di, dj = p // side - R, p % side - R
    y, x = r + di, c + dj
    ok = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
    yc, xc = np.clip(y, 1, H - 2), np.clip(x, 1, W - 2)
    dx = img[yc, xc + 1] - img[yc, xc - 1]
    dy = img[yc - 1, xc] - img[yc + 1, xc]
    w = np.exp((di * di + dj * dj).astype(F) * escale)
    mag = np.sqrt(dx * dx + dy * dy)
    ori = np.arctan2(dy, dx) * F(180.0 / math.pi)
    b = np.rint(ori * F(NBINS / 360.0)).astype(np.int64)
    b = np.where(b >= NBINS, b - NBINS, b)
    b = np.where(b < 0, b + NBINS, b)
    contrib = np.where(ok, w * mag, F(0))
    hl = np.zeros((64, NBINS), F)
    for k0 in range(0, len(p), 64):
        sl = slice(k0, min(k0 + 64, len(p)))
        lanes = p[sl] % 64
        hl[lanes, b[sl]] = hl[lanes, b[sl]] + contrib[sl]
    raw = hl[0].copy()
    for q in range(1, 64):
        raw = raw + hl[q]
    i = np.arange(NBINS)
    hs = (raw[(i - 2) % NBINS] + raw[(i + 2) % NBINS]) * F(1 / 16) + (raw[(i - 1) % NBINS] + raw[(i + 1) % NBINS]) * F(4 / 16) + raw * F(6 / 16)
    thr = hs.max() * F(0.8)
    L, Rr = hs[(i - 1) % NBINS], hs[(i + 1) % NBINS]
    peak = (hs > L) & (hs > Rr) & (hs >= thr)
    out = []
    for j in np.nonzero(peak)[0]:
        bn = F(j) + F(0.5) * (L[j] - Rr[j]) / (L[j] - F(2) * hs[j] + Rr[j])
        bn = F(NBINS) + bn if bn < 0 else (bn - F(NBINS) if bn >= NBINS else bn)
        ang = F(360) - F(360.0 / NBINS) * bn
        if abs(ang - F(360)) < np.finfo(F).eps:
            ang = F(0)
        out.append(F(ang))
    return out


def detect(gray):
    """gray uint8 [V, h, w] -> per view dict of float32 arrays x, y, size, angle, response in contract order, duplicates removed."""
    gray = np.asarray(gray, dtype=np.uint8)
    if gray.ndim == 2:
        gray = gray[None]
    Gs, Ds = pyramid(gray)
    V = gray.shape[0]
    rec = [[] for _ in range(V)]
    for o, (G, D) in enumerate(zip(Gs, Ds)):
        k = refine(D, o, extrema(D))
        for i in range(len(k["v"])):
            v = int(k["v"][i])
            for ang in orientations(G[v, k["l"][i]], int(k["r"][i]), int(k["c"][i]), k["scale"][i]):
                rec[v].append((k["x"][i], k["y"][i], k["size"][i], ang, k["response"][i]))
    res = []
    for v in range(V):
        a = np.array(rec[v], dtype=F).reshape(-1, 5)
        order = np.lexsort((-a[:, 4], a[:, 3], -a[:, 2], a[:, 1], a[:, 0]))
        a = a[order]
        if len(a):
            dup = np.zeros(len(a), bool)
            dup[1:] = np.all(a[1:, :4] == a[:-1, :4], axis=1)
            a = a[~dup]
        res.append({"x": a[:, 0], "y": a[:, 1], "size": a[:, 2], "angle": a[:, 3], "response": a[:, 4]})
    return res
