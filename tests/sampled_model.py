"""numpy model of SCNet's sampled tail (RELPOSE_FWD_SAMPLED_OUTPUTS; csrc/sample_pixels.h, heads_sampled_kernel in csrc/scnet.hip):
which elements of the network output relpose_sample_primitives reads for a keypoint -- the elements the sampled tail writes -- and which
pixels of the 224 x 224 head maps each of them is blended from.  tests/test_sampled_outputs_cpu.py checks it against the oracle's
sampling, tests/test_gpu_sampled_outputs.py compares the kernel's output with the dense path on exactly this set."""
import numpy as np

RS = 224


def sample_pixels(pts, h):
    """csrc/sample_pixels.h: pts [..., 2] float64 pixel coordinates -> (tx, ty, xi, yi) int64 arrays: normal / depth are read at the block
    (ty .. ty + 1, tx .. tx + 1), the 32 features at (yi .. yi + 1, xi .. xi + 1)."""
    pts = np.asarray(pts, np.float64)
    W = 4 * h
    px, py = pts[..., 0], pts[..., 1]
    tx, ty = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    ptx, pty = (px / W).astype(np.float32), (py / h).astype(np.float32)
    x, y = ptx * np.float32(W - 1), pty * np.float32(h - 1)
    return tx, ty, np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)


def lin_coef(dst, scale, n_in):
    """lin_coef of csrc/scnet.hip (bilinear, align_corners=False) for integer destination indices `dst`: (i0, i1, l0, l1), float32 weights.
    The kernels contract scale * (dst + 0.5) - 0.5 into one fused multiply-add: the exact product, rounded once."""
    dst = np.asarray(dst)
    src = (np.float64(np.float32(scale)) * (dst.astype(np.float32) + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def source_taps(oy, ox, H, W):
    """The four pixels of the 224 x 224 maps that output pixel (oy, ox) of the H x W map is blended from, and their weights:
    ((y0, y1, ly0, ly1), (x0, x1, lx0, lx1)); value = ly0 * (lx0 * v[y0, x0] + lx1 * v[y0, x1]) + ly1 * (lx0 * v[y1, x0] + lx1 * v[y1, x1])."""
    return lin_coef(oy, np.float32(RS) / np.float32(H), RS), lin_coef(ox, np.float32(RS) / np.float32(W), RS)


def read_mask(pts, npts, h, S):
    """bool [n, 7 + S + 32, h, 4h]: the elements of the network output that the sampler loads for pts [n, N, 2] / npts [n] -- channels 3:7
    at the (ty, tx) blocks and the feature channels at the (yi, xi) blocks of the keypoints k < npts[img]; entries beyond are never read."""
    pts = np.asarray(pts, np.float64)
    n = pts.shape[0]
    m = np.zeros((n, 7 + S + 32, h, 4 * h), bool)
    for i in range(n):
        k = int(npts[i])
        if k == 0:
            continue
        tx, ty, xi, yi = sample_pixels(pts[i, :k], h)
        for dy in (0, 1):
            for dx in (0, 1):
                m[i, 3:7, ty + dy, tx + dx] = True
                m[i][7 + S:, yi + dy, xi + dx] = True
    return m


def resize_out(v, H, W):
    """resize_out_kernel on one [224, 224] map in the blend's order (float32, the products and sums rounded one by one: the kernel's fused
    multiply-adds differ from this in the last bits only)."""
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = source_taps(np.arange(H), np.arange(W), H, W)
    v = v.astype(np.float32)
    top = lx0[None] * v[y0][:, x0] + lx1[None] * v[y0][:, x1]
    bot = lx0[None] * v[y1][:, x0] + lx1[None] * v[y1][:, x1]
    return ly0[:, None] * top + ly1[:, None] * bot
