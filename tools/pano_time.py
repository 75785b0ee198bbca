"""Milliseconds of relpose_frames_to_pano (csrc/panorama.hip) at the sizes a user runs: 64 views (32 pairs) with one 480 x 640 frame each
(ScanNet's case: identity pose, the kinect box, 15 % holes) and with four posed frames each (40 degrees apart, no box), into 160 x 640
panoramas.  The median over --reps of 10 back-to-back whole calls (the workspace clear and the three launches) after a warm-up, timed with
events on the current stream, ALTERNATING with the same expressions written with PyTorch ops on the same GPU (float64 geometry,
scatter_reduce_ amin, index_add_), so both see the same clocks.  For the kernels the bytes they must read -- 4 B of depth in each of the
two splat passes and 3 B of rgb in the second: 11 B per frame pixel -- over the call's time, as a share of the 8 TB/s HBM peak.
--ab-lib PATH alternates the product library with another build of it (tools/build_variant.py) in the same way: the A/B of the LDS
aggregation against plain per-point global atomics was taken like that.  Writes profiles/pano_time.txt (--out to write elsewhere), anew on
every run; what was measured once by other means -- that A/B, the kernel trace, the pose from frames -- is kept in
profiles/pano_measurements.txt.  For
the three launches' own times run --kernel-only (11 calls per size, nothing else, nothing written) under `rocprofv3 --kernel-trace --stats`.

  python tools/pano_time.py [--reps 5] [--ab-lib PATH] [--out PATH]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/pano_time.py --kernel-only"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
H = 160


def alternate(fa, fb, reps, inner=10, inner_b=1):
    """Medians (ms per call) of fa and fb, alternating: every repetition times `inner` back-to-back calls of fa, then `inner_b` of fb,
    after one warm-up call of each."""
    import torch
    fa(), fb()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts, k in ((fa, ta, inner), (fb, tb, inner_b)):
            ev[0].record()
            for _ in range(k):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / k)
    return float(np.median(ta)), float(np.median(tb))


def torch_pano(depth, rgb, scale, pose, dataset, h, box, gate=0.05):
    """The contract of DESIGN.md 4.13 with PyTorch ops (float64 geometry; a float minimum and float64 sums in place of the integer ones)
    -> (rgb [n,3,h,4h], depth [n,h,4h], valid [n,h,4h])."""
    import torch
    from relativepose_amd import synth
    n, F, Hf, Wf = depth.shape
    dev = depth.device
    z = depth.double()
    c = torch.arange(Wf, device=dev, dtype=torch.float64)
    r = torch.arange(Hf, device=dev, dtype=torch.float64)
    X = ((c / Wf - 0.5) * 2)[None, None, None, :] * z / scale[:, :, 0, None, None]
    Y = ((0.5 - r / Hf) * 2)[None, None, :, None] * z / scale[:, :, 1, None, None]
    P = torch.stack((X, Y, -z), -1)
    if pose is not None:
        P = torch.einsum("nfab,nfhwb->nfhwa", pose[:, :, :3, :3], P) + pose[:, :, None, None, :3, 3]
    ok = torch.isfinite(depth) & (depth > 0)
    pix = torch.full((n, F, Hf, Wf), -1, dtype=torch.int64, device=dev)
    d = torch.zeros((n, F, Hf, Wf), dtype=torch.float32, device=dev)
    for slot in range(4):
        q = P @ torch.from_numpy(synth.face_rotation(dataset, slot)).to(dev)          # Rs^T p, row-wise
        az = q[..., 2].abs() + 1e-32
        xn, yn = q[..., 0] / az, q[..., 1] / az
        hit = ok & (q[..., 2] < 0) & (xn.abs() < 1) & (yn.abs() < 1) & (pix < 0)
        cx = torch.round((xn + 1) * 0.5 * h).clamp(0, h - 1).long()
        cy = torch.round((1 - yn) * 0.5 * h).clamp(0, h - 1).long()
        pix = torch.where(hit, cy * 4 * h + slot * h + cx, pix)
        d = torch.where(hit, (-q[..., 2]).float(), d)
    keep = (pix >= 0) & (d < 32768.0)
    if box is not None:
        y0, y1, x0, x1 = box
        py, px = pix // (4 * h), pix % (4 * h)
        keep &= (py >= y0) & (py < y1) & (px >= x0) & (px < x1)
    hw = h * 4 * h
    view = torch.arange(n, device=dev)[:, None, None, None].expand_as(pix)
    idx = (view * hw + pix)[keep]
    dk = d[keep]
    zmin = torch.full((n * hw,), float("inf"), device=dev)
    zmin.scatter_reduce_(0, idx, dk, "amin")
    zm = zmin[idx]
    acc = dk <= zm + zm * gate
    ia, da = idx[acc], dk[acc].double()
    cnt = torch.zeros(n * hw, dtype=torch.float64, device=dev).index_add_(0, ia, torch.ones_like(da))
    sz = torch.zeros(n * hw, dtype=torch.float64, device=dev).index_add_(0, ia, da)
    sc = torch.zeros(n * hw, 3, dtype=torch.float64, device=dev).index_add_(0, ia, rgb[keep][acc].double())
    has = cnt > 0
    c1 = cnt.clamp(min=1)
    dep = torch.where(has, sz / c1, torch.zeros_like(sz)).float().reshape(n, h, 4 * h)
    col = torch.where(has[:, None], torch.floor(sc / c1[:, None] + 0.5) / 255.0, torch.zeros_like(sc)).float()
    return col.reshape(n, hw, 3).permute(0, 2, 1).reshape(n, 3, h, 4 * h).contiguous(), dep, has.reshape(n, h, 4 * h)


def _yaw(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = t
    return T


def inputs(views, F):
    """(depth, rgb, pose or None, box) as numpy: 8 distinct views, repeated."""
    from relativepose_amd import synth
    rep = (views + 7) // 8
    if F == 1:
        parts = [synth.make_full_res_pair(700 + k) for k in range(4)]
        dep = np.concatenate([p[0][0] for p in parts])[:, None]
        col = np.concatenate([np.moveaxis(p[1][0], 1, -1) for p in parts])[:, None]
        return np.concatenate([dep] * rep)[:views], np.concatenate([col] * rep)[:views], None, synth.observed_box("kinect", H)
    rs = np.random.RandomState(710)
    fp = [_yaw(-60.0, [0.05, -0.02, 0.03]), _yaw(-20.0, [0.0, 0.02, 0.0]), _yaw(20.0, [0.0, 0.0, 0.0]), _yaw(60.0, [-0.04, 0.03, 0.02])][:F]
    poses = [synth.random_rigid(rs, np.pi, 0.4) for _ in range(8)]
    dep, col = synth.render_frames(rs, poses, np.array([2.6, 1.9, 3.1]), frame_poses=[fp] * 8, hole_frac=0.15)
    pose = np.stack([np.stack(fp)] * 8)
    return np.concatenate([dep] * rep)[:views], np.concatenate([col] * rep)[:views], np.concatenate([pose] * rep)[:views], None


def caller(L, depth, rgb, scale, pose, box, out, ws):
    """A closure that calls L.relpose_frames_to_pano on fixed buffers (L: the product library or another build of it)."""
    from relativepose_amd import _lib
    L.relpose_frames_to_pano.restype = C.c_int
    L.relpose_frames_to_pano.argtypes = [C.POINTER(_lib.FramesToPanoArgs)]
    n, F, Hf, Wf = depth.shape
    a = _lib.FramesToPanoArgs()
    a.struct_size = C.sizeof(a)
    a.n_views, a.n_frames, a.frame_h, a.frame_w, a.h, a.dataset, a.gate = n, F, Hf, Wf, H, 2, 0.05
    a.box[:] = (-1, -1, -1, -1) if box is None else tuple(box)
    a.depth, a.rgb, a.scale, a.pose = _lib.ptr(depth), _lib.ptr(rgb), _lib.ptr(scale), _lib.ptr(pose)
    a.out_rgb, a.out_depth, a.out_valid = (_lib.ptr(t) for t in out)
    a.workspace, a.workspace_bytes, a.stream = _lib.ptr(ws), ws.numel(), _lib.stream_ptr()

    def call():
        rc = L.relpose_frames_to_pano(C.byref(a))
        assert rc == 0, rc
    return call


def main():
    import torch
    from relativepose_amd import _lib, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--ab-lib", default=None, help="another build of the library to alternate with the product one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pano_time.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="only the library's calls, 11 per size, for a kernel-trace run")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    Lb = C.CDLL(os.path.abspath(args.ab_lib)) if args.ab_lib else None
    lines = [f"# python tools/pano_time.py --reps {args.reps}, 1x MI355X (medians of whole calls: workspace clear + min + accumulate + resolve; "
             f"events on the stream, the two sides alternating; {args.views} views into {H} x {4 * H}, 480 x 640 frames with 15 % holes, gate 0.05)"]
    for F in (1, 4):
        dep, col, pose, box = inputs(args.views, F)
        n = dep.shape[0]
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        depth, rgb, ps = up(dep), up(col), up(pose)
        scale = up(np.array(np.broadcast_to(np.asarray(util.SCANNET_FRAME_SCALE), (n, F, 2))))
        out = (torch.empty(n, 3, H, 4 * H, device=dev), torch.empty(n, H, 4 * H, device=dev), torch.empty(n, H, 4 * H, dtype=torch.uint8, device=dev))
        ws = torch.empty(L.relpose_frames_to_pano_workspace_bytes(n, H), dtype=torch.uint8, device=dev)
        call = caller(L, depth, rgb, scale, ps, box, out, ws)
        if args.kernel_only:
            for _ in range(11):
                call()
            torch.cuda.synchronize()
            continue
        ms, tms = alternate(call, lambda: torch_pano(depth, rgb, scale, ps, "scannet", H, box), args.reps)
        call()
        tr, td, tv = torch_pano(depth, rgb, scale, ps, "scannet", H, box)
        both = (out[2] != 0) & tv
        derr = float(((out[1] - td).abs() / td.clamp(min=1e-6))[both].max())
        nbytes = n * F * 480 * 640 * 11
        lines.append(f"relpose_frames_to_pano, {n} views x {F} frame(s): {ms:.3f} ms per call ({n * F * 480 * 640 / ms / 1e6:.2f} G frame pixels per second); "
                     f"{nbytes / 1e9:.3f} GB to read at least (11 B per frame pixel over the two passes) = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = "
                     f"{100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak; valid panorama pixels {int((out[2] != 0).sum())}; "
                     f"the same expressions with PyTorch ops: {tms:.1f} ms, {tms / ms:.0f} x the kernels; validity differs from PyTorch's at "
                     f"{int(((out[2] != 0) != tv).sum())} pixels, largest relative depth difference {derr:.1e}")
        if Lb is not None:
            out_b = tuple(torch.empty_like(t) for t in out)
            call_b = caller(Lb, depth, rgb, scale, ps, box, out_b, ws)
            ma, mb = alternate(call, call_b, args.reps, 10, 10)
            call(), call_b()
            torch.cuda.synchronize()
            same = all(torch.equal(x, y) for x, y in zip(out, out_b))
            lines.append(f"  A/B, {n} views x {F} frame(s): product library {ma:.3f} ms, {os.path.basename(args.ab_lib)} {mb:.3f} ms per call "
                         f"({mb / ma:.2f} x); outputs bitwise equal: {same}")
        del out, ws
        torch.cuda.empty_cache()
    if args.kernel_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
