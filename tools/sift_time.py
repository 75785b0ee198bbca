"""Device-event timing of the batched SIFT detector (relpose_sift_detect) on 64 views at 160x160 (observed faces), 320x320 and 480x640
(kinect frames), gray random-blob textures.  Prints one JSON line per size: ms per call (mean / min over --iters after --warmup),
keypoints per view, and the issue's budgets (<= 1 ms per 64 faces at 160x160, <= 5 ms per 64 frames at 480x640 -- estimates from the
arithmetic, not measurements).  The call includes its own end-of-call synchronisation (the overflow flag).

    python tools/sift_time.py [--views 64] [--iters 20] [--warmup 3] [--sizes 160x160,320x320,480x640]
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sift_time.py --iters 5"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BUDGET_MS = {(160, 160): 1.0, (480, 640): 5.0}


def texture(rs, h, w, n):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.full((h, w), 128.0, np.float32)
    for _ in range(n):
        cx, cy, s, a = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(1.5, 6.0), rs.uniform(-90, 90)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-kp", type=int, default=8192)
    ap.add_argument("--sizes", default="160x160,320x320,480x640")
    args = ap.parse_args()
    import ctypes as C

    import torch
    from relativepose_amd import _lib
    dev = _lib.require_gpu()
    for hw in args.sizes.split(","):
        h, w = (int(v) for v in hw.split("x"))
        rs = np.random.RandomState(h * 7 + w)
        base = [texture(rs, h, w, max(h * w // 400, 16)) for _ in range(8)]
        img = torch.from_numpy(np.stack([base[v % 8] for v in range(args.views)])).to(dev)
        V, K = args.views, args.max_kp
        nb = _lib.lib().relpose_sift_workspace_bytes(V, h, w, K)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        xy = torch.empty(V, K, 2, dtype=torch.float32, device=dev)
        cnt = torch.empty(V, dtype=torch.int32, device=dev)
        a = _lib.SiftArgs(C.sizeof(_lib.SiftArgs), V, img.data_ptr(), h, w, 1, 0, 0, w, h, K, xy.data_ptr(), None, None, None, cnt.data_ptr(),
                          ws.data_ptr(), nb, _lib.stream_ptr().value)
        ms = []
        for i in range(args.warmup + args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = _lib.lib().relpose_sift_detect(C.byref(a))
            e1.record()
            torch.cuda.synchronize()
            _lib.check(rc, "relpose_sift_detect")
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        c = cnt.cpu().numpy()
        print(json.dumps({"size": f"{h}x{w}", "views": V, "ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms)), "iters": args.iters,
                          "kp_per_view_mean": float(c.mean()), "kp_per_view_max": int(c.max()), "workspace_gb": nb / 1e9,
                          "budget_ms": BUDGET_MS.get((h, w))}), flush=True)


if __name__ == "__main__":
    main()
