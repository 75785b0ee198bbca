"""Milliseconds of the overlap statistics (csrc/overlap.hip, relpose_overlap) on the four workloads a user runs, each ALTERNATING on the
same GPU with the path it replaces in the evaluation drivers: the per-pair loop over util.point_cloud_overlap (two brute-force
nn_dist_kernel launches and two host reads per pair), which is unchanged and is what the parent commit's drivers ran.

  pairs     32 synth.make_pairs SUNCG pairs at 160 x 640 (25 600 points per cloud; two unrelated poses per room: almost none overlap)
  scenes    32 SceneBatch pairs (mined from multi-view scenes: they do overlap)
  frames    4 full-frame pairs (synth.make_full_res_pair: 307 200 points per cloud, a small motion apart)
  matrix    the 32 x 32 overlap matrix of one 32-view scene (992 directed queries, util.overlap_matrix_dev) against the loop over its 496 pairs

Both sides start from the clouds where their driver has them (the new call on the device, the loop on the host) and end with the
statistics on the host; wall-clock around a synchronised call, the median over --reps alternations and the spread (min .. max).  For the
new call also the bytes its query pass must read -- 24 B per query point and 32 B per reference point and query (key and coordinates) --
over the whole call's time, as a share of the 8 TB/s HBM peak.  --evaluation also times evaluation.evaluate_pairs_sharded on 256
pre-rendered SUNCG pairs (batches of 32) with the records' overlap statistics from the new call and from the per-pair loop.
Writes profiles/overlap_time.txt (--out to write elsewhere).

  python tools/overlap_time.py [--reps 3] [--evaluation] [--out PATH]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def alternate(fa, fb, reps, inner=3):
    """(median, min, max) in ms per call of fa and of fb, alternating: every repetition times `inner` calls of fa, then one call of fb
    (the slower side), after one warm-up call of each."""
    import torch
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts, k in ((fa, ta, inner), (fb, tb, 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / k)
    st = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    return st(ta), st(tb)


def loop_pairs(host_clouds, R_gt):
    """the per-pair path: util.point_cloud_overlap on the host clouds of every pair -> [B,4]"""
    from relativepose_amd import util
    return np.array([util.point_cloud_overlap(host_clouds[2 * b], host_clouds[2 * b + 1], R_gt[b]) for b in range(len(R_gt))])


def host_clouds_of(pcd, vad):
    pc, va = pcd.cpu().numpy(), vad.cpu().numpy() != 0
    return [pc[k][va[k]] for k in range(len(pc))]


def main():
    import torch
    from relativepose_amd import _lib, evaluation as E, synth, util
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--evaluation", action="store_true", help="also time a 256-pair evaluation run with either source of the records' statistics")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# python tools/overlap_time.py --reps {args.reps}{' --evaluation' if args.evaluation else ''}, 1x MI355X (wall-clock of whole synchronised "
             "calls, median (min .. max) over the alternations; new = one util.point_cloud_overlap_dev / overlap_matrix_dev call, loop = the "
             "per-pair util.point_cloud_overlap loop the drivers ran before)"]

    def report(name, new, old, n_queries, P, note):
        (m, lo, hi), (om, olo, ohi) = new, old
        nbytes = n_queries * P * (24 + 32)
        faster = lo > 0 and olo > hi
        lines.append(f"{name}: new {m:.2f} ms ({lo:.2f} .. {hi:.2f}), loop {om:.1f} ms ({olo:.1f} .. {ohi:.1f}): {om / m:.1f} x"
                     f"{'' if faster else ' -- NOT faster beyond the spread'}; {n_queries} queries of {P} points, {nbytes / 1e9:.3f} GB for the query pass to "
                     f"read at least = {nbytes / (m * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (m * 1e-3) / HBM_PEAK:.2f} % of the 8 TB/s HBM peak; {note}")

    def paired(name, pcd, vad, R_gt):
        hc = host_clouds_of(pcd, vad)
        new_fn = lambda: [t.cpu() for t in util.point_cloud_overlap_dev(pcd, vad, R_gt)]
        got = np.stack([t.numpy() for t in new_fn()], 1)
        want = loop_pairs(hc, R_gt)
        same = np.array_equal(got[:, [0, 3]].view(np.uint64), want[:, [0, 3]].view(np.uint64))
        new, old = alternate(new_fn, lambda: loop_pairs(hc, R_gt), args.reps)
        ov = got[:, 0]
        report(name, new, old, 2 * len(R_gt), pcd.shape[1],
               f"overlap and pc_nearest bitwise the loop's: {same}; pairs per bucket {[int((np.array([E.overlap_bucket(v) for v in ov]) == k).sum()) for k in E.OVERLAPS]}")

    # 1. unrelated poses
    d = synth.make_pairs(32, 4000, "suncg")
    pcd, vad = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(64, 160, 640)).to(dev), "suncg")
    paired("pairs (32 make_pairs SUNCG pairs)", pcd, vad, [np.matmul(d["R"][b, 1], np.linalg.inv(d["R"][b, 0])) for b in range(32)])
    # 2. mined pairs
    sb = E.SceneBatch(32, 4000, "suncg", "second", 1, views=6, balanced=True)
    d = sb.take(range(32))
    pcd, vad = util.depth2pc_dev(torch.from_numpy(d["depth"].reshape(64, 160, 640)).to(dev), "suncg")
    paired("scenes (32 SceneBatch pairs)", pcd, vad, [np.matmul(d["R"][b, 1], np.linalg.inv(d["R"][b, 0])) for b in range(32)])
    # 3. full frames
    depth = np.concatenate([synth.make_full_res_pair(50 + k)[0][0] for k in range(4)])
    dd = torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
    pcd = torch.empty(8, 480 * 640, 3, dtype=torch.float64, device=dev)
    vad = torch.empty(8, 480 * 640, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().relpose_depth2pc_full(_lib.ptr(dd), _lib.ptr(pcd), _lib.ptr(vad), 8, 480, 640, _lib.stream_ptr()), "relpose_depth2pc_full")
    paired("frames (4 full-frame pairs)", pcd, vad, [synth.random_rigid(np.random.RandomState(60 + k), 0.05, 0.1) for k in range(4)])
    del pcd, vad
    # 4. the matrix of one scene
    sc = synth.render_scene(77, 32, "suncg")
    pcd, vad = util.depth2pc_dev(torch.from_numpy(sc["depth"]).to(dev), "suncg")
    hc = host_clouds_of(pcd, vad)
    ij = [(i, j) for i in range(32) for j in range(i + 1, 32)]
    R_ij = [np.matmul(sc["R"][j], np.linalg.inv(sc["R"][i])) for i, j in ij]
    hc2 = [hc[k] for p in ij for k in p]
    new_fn = lambda: [t.cpu() for t in util.overlap_matrix_dev(pcd, vad, sc["R"])]
    frac = new_fn()[0].numpy()
    want = loop_pairs(hc2, R_ij)
    sym = np.array([max(frac[i, j], frac[j, i]) for i, j in ij])
    new, old = alternate(new_fn, lambda: loop_pairs(hc2, R_ij), args.reps, inner=1)
    report("matrix (one 32-view scene, 992 directed queries against the loop over its 496 pairs)", new, old, 992, pcd.shape[1],
           f"symmetric overlaps within 1e-12 of the loop's: {bool(np.allclose(sym, want[:, 0], rtol=0, atol=1e-12))} (the loop inverts R_gt, the matrix forms "
           f"R_i inv(R_j) itself); pairs per bucket {[int((np.array([E.overlap_bucket(v) for v in sym]) == k).sum()) for k in E.OVERLAPS]}")

    if args.evaluation:
        from types import SimpleNamespace
        from relativepose_amd import params, weights
        from relativepose_amd.model import SCNet
        from relativepose_amd.pipeline import RelativePosePipeline
        ds, mm, S = "suncg", "second", 15
        net = SCNet(SimpleNamespace(batchnorm=1, useTanh=1, skipLayer=1, outputType="rgbdnsf", snumclass=S))
        net.load_state_dict(weights.make_state_dict(7, S))
        pipe = RelativePosePipeline(net, ds, mm, params.final_params(ds))
        batches = [E.SyntheticBatch(32, 4000 + k, ds, mm, 200).take(range(32)) for k in range(0, 256, 32)]

        def loop_stats(pcs_dev, valid_dev, R_gts):
            hc = host_clouds_of(pcs_dev, valid_dev)
            r = loop_pairs(hc, R_gts)
            return r[:, 0], r[:, 3]

        new_stats = E._pair_overlap_stats
        run = lambda: E.evaluate_pairs_sharded(pipe, batches, dev)

        def run_loop():
            E._pair_overlap_stats = loop_stats
            try:
                return run()
            finally:
                E._pair_overlap_stats = new_stats

        a, b = run(), run_loop()
        same = all(x[k] == y[k] for x, y in zip(a, b) for k in ("overlap", "pc_nearest", "pc_dist", "cam_dist"))
        (m, lo, hi), (om, olo, ohi) = alternate(run, run_loop, args.reps, inner=1)
        lines.append(f"evaluation (evaluate_pairs_sharded, 256 pre-rendered SUNCG pairs in batches of 32, 200 keypoints, f32): {m / 1e3:.2f} s "
                     f"({lo / 1e3:.2f} .. {hi / 1e3:.2f}) with the new call, {om / 1e3:.2f} s ({olo / 1e3:.2f} .. {ohi / 1e3:.2f}) with the per-pair loop; "
                     f"the records' four statistics are identical: {same}")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
