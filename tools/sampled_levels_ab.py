"""A/B of RelativePosePipeline(sampled_levels=...): bench.py's compute-only loop (configs[k], 6 prepared batches rotated, 3 in flight, the pose
gather per step) with the pose-outputs levels computed at the keypoints only (True, what bench.py measures) or densely (False, the opt-out).
bench.py has no switch for it and is not to grow one; this drives run_pipelined the way bench does.

Like tools/level_outputs_ab.py it mirrors bench.py's run(): the weights (`_shared_state_dict(7, S, rank, world)`, a private helper of bench), the
pipeline's `max_edges` formula, the batch seeds (`1000 * (config + 1) + lo + 100000 * j`), the six prepared batches and the compute-only branch
of `run_steps` (depth 3, the per-step gather).  If bench.py changes any of these, change them here too: nothing checks that the two agree.

    python tools/sampled_levels_ab.py --config 1 --steps 60 --rounds 3        # alternates the two arms, one line each per round
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import bench  # noqa: E402
from relativepose_amd import distributed as D  # noqa: E402
from relativepose_amd import params, synth  # noqa: E402
from relativepose_amd.model import SCNet  # noqa: E402
from relativepose_amd.pipeline import RelativePosePipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default=None)
    args = ap.parse_args()
    cfg = dict(bench.CONFIGS[args.config])
    prec = args.precision or cfg["precision"]
    ds, mm, h, S, N, nloc = cfg["dataset"], cfg["mask"], cfg["h"], cfg["S"], cfg["N"], cfg["pairs"]
    dev = torch.device("cuda", 0)
    net = SCNet(SimpleNamespace(batchnorm=1, useTanh=cfg["tanh"], skipLayer=1, outputType="rgbdnsf", snumclass=S))
    net.load_state_dict(bench._shared_state_dict(7, S, 0, 1))
    net.set_precision(prec)
    Cc = N * 5
    pipes = {a: RelativePosePipeline(net, ds, mm, params.final_params(ds), max_edges=min(Cc * (Cc - 1), (1 << 20) * max(1, (N // 200) ** 2)),
                                     sampled_levels=a) for a in (True, False)}
    batches = []
    for j in range(6):
        seed = 1000 * (args.config + 1) + 100000 * j
        dj = synth.make_pairs(nloc, seed, ds, h=h)
        pj, wj = synth.make_keypoints(nloc, N, seed, mm, h=h)
        batches.append(pipes[True].prepare(dj["rgb"], dj["norm"], dj["depth"], pj, wj, dev))

    def run(pipe, k):
        return pipe.run_pipelined(batches, k, lambda i, pose, status: D.gather_poses(pose, status, nloc, 1), depth=3)[-1]

    for pipe in pipes.values():
        run(pipe, 3)
        run(pipe, args.warmup)
    for rnd in range(args.rounds):
        for arm, pipe in pipes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pipe, args.steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"config": args.config, "precision": prec, "sampled_levels": arm, "round": rnd, "ms_per_step": dt / args.steps * 1e3,
                              "pairs_per_s": nloc * args.steps / dt}), flush=True)


if __name__ == "__main__":
    main()
