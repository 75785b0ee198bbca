"""CPU census of SCNet's zero-tile skipping on the bench's seeded inputs (tests/zero_tiles_model.py; no GPU needed):
python tools/zero_tiles_census.py [config ...]      -> the table of profiles/zero_tiles_census.txt

Per config: bench.py's first batch (synth.make_pairs(pairs, 1000 * (config + 1), dataset)), the oracle's masked views and warps at the
ground-truth relative poses, the oracle's resize; then per level of a step the conv2 / conv3 workgroups the plan launches and the share
the tile lists drop.  Level 0 runs the level-0 plan (warped streams on one image pair), levels 1-2 the self-cached plan."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import geom_oracle as G          # noqa: E402
from relativepose_amd import synth          # noqa: E402
import zero_tiles_model as Z                # noqa: E402

CONFIGS = {1: ("suncg", "second"), 2: ("matterport", "second"), 3: ("scannet", "kinect")}


def batch_input(config, pairs):
    ds, mm = CONFIGS[config]
    d = synth.make_pairs(pairs, 1000 * (config + 1), ds)
    xs = []
    for b in range(pairs):
        views = [G.build_view(d["rgb"][b, v], d["norm"][b, v], d["depth"][b, v], mm)[0] for v in range(2)]
        R = np.linalg.inv(d["R"][b, 1]) @ d["R"][b, 0]
        t2s = G.warping(views[1], np.linalg.inv(R), ds).astype(np.float32)
        s2t = G.warping(views[0], R, ds).astype(np.float32)
        xs += [np.concatenate((views[0], t2s), 1), np.concatenate((views[1], s2t), 1)]
    return np.concatenate(xs)


def main():
    configs = [int(a) for a in sys.argv[1:]] or [1, 2]
    pairs = 32
    for c in configs:
        x = batch_input(c, pairs)
        nzw = [(x[i, 8:16] != 0).any(0).mean() for i in range(len(x))]
        x0 = F.interpolate(torch.from_numpy(x), [224, 224], mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous().numpy()
        print(f"config {c} ({CONFIGS[c][0]}, {CONFIGS[c][1]}), {pairs} pairs = {2 * pairs} images; warped view nonzero pixels "
              f"{100 * min(nzw):.1f}-{100 * max(nzw):.1f} % (mean {100 * np.mean(nzw):.1f} %)")
        tot = {2: [0, 0], 3: [0, 0]}
        for level, plan in ((0, "zero_warp"), (1, "self_cached"), (2, "self_cached")):
            xl = x0
            if level == 0:                   # util.warping returns zeros for the identity pose
                xl = x0.copy()
                xl[..., 8:16] = 0
            r = Z.counts(xl, plan)
            line = f"  level {level} ({plan:11s})"
            for layer in (2, 3):
                comp, drop = r[layer]
                tot[layer][0] += comp + drop
                tot[layer][1] += drop
                line += f"  conv{layer}: {comp + drop:5d} workgroups, {drop:5d} dropped = {100.0 * drop / (comp + drop):4.1f} %"
            print(line)
        r = Z.counts(x0, "full")
        print("  (full plan, warped input)  " + "  ".join(f"conv{l}: {sum(r[l]):5d} workgroups, {r[l][1]:5d} dropped = {100.0 * r[l][1] / sum(r[l]):4.1f} %"
                                                           for l in (2, 3)))
        a = tot[2][0] + tot[3][0]
        b = tot[2][1] + tot[3][1]
        print(f"  step: conv2 {100.0 * tot[2][1] / tot[2][0]:.1f} %, conv3 {100.0 * tot[3][1] / tot[3][0]:.1f} %, both {100.0 * b / a:.1f} % of the workgroups dropped")


if __name__ == "__main__":
    main()
