"""CPU census of conv4's row lists on the bench's seeded inputs (tests/conv4_rows_model.py; no GPU needed):
python tools/conv4_rows_census.py [config ...]      -> the table of profiles/conv4_rows_census.txt

Inputs as tools/zero_tiles_census.py: bench.py's first batch, the oracle's masked views and warps at the ground-truth relative poses, the
oracle's resize.  Per level of a step the (image, stream, pixel) rows of conv4's launched K slices and the share a row list drops (every
slice listed, RELPOSE_TUNE_CONV4_ROWS = 2: the census is of the rows, not of the density rule).  Level 0 runs the level-0 plan (the
warped slices' rows are those of one image pair), levels 1-2 the self-cached plan (the warped slices only)."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv4_rows_model as M                # noqa: E402
from zero_tiles_census import CONFIGS, batch_input      # noqa: E402


def main():
    configs = [int(a) for a in sys.argv[1:]] or [1, 2, 3]
    pairs = 32
    print("config | level 0 plan | levels 1-2 (self-cached) | slices on the list path at theta = %.2f (level 0 / 1-2)" % (M.THETA_1024 / 1024))
    for c in configs:
        x = batch_input(c, pairs)
        x0 = F.interpolate(torch.from_numpy(x), [224, 224], mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous().numpy()
        xz = x0.copy()
        xz[..., 8:16] = 0                    # util.warping returns zeros for the identity pose
        cells = []
        for xl, plan in ((xz, "zero_warp"), (x0, "self_cached")):
            r = M.counts(xl, plan, 2)
            rows = sum(a + b for a, b, _ in r)
            lp = sum(1 for (a, b, p), (_, _, p0) in zip(r, M.counts(xl, plan, 0)) if p0)
            cells.append((100.0 * sum(b for _, b, _ in r) / rows, rows, lp, sum(1 for a, b, _ in r if a + b)))
        print(f"{c} ({CONFIGS[c][0]}, {CONFIGS[c][1]}) | {cells[0][0]:.1f} % of {cells[0][1]} rows droppable | {cells[1][0]:.1f} % of {cells[1][1]} | "
              f"{cells[0][2]} of {cells[0][3]} / {cells[1][2]} of {cells[1][3]}")


if __name__ == "__main__":
    main()
