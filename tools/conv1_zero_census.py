"""CPU census of conv1's zero-unit skipping on the bench's seeded inputs (tests/zero_tiles_model.py; no GPU needed):
python tools/conv1_zero_census.py [config ...]      -> the table of profiles/conv1_zero_census.txt

A unit is one (image, stream, 8 x 32 tile) block of A1 that conv1_mfma_kernel's plan launches.  It passes iff the occupancy bits of block
rows by - 1 .. by + 1 and block columns 4 tx - 1 .. 4 tx + 4 of its stream are clear and none of those words carries the non-finite flag
(csrc/scnet.hip: c1z_unit_zero).  Inputs as in tools/zero_tiles_census.py: level 0 runs the level-0 plan (warped streams on one image
pair, warped channels zero), levels 1-2 the self-cached plan (warped streams only)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zero_tiles_model as Z                # noqa: E402
import zero_tiles_census as ZC              # noqa: E402

TY, TX = 28, 7                              # conv1 tiles per image: 28 rows of 8 pixels x 7 columns of 32 pixels


def unit_zero(occ, nonfinite_rows):
    """occ [n, 6, 28, 28] bool, nonfinite_rows [n, 6, 28] bool (bit 31 of the word of that block row) -> [n, 6, 28, 7] bool."""
    n = occ.shape[0]
    z = np.zeros((n, 6, TY, TX), bool)
    for by in range(TY):
        y0, y1 = max(by - 1, 0), min(by + 2, Z.NB)
        bad = nonfinite_rows[:, :, y0:y1].any(2)
        for tx in range(TX):
            x0, x1 = Z.block_range(tx)
            z[:, :, by, tx] = ~occ[:, :, y0:y1, x0:x1].any((2, 3)) & ~bad
    return z


def nonfinite_rows(x0):
    bits = np.asarray(x0, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    bad = (bits >= np.uint32(0x7f800000)).reshape(x0.shape[0], Z.NB, Z.BLK * Z.RS, 16).any(2)     # [n, 28, 16]
    return np.stack([bad[..., Z.stream_channels(q)].any(-1) for q in range(6)], 1)                # [n, 6, 28]


def launched(plan, n):
    """[n, 6] bool: the (image, stream) blocks conv1_mfma_kernel computes in this plan."""
    m = np.zeros((n, 6), bool)
    for q, nimg in Z.plan_members(plan, n):
        m[:nimg, q] = True
    return m


def main():
    configs = [int(a) for a in sys.argv[1:]] or [1, 2, 3]
    pairs = 32
    for c in configs:
        x = ZC.batch_input(c, pairs)
        x0 = F.interpolate(torch.from_numpy(x), [224, 224], mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous().numpy()
        print(f"config {c} ({ZC.CONFIGS[c][0]}, {ZC.CONFIGS[c][1]}), {pairs} pairs = {2 * pairs} images")
        tot = [0, 0]
        for level, plan in ((0, "zero_warp"), (1, "self_cached"), (2, "self_cached")):
            xl = x0
            if level == 0:                   # util.warping returns zeros for the identity pose
                xl = x0.copy()
                xl[..., 8:16] = 0
            occ, _ = Z.occupancy(xl)
            z = unit_zero(occ, nonfinite_rows(xl))
            m = launched(plan, len(xl))
            units = int(m.sum()) * TY * TX
            zero = int(z[m].sum())
            tot[0] += units
            tot[1] += zero
            per = "  ".join(f"q{q}: {100.0 * z[:, q][m[:, q]].mean():4.1f} %" for q in range(6) if m[:, q].any())
            print(f"  level {level} ({plan:11s})  conv1: {units:6d} units, {zero:6d} zero = {100.0 * zero / units:4.1f} %   ({per})")
        print(f"  step: {tot[0]} units launched, {tot[1]} pass = {100.0 * tot[1] / tot[0]:.1f} %")


if __name__ == "__main__":
    main()
