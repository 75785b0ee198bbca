// Which pixels of the network output a keypoint is sampled from (relpose_sample_primitives, csrc/geometry.hip): the ONE place that turns
// a keypoint (px, py) into pixel indices.  sample_primitives_kernel reads through it and the sampled tail of the SCNet forward
// (heads_sampled_kernel, csrc/scnet.hip: RELPOSE_FWD_SAMPLED_OUTPUTS) writes through it, so the two cannot drift.
// Plain C++ (host and device); only conversions, one division, one product and a floor per axis: nothing that FMA contraction could change.
#pragma once
#include "rp_math.h"                                // RP_HD

// Normal and depth: rputil.getPixel :88-119 blends channels 3:7 at the block (ty .. ty + 1, tx .. tx + 1).
// Features: rputil.interpolate :43-58 in float32 -- pt = (x / W, y / H) cast to float32, x = pt * (W - 1) -- blends the 32 feature channels
// at the block (yi .. yi + 1, xi .. xi + 1); x / y / x0 / y0 are the float32 coordinates its weights come from.
struct RpSamplePix { int tx, ty, xi, yi; float x, y, x0, y0; };
RP_HD RpSamplePix rp_sample_pixels(double px, double py, int h) {
    const int W = 4 * h;
    RpSamplePix s;
    s.tx = (int)floor(px); s.ty = (int)floor(py);
    const float ptx = (float)(px / W), pty = (float)(py / h);
    s.x = ptx * (float)(W - 1); s.y = pty * (float)(h - 1);
    s.x0 = floorf(s.x); s.y0 = floorf(s.y);
    s.xi = (int)s.x0; s.yi = (int)s.y0;
    return s;
}
