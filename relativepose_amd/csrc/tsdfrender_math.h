// The arithmetic of relpose_tsdf_render (the contract stands above the declaration in include/relpose.h, tests/render_model.py
// restates it in numpy): a pixel's ray, a sample's cell, the eight-corner value / gradient / colour in relpose_tsdf_align's order of lerps, the
// conservative clip of a ray against the box and the march itself.  Only + - * / sqrt floor, one statement per rounding: the including file is
// built with -ffp-contract=off.  The functions are __host__ __device__ and depend on <cmath> alone, so a host program can run this very text
// against the model.  tsdfalign_math.h gives the rigid inverse (align_inverse) and the fixed-point scale; its align_row classifies saturated
// corners and quantises, which a renderer must not, so the lerps are restated here in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsdfalign_math.h"

#define RP_RENDER_FN __host__ __device__ __forceinline__

constexpr int kRenderBrick = 8;                  // a brick is 8^3 cells
constexpr int kRenderMaxSteps = 65536;
constexpr int kRenderMiss = 0, kRenderHit = 1, kRenderBack = 2;

struct RenderVolume {
    int nx, ny, nz, min_weight;
    int bx, by, bz;                              // bricks per axis: ceil((n - 1) / 8)
    size_t nvox;
    double voxel;
    double origin[3];
    const int* tsdf;                             // the scene's [nz, ny, nx]
    const int* weight;
    const unsigned* color;                       // the scene's [3, nz, ny, nx] or NULL
    const uint8_t* flags;                        // the scene's [bz, by, bx] or NULL: every in-range sample is evaluated
};

struct RenderCell {                              // where a sample lies
    bool in;                                     // its world point is finite and its cell lies within 0 .. n - 2 on every axis
    bool flagged;                                // ... and that cell's brick is flagged (false without flags)
    int i0[3];
    double f[3];
};

struct RenderPixel {
    float depth, normal[3], color[3];
    int cls, n_evaluated;
};

RP_RENDER_FN int render_bricks(int n) { return n > 1 ? (n - 1 + kRenderBrick - 1) / kRenderBrick : 0; }

// Rs[k] v: an exact signed permutation (skybox.h's rp_face_rot, restated so that a host program can run it)
RP_RENDER_FN void render_face_rot(int k, double x, double y, double z, double& ox, double& oy, double& oz) {
    switch (k & 3) {
        case 0: ox = x; oy = y; oz = z; break;
        case 1: ox = -z; oy = y; oz = x; break;
        case 2: ox = -x; oy = y; oz = -z; break;
        default: ox = z; oy = y; oz = -x; break;
    }
}

// the camera-frame direction per unit of face depth of panorama pixel (row, col): the ray relpose_tsdf_align unprojects
RP_RENDER_FN void render_ray(bool suncg, int h, int row, int col, double dir[3]) {
    const int slot = col / h, px = col - slot * h;
    const double xn = (2.0 * (double)px) / (double)h - 1.0;
    const double yn = 1.0 - (2.0 * (double)row) / (double)h;
    render_face_rot(suncg ? slot : (slot + 3) & 3, xn, yn, -1.0, dir[0], dir[1], dir[2]);
}

RP_RENDER_FN double render_depth_of(double d_min, double step, int k) { return d_min + (double)k * step; }

// sample k of the ray: the world point of d_k * dir under W, its cell and fractions, and the cell's brick flag
RP_RENDER_FN void render_cell(const RenderVolume& g, const double* W, const double* dir, double d, RenderCell& c) {
    const double x = d * dir[0], y = d * dir[1], z = d * dir[2];
    const int n[3] = {g.nx, g.ny, g.nz};
    bool in = true;
    double fl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = ((W[4 * a] * x + W[4 * a + 1] * y) + W[4 * a + 2] * z) + W[4 * a + 3];
        const double u = (q - g.origin[a]) / g.voxel - 0.5;
        fl[a] = floor(u);
        in = in && std::isfinite(q) && fl[a] >= 0.0 && fl[a] <= (double)(n[a] - 2);
        c.f[a] = u - fl[a];
    }
    c.in = in;
    c.flagged = false;
    if (!in) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) c.i0[a] = (int)fl[a];
    if (g.flags)
        c.flagged = g.flags[((size_t)(c.i0[2] / kRenderBrick) * (size_t)g.by + (size_t)(c.i0[1] / kRenderBrick)) * (size_t)g.bx +
                            (size_t)(c.i0[0] / kRenderBrick)] != 0;
}

RP_RENDER_FN void render_lerp8(const double* t, const double* f, double& r, double* grad) {
    const double d00 = t[1] - t[0], d10 = t[3] - t[2], d01 = t[5] - t[4], d11 = t[7] - t[6];
    const double a00 = t[0] + f[0] * d00, a10 = t[2] + f[0] * d10, a01 = t[4] + f[0] * d01, a11 = t[6] + f[0] * d11;
    const double c0 = a10 - a00, c1 = a11 - a01;
    const double b0 = a00 + f[1] * c0, b1 = a01 + f[1] * c1;
    const double gz = b1 - b0;
    r = b0 + f[2] * gz;
    if (grad) {
        grad[2] = gz;
        grad[1] = c0 + f[2] * (c1 - c0);
        const double e0 = d00 + f[1] * (d10 - d00), e1 = d01 + f[1] * (d11 - d01);
        grad[0] = e0 + f[2] * (e1 - e0);
    }
}

// An evaluation: the sixteen loads of an in-range sample.  False if a corner is unknown; else t, with grad the gradient per voxel and with
// want_col the three colour channels in col.  All sixteen loads are issued before the first is used.
RP_RENDER_FN bool render_sample(const RenderVolume& g, const RenderCell& c, double& t, double* grad, double* col, bool want_col) {
    size_t lin[8];
    int w[8], s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        lin[e] = ((size_t)(c.i0[2] + (e >> 2 & 1)) * (size_t)g.ny + (size_t)(c.i0[1] + (e >> 1 & 1))) * (size_t)g.nx + (size_t)(c.i0[0] + (e & 1));
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = g.weight[lin[e]];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = g.tsdf[lin[e]];
    bool known = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) known = known && w[e] >= g.min_weight;
    if (!known) return false;
    double v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (double)s[e] / (kAlignFix * (double)w[e]);
    render_lerp8(v, c.f, t, grad);
    if (want_col) {                                                  // g.color may be NULL otherwise: nothing is read from it
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (double)g.color[(size_t)ch * g.nvox + lin[e]] / (255.0 * (double)w[e]);
            render_lerp8(v, c.f, col[ch], nullptr);
        }
    }
    return true;
}

// A conservative range k0 .. k1 of the samples that can be in range: the slabs origin_a .. origin_a + n_a voxel lie half a voxel outside the
// cells' region on every side; the range is cut only where every rounding error of a sample's world point (bounded by 2^-48 of the sum of the
// magnitudes that enter it) stays below a quarter voxel, and is widened by one sample at each end.  Whatever is not finite leaves 0 .. n_steps - 1.
RP_RENDER_FN void render_clip(const RenderVolume& g, const double* W, const double* dir, double d_min, double step, int n_steps, int& k0, int& k1) {
    k0 = 0;
    k1 = n_steps - 1;
    const int n[3] = {g.nx, g.ny, g.nz};
    const double d_max = d_min + (double)n_steps * step;
    double lo = d_min, hi = d_max;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double w = (W[4 * a] * dir[0] + W[4 * a + 1] * dir[1]) + W[4 * a + 2] * dir[2];
        const double mag = d_max * ((fabs(W[4 * a] * dir[0]) + fabs(W[4 * a + 1] * dir[1])) + fabs(W[4 * a + 2] * dir[2])) + fabs(W[4 * a + 3]) +
                           fabs(g.origin[a]) + (double)n[a] * g.voxel;
        if (!(mag * 3.552713678800501e-15 <= 0.25 * g.voxel)) return;          // 2^-48; NaN and inf land here
        const double s0 = g.origin[a] - W[4 * a + 3], s1 = (g.origin[a] + (double)n[a] * g.voxel) - W[4 * a + 3];
        if (w == 0.0) {
            empty = empty || s0 > 0.0 || s1 < 0.0;                              // parallel to the slab and outside it: no sample
            continue;
        }
        const double e0 = s0 / w, e1 = s1 / w;
        lo = fmax(lo, fmin(e0, e1));
        hi = fmin(hi, fmax(e0, e1));
    }
    if (empty || !(lo <= hi)) {
        k0 = 1;
        k1 = 0;
        return;
    }
    const double a0 = floor((lo - d_min) / step) - 1.0, a1 = floor((hi - d_min) / step) + 2.0;
    if (a0 > 0.0) k0 = a0 < (double)n_steps ? (int)a0 : n_steps;
    if (a1 < (double)(n_steps - 1)) k1 = a1 > -1.0 ? (int)a1 : -1;
}

// One pixel: the march over the samples k0 .. k1 (render_clip's, or 0 .. n_steps - 1: samples outside are out of range by the clip's
// argument).  W: camera -> world [3][4]; its rotation block transposed is the pose's.  With flags a sample is evaluated only if the cell of
// sample k - 1, k or k + 1 (within 0 .. n_steps - 1) lies in a flagged brick.  At a hit both samples of the pair are evaluated again, with
// gradient and colour: the march itself carries one value.
RP_RENDER_FN void render_march(const RenderVolume& g, const double* W, const double* dir, double d_min, double step, int k0, int k1,
                               bool want_normal, bool want_color, RenderPixel& o) {
    o.depth = 0.0f;
    o.cls = kRenderMiss;
    o.n_evaluated = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.normal[a] = o.color[a] = 0.0f;
    RenderCell cur, nxt;
    bool pv = false, pflag = false;
    double pt = 0.0;
    int hit = -1;
    if (k0 <= k1) render_cell(g, W, dir, render_depth_of(d_min, step, k0), cur);
    for (int k = k0; k <= k1; ++k) {
        nxt.in = nxt.flagged = false;
        if (k < k1) render_cell(g, W, dir, render_depth_of(d_min, step, k + 1), nxt);
        const bool ev = cur.in && (!g.flags || pflag || cur.flagged || nxt.flagged);
        bool v = false;
        double t = 0.0;
        if (ev) {
            ++o.n_evaluated;
            v = render_sample(g, cur, t, nullptr, nullptr, false);
        }
        if (v && pv) {
            if (pt >= 0.0 && t < 0.0) {
                hit = k;
                break;
            }
            if (pt < 0.0 && t >= 0.0) {
                o.cls = kRenderBack;
                break;
            }
        }
        pv = v;
        pt = t;
        pflag = cur.flagged;
        cur = nxt;
    }
    if (hit < 0) return;
    o.cls = kRenderHit;
    const double da = render_depth_of(d_min, step, hit - 1), db = render_depth_of(d_min, step, hit);
    RenderCell ca, cb;
    render_cell(g, W, dir, da, ca);
    render_cell(g, W, dir, db, cb);
    double ta, tb, ga[3], gb[3], cola[3], colb[3];
    render_sample(g, ca, ta, ga, cola, want_color);
    render_sample(g, cb, tb, gb, colb, want_color);
    const double s = ta / (ta - tb);
    o.depth = (float)(da + s * step);
    if (want_normal) {
        double nv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) nv[a] = ga[a] + s * (gb[a] - ga[a]);
        const double nn = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
        if (nn > 0.0)
#pragma unroll
            for (int a = 0; a < 3; ++a) nv[a] = nv[a] / nn;
#pragma unroll
        for (int i = 0; i < 3; ++i) o.normal[i] = (float)((W[i] * nv[0] + W[4 + i] * nv[1]) + W[8 + i] * nv[2]);      // the pose's rotation: T_ij = W_ji
    }
    if (want_color)
        for (int ch = 0; ch < 3; ++ch) o.color[ch] = (float)(cola[ch] + s * (colb[ch] - cola[ch]));
}
