// Completion quality: the losses of the reference's validation pass (learner.step(mode='val'), mainPanoCompletion2view.py:457-602) for a
// batch of network outputs -- dataMask-weighted L1 on rgb / normal / depth (:553-561), cross-entropy on the semantic head (:565-567) and
// the contrastive descriptor loss (contrast_loss, :429-455).  Forward only.  The contract -- the fp32 terms, the float64 sums, the
// regions, the slots -- is DESIGN.md §4.11; tests/completion_model.py restates it in numpy.  Built with -ffp-contract=off.
//
//   loss_kernel          one block per 1024 pixels of an image, four adjacent pixels per thread (16-byte loads of every map): the seven
//                        L1 channels, then the S logits twice (the maximum, then the exponentials: the second read comes from the cache),
//                        twelve float64 partial sums per block (wave DPP sum, LDS, thread 0) into a fixed slot of the workspace, and the
//                        per-pixel CE / w maps for ce_cross.  The 32 feature channels are never touched
//   loss_cross_kernel    one thread per pixel over the N images in ascending order, one partial per block
//   loss_final_kernel    block i sums image i's partials in block order; block N the ce_cross partials
//   contrast_kernel      one block per 16 correspondences of a pair, one wave per correspondence at a time: the source descriptor sits in
//                        LDS (same-address broadcast reads), lane m takes the negatives m, m + 64, ...; partials per block
//   contrast_final_kernel   one block per pair sums its partials in block order
// No floating-point atomics anywhere: the partial grids depend on the map size (and K) alone, so every sum has one order whatever the
// batch around it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "desc_dist.h"

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossVals = 12;            // sums[5][2], ce_mag, n_bad_label (an integer count, exact in float64)
constexpr int kCrossThreads = 256;

struct LossBufs {
    int N, Ct, S, HW, nblk, nblk2;
    const float* f;          // [N, Ct, HW]
    const float* complete;   // [N, 7, HW]
    const uint8_t* label;    // [N, HW] or NULL
    const float* mask;       // [N, HW]
    const float* weight;     // [N, HW] or NULL
    double* part;            // [N, nblk, kLossVals]
    double* cross_part;      // [nblk2] or NULL
    double* ce_map;          // [N, HW] or NULL
    float* w_map;            // [N, HW] or NULL
    double* sums;
    double* ce_mag;
    double* ce_cross;
    int* n_bad;
};

__global__ __launch_bounds__(kLossThreads) void loss_kernel(LossBufs a) {
    __shared__ double red[kLossVals * (kLossThreads / 64)];
    const int i = blockIdx.y, tid = threadIdx.x;
    const size_t HW = (size_t)a.HW;
    const size_t p = ((size_t)blockIdx.x * kLossThreads + tid) * 4;       // HW is a multiple of 4: the four pixels are inside or outside as one
    double v[kLossVals];
#pragma unroll
    for (int k = 0; k < kLossVals; ++k) v[k] = 0.0;
    if (p < HW) {
        const float* fi = a.f + (size_t)i * a.Ct * HW + p;
        const float* ci = a.complete + (size_t)i * 7 * HW + p;
        const size_t ip = (size_t)i * HW + p;
        const float4 c6 = rp_ldg4(ci + 6 * HW);
        const float4 mk = rp_ldg4(a.mask + ip);
        const float4 wt = a.weight ? rp_ldg4(a.weight + ip) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const float w[4] = {(c6.x != 0.0f ? 1.0f : 0.0f) * wt.x, (c6.y != 0.0f ? 1.0f : 0.0f) * wt.y,
                            (c6.z != 0.0f ? 1.0f : 0.0f) * wt.z, (c6.w != 0.0f ? 1.0f : 0.0f) * wt.w};
        const bool obs[4] = {mk.x != 0.0f, mk.y != 0.0f, mk.z != 0.0f, mk.w != 0.0f};
#pragma unroll
        for (int ch = 0; ch < 7; ++ch) {
            const int row = ch < 3 ? 0 : (ch < 6 ? 1 : 2);
            const float4 x = rp_ldg4(fi + ch * HW);
            const float4 c = ch == 6 ? c6 : rp_ldg4(ci + ch * HW);
            const float xs[4] = {x.x, x.y, x.z, x.w}, cs[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = (double)fabsf((xs[e] - cs[e]) * w[e]);
                v[2 * row] += obs[e] ? 0.0 : t;            // (+0 is bitwise neutral on these non-negative sums)
                v[2 * row + 1] += obs[e] ? t : 0.0;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[8] += obs[e] ? 0.0 : (double)w[e];
            v[9] += obs[e] ? (double)w[e] : 0.0;
        }
        if (a.label) {
            const uint32_t l4 = *(RP_GLOBAL const uint32_t*)(a.label + ip);
            const int lab[4] = {(int)(l4 & 255u), (int)((l4 >> 8) & 255u), (int)((l4 >> 16) & 255u), (int)(l4 >> 24)};
            const float* z = fi + 7 * HW;
            float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            for (int c = 0; c < a.S; ++c) {
                const float4 q = rp_ldg4(z + c * HW);
                m[0] = fmaxf(m[0], q.x); m[1] = fmaxf(m[1], q.y); m[2] = fmaxf(m[2], q.z); m[3] = fmaxf(m[3], q.w);
            }
            double s[4] = {0.0, 0.0, 0.0, 0.0}, zl[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < a.S; ++c) {
                const float4 q = rp_ldg4(z + c * HW);
                const float qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[e] += exp((double)qs[e] - (double)m[e]);
                    zl[e] = c == lab[e] ? (double)qs[e] : zl[e];
                }
            }
            double ce[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = lab[e] < a.S;
                const double lse = (double)m[e] + log(s[e]);
                ce[e] = ok ? lse - zl[e] : 0.0;
                const double cw = ce[e] * (double)w[e];
                v[6] += obs[e] ? 0.0 : cw;
                v[7] += obs[e] ? cw : 0.0;
                v[10] += ok ? (double)w[e] * (fabs(lse) + fabs(zl[e])) : 0.0;
                v[11] += ok ? 0.0 : 1.0;
            }
            if (a.ce_map) {
                double* cm = a.ce_map + ip;
#pragma unroll
                for (int e = 0; e < 4; ++e) rp_stg(cm + e, ce[e]);
                rp_stg4(a.w_map + ip, make_float4(w[0], w[1], w[2], w[3]));
            }
        }
    }
    rp_block_sum<kLossVals>(v, red);
    if (tid == 0) {
        double* o = a.part + ((size_t)i * a.nblk + blockIdx.x) * kLossVals;
#pragma unroll
        for (int k = 0; k < kLossVals; ++k) o[k] = v[k];
    }
}

__global__ __launch_bounds__(kCrossThreads) void loss_cross_kernel(LossBufs a) {
    __shared__ double red[kCrossThreads / 64];
    const size_t HW = (size_t)a.HW;
    const size_t p = (size_t)blockIdx.x * kCrossThreads + threadIdx.x;
    double v[1] = {0.0};
    if (p < HW) {
        double sc = 0.0, sw = 0.0;
        for (int i = 0; i < a.N; ++i) {
            sc += a.ce_map[(size_t)i * HW + p];
            sw += (double)a.w_map[(size_t)i * HW + p];
        }
        v[0] = sc * sw;
    }
    rp_block_sum<1>(v, red);
    if (threadIdx.x == 0) a.cross_part[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(64) void loss_final_kernel(LossBufs a) {
    const int i = blockIdx.x, t = threadIdx.x;
    if (i < a.N) {
        if (t >= kLossVals) return;
        double s = 0.0;
        for (int b = 0; b < a.nblk; ++b) s += a.part[((size_t)i * a.nblk + b) * kLossVals + t];
        if (t < 10) a.sums[(size_t)i * 10 + t] = s;
        else if (t == 10) a.ce_mag[i] = s;
        else a.n_bad[i] = (int)s;
        return;
    }
    if (t != 0 || !a.ce_cross) return;
    double s = 0.0;
    if (a.cross_part)
        for (int b = 0; b < a.nblk2; ++b) s += a.cross_part[b];
    a.ce_cross[0] = s;
}

struct LossLayout {
    size_t part, cross_part, ce_map, w_map, total;
};

LossLayout loss_layout(int N, int H, int W, bool with_cross) {
    const size_t HW = (size_t)H * W;
    const size_t nblk = (HW / 4 + kLossThreads - 1) / kLossThreads, nblk2 = (HW + kCrossThreads - 1) / kCrossThreads;
    LossLayout l{};
    size_t o = 0;
    l.part = o; o += rp_align((size_t)N * nblk * kLossVals * sizeof(double));
    l.cross_part = o; o += with_cross ? rp_align(nblk2 * sizeof(double)) : 0;
    l.ce_map = o; o += with_cross ? rp_align((size_t)N * HW * sizeof(double)) : 0;
    l.w_map = o; o += with_cross ? rp_align((size_t)N * HW * sizeof(float)) : 0;
    l.total = o;
    return l;
}

bool loss_shape_ok(int N, int H, int W) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= (1ll << 30) && ((long long)H * W) % 4 == 0;
}

// ------------------------------------------------------------------------------------------------------------- contrastive loss
constexpr int kCtThreads = 256;
constexpr int kCtWaves = kCtThreads / 64;
constexpr int kCtPerWave = 4;
constexpr int kCtPerBlock = kCtWaves * kCtPerWave;      // correspondences per block

struct ContrastBufs {
    int B, Ct, off, C, h, K, M, nblk;
    float margin;
    const float* f;          // [2B, Ct, h, 4h]
    const int* idx_src;      // [B, K, 2] (x, y)
    const int* idx_tgt;
    const uint8_t* pair_valid;
    const int* neg;          // [B, K, M, 2] (x, y)
    double* part_d;          // [B, nblk, 2]
    int* part_i;             // [B, nblk, 2]
    double* pos_sum;
    double* neg_sum;
    int* n_active;
    int* n_skipped;
};

// the pixel offset y * 4h + x of (x, y), or -1 outside the map
__device__ __forceinline__ int map_pixel(const int* xy, int h) {
    const int w = 4 * h, x = xy[0], y = xy[1];
    return (x < 0 || x >= w || y < 0 || y >= h) ? -1 : y * w + x;
}

__global__ __launch_bounds__(kCtThreads) void contrast_kernel(ContrastBufs r) {
    __shared__ float sdesc[kCtWaves][RELPOSE_DESC_MAX_CHANNELS];
    __shared__ double red[2 * kCtWaves];
    __shared__ int redi[2 * kCtWaves];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool pv = !r.pair_valid || r.pair_valid[b];      // uniform over the block
    const size_t HW = (size_t)r.h * 4 * r.h;
    const float* fs = r.f + ((size_t)(2 * b) * r.Ct + r.off) * HW;
    const float* ft = r.f + ((size_t)(2 * b + 1) * r.Ct + r.off) * HW;
    double v[2] = {0.0, 0.0};                               // positive, negative
    int act = 0, skip = 0;
    for (int j = 0; j < kCtPerWave; ++j) {                  // the same trip count in every wave: the barriers below are uniform
        const int k = (blockIdx.x * kCtWaves + wave) * kCtPerWave + j;
        const bool have = pv && k < r.K;
        const size_t ok = (size_t)b * r.K + (have ? k : 0);
        const int ps = have ? map_pixel(r.idx_src + 2 * ok, r.h) : -1;
        __syncthreads();                                    // the previous correspondence's descriptor has been read
        if (ps >= 0 && lane < r.C) sdesc[wave][lane] = fs[(size_t)lane * HW + ps];
        __syncthreads();
        if (!have) continue;
        if (lane == 0) {
            const int pt = map_pixel(r.idx_tgt + 2 * ok, r.h);
            if (ps < 0 || pt < 0) ++skip;
            else v[0] += (double)rp_desc_dist2(sdesc[wave], 1, ft + pt, HW, r.C);
        }
        const int* ng = r.neg + ok * r.M * 2;
        for (int m = lane; m < r.M; m += 64) {
            const int pn = map_pixel(ng + 2 * (size_t)m, r.h);
            if (ps < 0 || pn < 0) { ++skip; continue; }
            const float d = rp_desc_dist2(sdesc[wave], 1, ft + pn, HW, r.C);
            v[1] += (double)fmaxf(r.margin - d, 0.0f);
            act += d < r.margin ? 1 : 0;
        }
    }
    rp_block_sum<2>(v, red);
    act = rp_wave_sum_i(act);
    skip = rp_wave_sum_i(skip);
    if (lane == 0) { redi[2 * wave] = act; redi[2 * wave + 1] = skip; }
    __syncthreads();
    if (tid == 0) {
        const size_t o = ((size_t)b * r.nblk + blockIdx.x) * 2;
        int na = 0, ns = 0;
#pragma unroll
        for (int w = 0; w < kCtWaves; ++w) { na += redi[2 * w]; ns += redi[2 * w + 1]; }
        r.part_d[o] = v[0]; r.part_d[o + 1] = v[1];
        r.part_i[o] = na; r.part_i[o + 1] = ns;
    }
}

__global__ __launch_bounds__(64) void contrast_final_kernel(ContrastBufs r) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    double sp = 0.0, sn = 0.0;
    int na = 0, ns = 0;
    for (int q = 0; q < r.nblk; ++q) {
        const size_t o = ((size_t)b * r.nblk + q) * 2;
        sp += r.part_d[o]; sn += r.part_d[o + 1];
        na += r.part_i[o]; ns += r.part_i[o + 1];
    }
    r.pos_sum[b] = sp; r.neg_sum[b] = sn;
    r.n_active[b] = na; r.n_skipped[b] = ns;
}

bool contrast_shape_ok(int B, int K) { return B >= 1 && B <= 65535 && K >= 1; }
int contrast_blocks(int K) { return (K + kCtPerBlock - 1) / kCtPerBlock; }

}  // namespace

extern "C" {

size_t relpose_completion_loss_workspace_bytes(int32_t n_images, int32_t H, int32_t W, int32_t with_cross) {
    if (!loss_shape_ok(n_images, H, W)) return 0;
    return loss_layout(n_images, H, W, with_cross != 0).total;
}

int relpose_completion_loss(const RelposeCompletionLossArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeCompletionLossArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeCompletionLossArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeCompletionLossArgs)));
    if (!a.f || !a.complete || !a.mask || !a.sums || !a.ce_mag || !a.n_bad_label || !a.workspace) return RELPOSE_EINVAL;
    if (!loss_shape_ok(a.n_images, a.H, a.W) || a.n_classes < 1 || a.n_classes > 256 || a.total_channels < 7 + a.n_classes) return RELPOSE_EINVAL;
    if (((uintptr_t)a.f | (uintptr_t)a.complete | (uintptr_t)a.mask | (uintptr_t)a.weight) & 15) return RELPOSE_EINVAL;
    if (((uintptr_t)a.label & 3) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    const bool cross = a.ce_cross && a.label;
    const LossLayout l = loss_layout(a.n_images, a.H, a.W, cross);
    if (a.workspace_bytes < l.total) return RELPOSE_EINVAL;
    char* ws = (char*)a.workspace;
    LossBufs k{};
    k.N = a.n_images; k.Ct = a.total_channels; k.S = a.n_classes; k.HW = a.H * a.W;
    k.nblk = (k.HW / 4 + kLossThreads - 1) / kLossThreads;
    k.nblk2 = (k.HW + kCrossThreads - 1) / kCrossThreads;
    k.f = a.f; k.complete = a.complete; k.label = a.label; k.mask = a.mask; k.weight = a.weight;
    k.part = (double*)(ws + l.part);
    k.cross_part = cross ? (double*)(ws + l.cross_part) : nullptr;
    k.ce_map = cross ? (double*)(ws + l.ce_map) : nullptr;
    k.w_map = cross ? (float*)(ws + l.w_map) : nullptr;
    k.sums = a.sums; k.ce_mag = a.ce_mag; k.ce_cross = a.ce_cross; k.n_bad = a.n_bad_label;
    hipStream_t s = (hipStream_t)a.stream;
    hipLaunchKernelGGL(loss_kernel, dim3(k.nblk, k.N), dim3(kLossThreads), 0, s, k);
    RP_CHECK_LAUNCH();
    if (cross) {
        hipLaunchKernelGGL(loss_cross_kernel, dim3(k.nblk2), dim3(kCrossThreads), 0, s, k);
        RP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(loss_final_kernel, dim3(k.N + 1), dim3(64), 0, s, k);
    RP_CHECK_LAUNCH();
    return 0;
}

size_t relpose_contrast_loss_workspace_bytes(int32_t n_pairs, int32_t n_corres) {
    if (!contrast_shape_ok(n_pairs, n_corres)) return 0;
    const size_t n = (size_t)n_pairs * contrast_blocks(n_corres) * 2;
    return rp_align(n * sizeof(double)) + rp_align(n * sizeof(int));
}

int relpose_contrast_loss(const RelposeContrastLossArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeContrastLossArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeContrastLossArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeContrastLossArgs)));
    if (!a.f || !a.idx_src || !a.idx_tgt || !a.neg || !a.pos_sum || !a.neg_sum || !a.n_active || !a.n_skipped || !a.workspace) return RELPOSE_EINVAL;
    if (!contrast_shape_ok(a.n_pairs, a.n_corres) || a.h < 1 || a.h > 8192 || a.n_neg < 1) return RELPOSE_EINVAL;
    if (a.n_channels < 1 || a.n_channels > RELPOSE_DESC_MAX_CHANNELS || a.feat_off < 0 || a.total_channels < a.feat_off + a.n_channels) return RELPOSE_EINVAL;
    if ((long long)a.n_corres * a.n_neg > (1ll << 30) || !(a.margin == a.margin) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    if (a.workspace_bytes < relpose_contrast_loss_workspace_bytes(a.n_pairs, a.n_corres)) return RELPOSE_EINVAL;
    ContrastBufs r{};
    r.B = a.n_pairs; r.Ct = a.total_channels; r.off = a.feat_off; r.C = a.n_channels; r.h = a.h; r.K = a.n_corres; r.M = a.n_neg;
    r.nblk = contrast_blocks(a.n_corres);
    r.margin = a.margin;
    r.f = a.f; r.idx_src = a.idx_src; r.idx_tgt = a.idx_tgt; r.pair_valid = a.pair_valid; r.neg = a.neg;
    const size_t n = (size_t)r.B * r.nblk * 2;
    r.part_d = (double*)a.workspace;
    r.part_i = (int*)((char*)a.workspace + rp_align(n * sizeof(double)));
    r.pos_sum = a.pos_sum; r.neg_sum = a.neg_sum; r.n_active = a.n_active; r.n_skipped = a.n_skipped;
    hipStream_t s = (hipStream_t)a.stream;
    hipLaunchKernelGGL(contrast_kernel, dim3(r.nblk, r.B), dim3(kCtThreads), 0, s, r);
    RP_CHECK_LAUNCH();
    hipLaunchKernelGGL(contrast_final_kernel, dim3(r.B), dim3(64), 0, s, r);
    RP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
