// SIFT descriptors of given keypoints, batched over views, and the exact rank count over them: the SIFT baseline of the descriptor metric
// (evalSiftDescriptor, mainPanoCompletion2view.py:353-381: cv2.xfeatures2d.SIFT_create().compute(gray, [cv2.KeyPoint(x, y, 5)]) on the
// correspondences and on a step-5 grid of the target, then the rank of the true match among the grid descriptors, :373-379).  The contract
// -- the project's own, written from Lowe (IJCV 60(2), 2004) with that call's parameters -- is DESIGN.md 4.10; tests/siftdesc_model.py
// implements it in numpy.  Compiled with -ffp-contract=off: the base blur rounds exactly like the float32 model (sift_model.blur).  The
// source image, its gray value and the border rule are sift_common.h's, shared with sift.hip.
//
// Launches (none of them depends on the number of views):
//   relpose_sift_describe   base image (gray + 13-tap blur, one LDS tile kernel), descriptors (one workgroup per keypoint slot)
//   relpose_sift_rank       thresholds (one lane per slot), counts (i8 MFMA tiles of 32 slots x 32 grid points)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>

#include "common.h"
#include "sift_common.h"

namespace {

constexpr int SD_R = 6;                 // 13 taps: round(8 sigma + 1) | 1 at sigma = sqrt(1.6^2 - 0.5^2)
constexpr int SD_TW = 64, SD_TH = 16;   // blur output tile
constexpr int SD_THREADS = 128;         // descriptor workgroup: one thread per output bin (4 x 4 x 8)
constexpr int SD_CAP = 2048;            // samples held in LDS at a time (whole raster rows of the keypoint's window)
constexpr int SD_MAX_SIDE = RELPOSE_SIFT_MAX_SIDE;

struct SdTaps {
    float t[2 * SD_R + 1];
};

// ------------------------------------------------------------------------------------------------------------------ base image
// base = blur(gray as float32): rows first, then columns, reflect-101 border, taps summed in index order.
__global__ __launch_bounds__(256) void siftdesc_base_kernel(SiftImage s, float* __restrict__ base, SdTaps tp) {
    __shared__ float tin[SD_TH + 2 * SD_R][SD_TW + 2 * SD_R];
    __shared__ float tmid[SD_TH + 2 * SD_R][SD_TW];
    const int v = blockIdx.z, H = s.h, W = s.w;
    const int x0 = blockIdx.x * SD_TW, y0 = blockIdx.y * SD_TH;
    constexpr int rows = SD_TH + 2 * SD_R, cols = SD_TW + 2 * SD_R;
    const uint8_t* im = s.img + v * s.vstride;
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        tin[ly][lx] = (float)sift_gray_at(s, im, sift_refl101(y0 + ly - SD_R, H), sift_refl101(x0 + lx - SD_R, W));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * SD_TW; i += 256) {
        const int ly = i / SD_TW, lx = i - ly * SD_TW;
        float acc = tp.t[0] * tin[ly][lx];
        for (int j = 1; j <= 2 * SD_R; ++j) acc = acc + tp.t[j] * tin[ly][lx + j];
        tmid[ly][lx] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SD_TH * SD_TW; i += 256) {
        const int ly = i / SD_TW, lx = i - ly * SD_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float acc = tp.t[0] * tmid[ly][lx];
        for (int j = 1; j <= 2 * SD_R; ++j) acc = acc + tp.t[j] * tmid[ly + j][lx];
        base[((long long)v * H + gy) * W + gx] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------------ descriptors
struct SdArgs {
    const float* base;          // [V, h, w]
    const float* kp;            // [V, n_kp, 4] (x, y, size, angle) or NULL: the grid
    const int* kp_count;        // [V] or NULL
    uint8_t* desc;              // [V, n_kp, 128]
    float* desc_f32;            // [V, n_kp, 128] or NULL
    int n_kp, h, w, grid_step, grid_nx, max_radius;
};

// One workgroup per keypoint slot, one thread per output bin.  The keypoint's window (its (2 radius + 1)^2 raster, cut to the pixels with
// all four neighbours inside the image) is taken in chunks of whole raster rows: phase 1, all lanes write (mag, rbin, cbin, obin) of every
// sample of the chunk to LDS at its raster position; phase 2, thread (row, col, o) walks the raster bounding box of its cell's rotated
// support inside the chunk, rows ascending, columns ascending, and adds mag * (1 - |rbin - row|) * (1 - |cbin - col|) * (1 - |obin - o| mod 8)
// for the samples where all three factors are positive -- the trilinear split of the contract seen from the receiving bin.  Every bin is
// summed by one thread in raster order: the order is fixed by the keypoint alone, and there are no atomics.
__global__ __launch_bounds__(SD_THREADS) void siftdesc_kernel(SdArgs a) {
    __shared__ float4 smp[SD_CAP];
    __shared__ float hist[128];
    const int v = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const long long slot = (long long)v * a.n_kp + k;
    float kx, ky, ksize, kangle;
    if (a.kp) {
        const float* q = a.kp + slot * 4;
        kx = q[0]; ky = q[1]; ksize = q[2]; kangle = q[3];
    } else {
        kx = (float)((k % a.grid_nx) * a.grid_step);
        ky = (float)((k / a.grid_nx) * a.grid_step);
        ksize = (float)a.grid_step;
        kangle = -1.f;
    }
    bool used = !(a.kp_count && k >= a.kp_count[v]);
    used = used && isfinite(kx) && isfinite(ky) && isfinite(ksize) && isfinite(kangle) && ksize > 0.f;
    const int h = a.h, w = a.w;
    int i0 = 0, i1 = -1, j0 = 0, j1 = -1, ptx = 0, pty = 0;
    float cos_t = 0.f, sin_t = 0.f, ang = 0.f, hw = 1.f;
    if (used) {
        // (positions beyond +-2^30 lie outside every image: clamped so that the integer arithmetic below cannot overflow)
        ptx = (int)fminf(fmaxf(rintf(kx), -1073741824.f), 1073741824.f);
        pty = (int)fminf(fmaxf(rintf(ky), -1073741824.f), 1073741824.f);
        ang = 360.f - kangle;
        if (ang >= 360.f) ang -= 360.f;
        const float s = ksize * 0.5f;
        hw = 3.f * s;
        const int radius = (int)fminf(rintf(hw * 1.4142135623730951f * 5.f * 0.5f), (float)a.max_radius);
        const float rad = ang * (float)(M_PI / 180.0);
        cos_t = cosf(rad) / hw;
        sin_t = sinf(rad) / hw;
        i0 = max(-radius, 1 - pty); i1 = min(radius, h - 2 - pty);
        j0 = max(-radius, 1 - ptx); j1 = min(radius, w - 2 - ptx);
    }
    const int Wd = j1 - j0 + 1, Hd = i1 - i0 + 1;
    float acc = 0.f;
    if (used && Wd > 0 && Hd > 0) {              // uniform over the workgroup
        const int rb = tid >> 5, cb = (tid >> 3) & 3, ob = tid & 7;
        // raster bounding box of the cell's support rbin in (rb - 1, rb + 1), cbin in (cb - 1, cb + 1):
        // j = hw (c_rot cos a + r_rot sin a), i = hw (r_rot cos a - c_rot sin a) at the four corners, widened by one sample.  The box only
        // limits the walk (a sample outside a cell's support has a non-positive factor), so it is clamped, not exact: hw to 1e6 (far
        // beyond any window) and the corners to +-(max_radius + 4), which contains the window.
        const float hwb = fminf(hw, 1e6f), cs = cosf(ang * (float)(M_PI / 180.0)), sn = sinf(ang * (float)(M_PI / 180.0));
        float bi0 = INFINITY, bi1 = -INFINITY, bj0 = INFINITY, bj1 = -INFINITY;
        for (int q = 0; q < 4; ++q) {
            const float rr = (float)rb - 2.5f + ((q & 1) ? 2.f : 0.f), cr = (float)cb - 2.5f + ((q & 2) ? 2.f : 0.f);
            const float fj = hwb * (cr * cs + rr * sn), fi = hwb * (rr * cs - cr * sn);
            bi0 = fminf(bi0, fi); bi1 = fmaxf(bi1, fi); bj0 = fminf(bj0, fj); bj1 = fmaxf(bj1, fj);
        }
        const float lim = (float)a.max_radius + 4.f;
        const int ci0 = max(i0, (int)fminf(fmaxf(floorf(bi0) - 1.f, -lim), lim)), ci1 = min(i1, (int)fmaxf(fminf(ceilf(bi1) + 1.f, lim), -lim));
        const int cj0 = max(j0, (int)fminf(fmaxf(floorf(bj0) - 1.f, -lim), lim)), cj1 = min(j1, (int)fmaxf(fminf(ceilf(bj1) + 1.f, lim), -lim));
        const float* im = a.base + (long long)v * h * w;
        const int rpc = max(1, SD_CAP / Wd);     // Wd <= w - 2 <= SD_CAP
        for (int ic = i0; ic <= i1; ic += rpc) {
            const int nrow = min(rpc, i1 - ic + 1), n = nrow * Wd;
            for (int p = tid; p < n; p += SD_THREADS) {
                const int li = p / Wd, lj = p - li * Wd;
                const int i = ic + li, j = j0 + lj;
                const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
                const float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
                float4 o = make_float4(0.f, -100.f, -100.f, 0.f);
                if (rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f) {
                    const float* q = im + (long long)(pty + i) * w + (ptx + j);
                    const float dx = q[1] - q[-1], dy = q[-w] - q[w];
                    const float mag = sqrtf(dx * dx + dy * dy) * expf(-(c_rot * c_rot + r_rot * r_rot) * 0.125f);
                    float ori = atan2f(dy, dx) * (float)(180.0 / M_PI);
                    if (ori < 0.f) ori += 360.f;
                    if (ori >= 360.f) ori -= 360.f;
                    o = make_float4(mag, rbin, cbin, (ori - ang) * (8.f / 360.f));
                }
                smp[p] = o;
            }
            __syncthreads();
            const int r0 = max(ci0, ic), r1 = min(ci1, ic + nrow - 1);
            for (int i = r0; i <= r1; ++i) {
                const float4* row = smp + (i - ic) * Wd - j0;
                for (int j = cj0; j <= cj1; ++j) {
                    const float4 sm = row[j];
                    const float wr = 1.f - fabsf(sm.y - (float)rb), wc = 1.f - fabsf(sm.z - (float)cb);
                    float d = sm.w - (float)ob;                  // obin in (-8, 8): d in (-15, 8)
                    d = d - 8.f * rintf(d * 0.125f);             // orientation bins are taken modulo 8
                    const float wo = 1.f - fabsf(d);
                    if (wr > 0.f && wc > 0.f && wo > 0.f) acc = acc + ((sm.x * wr) * wc) * wo;
                }
            }
            __syncthreads();                     // smp is rewritten by the next chunk
        }
    }
    hist[tid] = acc;
    __syncthreads();
    float n2 = 0.f;
    for (int q = 0; q < 128; ++q) n2 = n2 + hist[q] * hist[q];      // every thread the same index-order sum
    const float cap = 0.2f * sqrtf(n2);
    float m2 = 0.f;
    for (int q = 0; q < 128; ++q) { const float t = fminf(hist[q], cap); m2 = m2 + t * t; }
    const float u = fminf(acc, cap) * (512.f / fmaxf(sqrtf(m2), FLT_EPSILON));
    a.desc[slot * 128 + tid] = (uint8_t)fminf(fmaxf(rintf(u), 0.f), 255.f);
    if (a.desc_f32) a.desc_f32[slot * 128 + tid] = u;
}

// ------------------------------------------------------------------------------------------------------------------ rank
typedef int sd_v4i __attribute__((ext_vector_type(4)));
typedef int sd_v16i __attribute__((ext_vector_type(16)));

constexpr int RK_MT = 2;                // 32-slot tiles per workgroup (their A fragments stay in registers)
constexpr int RK_NT = 4;                // 32-point tiles per wave
constexpr int RK_WAVES = 4;
constexpr int RK_SLOTS = 32 * RK_MT, RK_POINTS = 32 * RK_NT * RK_WAVES;

struct RkArgs {
    const uint8_t* src;         // [B, E, 128]
    const uint8_t* tgt;         // [B, E, 128]
    const uint8_t* dense;       // [B, P, 128]
    const uint8_t* pair_valid;  // [B] or NULL
    int* thr;                   // [B, E]
    int* count;                 // [B, E]
    int B, E, P;
};

__global__ __launch_bounds__(256) void siftrank_prep_kernel(RkArgs r) {
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= r.E) return;
    const size_t o = (size_t)b * r.E + e;
    if (r.pair_valid && !r.pair_valid[b]) { r.thr[o] = -1; r.count[o] = -1; return; }
    const sd_v4i* s = (const sd_v4i*)(r.src + o * 128);
    const sd_v4i* t = (const sd_v4i*)(r.tgt + o * 128);
    int acc = 0;
    for (int q = 0; q < 8; ++q) {
        const sd_v4i x = s[q], y = t[q];
        for (int c = 0; c < 4; ++c)
            for (int sh = 0; sh < 32; sh += 8) {
                const int d = ((x[c] >> sh) & 255) - ((y[c] >> sh) & 255);
                acc += d * d;
            }
    }
    r.thr[o] = acc;
    r.count[o] = 0;
}

// sum of the squares of the 16 int8 in a fragment
__device__ inline int sd_sq16(sd_v4i x) {
    int s = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) s = __builtin_amdgcn_sdot4(x[c], x[c], s, false);      // v_dot4c_i32_i8
    return s;
}

// 16 descriptor bytes [32 s + 16 half, + 16) of a row, biased by -128 into int8 (x ^ 0x80 per byte): differences are unchanged
__device__ inline sd_v4i sd_frag(const uint8_t* row, int s, int half) {
    const sd_v4i x = *(const sd_v4i*)(row + 32 * s + 16 * half);
    const int m = (int)0x80808080u;
    return sd_v4i{x[0] ^ m, x[1] ^ m, x[2] ^ m, x[3] ^ m};
}

// count[b, e] += #{p in the workgroup's points : |a_e|^2 + |b_p|^2 - 2 a_e . b_p < thr[b, e]}, a = src - 128, b = dense - 128, the products
// on v_mfma_i32_32x32x32_i8.  Both operands are loaded alike -- lane half `hf` holds bytes [32 s + 16 hf, + 16) of k-step s of its A row
// (slot) and of its B column (point) -- so the dot product is right for any order of k inside the instruction.  C/D: column = lane & 31
// (point), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (slot).
__global__ __launch_bounds__(64 * RK_WAVES) void siftrank_count_kernel(RkArgs r) {
    __shared__ int s_cnt[RK_SLOTS];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hf = lane >> 5;
    if (r.pair_valid && !r.pair_valid[b]) return;          // uniform over the workgroup: before any barrier
    const int e0 = blockIdx.y * RK_SLOTS;
    if (tid < RK_SLOTS) s_cnt[tid] = 0;
    sd_v4i A[RK_MT][4];
    int trow[RK_MT][16];            // thr - |a|^2 of the slot behind accumulator register `reg` of this lane half; INT_MIN past E
    int cnt[RK_MT][16];
#pragma unroll
    for (int m = 0; m < RK_MT; ++m) {
        const int e = e0 + 32 * m + r32;
        const uint8_t* row = r.src + ((size_t)b * r.E + min(e, r.E - 1)) * 128;
        int na = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) { A[m][s] = sd_frag(row, s, hf); na += sd_sq16(A[m][s]); }
        na += __shfl_xor(na, 32, 64);
        const int t = e < r.E ? r.thr[(size_t)b * r.E + e] - na : INT_MIN;     // lane l and l + 32: slot e0 + 32 m + (l & 31)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            trow[m][g] = __shfl(t, (g & 3) + 8 * (g >> 2) + 4 * hf, 64);
            cnt[m][g] = 0;
        }
    }
    __syncthreads();
    const uint8_t* dn = r.dense + (size_t)b * r.P * 128;
    for (int t = 0; t < RK_NT; ++t) {
        const int p0 = (blockIdx.x * RK_NT * RK_WAVES + t * RK_WAVES + wave) * 32;
        if (p0 >= r.P) break;                              // uniform over the wave; no barrier inside the loop
        const int p = p0 + r32;
        const uint8_t* row = dn + (size_t)min(p, r.P - 1) * 128;
        sd_v4i Bf[4];
        int nb = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) { Bf[s] = sd_frag(row, s, hf); nb += sd_sq16(Bf[s]); }
        nb += __shfl_xor(nb, 32, 64);
        if (p >= r.P) nb = 0x3fffffff;                     // a padding column is never below a threshold
#pragma unroll
        for (int m = 0; m < RK_MT; ++m) {
            sd_v16i c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[m][s], Bf[s], c, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 16; ++g) cnt[m][g] += (nb - 2 * c[g] < trow[m][g]) ? 1 : 0;
        }
    }
#pragma unroll
    for (int m = 0; m < RK_MT; ++m)
#pragma unroll
        for (int g = 0; g < 16; ++g)
            if (cnt[m][g]) atomicAdd(&s_cnt[32 * m + (g & 3) + 8 * (g >> 2) + 4 * hf], cnt[m][g]);
    __syncthreads();
    if (tid < RK_SLOTS && e0 + tid < r.E && s_cnt[tid]) atomicAdd(r.count + (size_t)b * r.E + e0 + tid, s_cnt[tid]);
}

// ------------------------------------------------------------------------------------------------------------------ host
SdTaps g_sd_taps;
std::once_flag g_sd_taps_once;

void sd_init_taps() {
    const double sigma = std::sqrt(1.6 * 1.6 - 0.5 * 0.5);
    const int ks = (int)std::floor(sigma * 8.0 + 1.0 + 0.5) | 1;      // 13
    double w[2 * SD_R + 1], sum = 0.0;
    for (int i = 0; i < 2 * SD_R + 1; ++i) { const double x = i - ks / 2; w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma)); sum += w[i]; }
    for (int i = 0; i < 2 * SD_R + 1; ++i) g_sd_taps.t[i] = (float)(w[i] / sum);
}

bool sd_shape_ok(int V, int h, int w) { return V >= 1 && V <= 65535 && h >= 1 && w >= 1 && h <= SD_MAX_SIDE && w <= SD_MAX_SIDE; }

}  // namespace

extern "C" {

size_t relpose_sift_describe_workspace_bytes(int32_t n_views, int32_t h, int32_t w) {
    return sd_shape_ok(n_views, h, w) ? rp_align((size_t)n_views * h * w * sizeof(float)) : 0;
}

int relpose_sift_describe(const RelposeSiftDescArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeSiftDescArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeSiftDescArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeSiftDescArgs)));
    if (!a.images || (a.channels != 1 && a.channels != 3) || a.img_h <= 0 || a.img_w <= 0 || !sd_shape_ok(a.n_views, a.crop_h, a.crop_w) ||
        a.crop_x < 0 || a.crop_y < 0 || a.crop_x + a.crop_w > a.img_w || a.crop_y + a.crop_h > a.img_h)
        return RELPOSE_EINVAL;
    if (a.n_kp < 0 || a.grid_step < 0 || (a.n_kp > 0 && !a.desc) || (a.grid_step == 0 && a.n_kp > 0 && !a.kp)) return RELPOSE_EINVAL;
    if (((uintptr_t)a.kp & 3) || ((uintptr_t)a.desc_f32 & 3) || ((uintptr_t)a.base & 3) || ((uintptr_t)a.kp_count & 3)) return RELPOSE_EINVAL;
    int grid_nx = 0;
    if (a.grid_step > 0) {
        grid_nx = (a.crop_w + a.grid_step - 1) / a.grid_step;
        const long long n = (long long)grid_nx * ((a.crop_h + a.grid_step - 1) / a.grid_step);
        if (a.kp || a.kp_count || n != (long long)a.n_kp) return RELPOSE_EINVAL;
    }
    float* base = a.base;
    if (!base) {
        const size_t need = relpose_sift_describe_workspace_bytes(a.n_views, a.crop_h, a.crop_w);
        if (!a.workspace || ((uintptr_t)a.workspace & 3)) return RELPOSE_EINVAL;
        if (a.workspace_bytes < need) return RELPOSE_ENOMEM;
        base = (float*)a.workspace;
    }
    std::call_once(g_sd_taps_once, sd_init_taps);
    hipStream_t s = (hipStream_t)a.stream;
    const int V = a.n_views, h = a.crop_h, w = a.crop_w;
    SiftImage src{a.images, (long long)a.img_h * a.img_w * a.channels, a.img_w, a.channels, a.crop_x, a.crop_y, w, h};
    hipLaunchKernelGGL(siftdesc_base_kernel, dim3((w + SD_TW - 1) / SD_TW, (h + SD_TH - 1) / SD_TH, V), dim3(256), 0, s, src, base, g_sd_taps);
    RP_CHECK_LAUNCH();
    if (a.n_kp > 0) {
        SdArgs d{};
        d.base = base; d.kp = a.kp; d.kp_count = a.kp_count; d.desc = a.desc; d.desc_f32 = a.desc_f32;
        d.n_kp = a.n_kp; d.h = h; d.w = w; d.grid_step = a.grid_step; d.grid_nx = grid_nx;
        d.max_radius = (int)std::sqrt((double)w * w + (double)h * h);
        hipLaunchKernelGGL(siftdesc_kernel, dim3(a.n_kp, V), dim3(SD_THREADS), 0, s, d);
        RP_CHECK_LAUNCH();
    }
    return 0;
}

int relpose_sift_rank(const RelposeSiftRankArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeSiftRankArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeSiftRankArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeSiftRankArgs)));
    if (!a.src || !a.tgt || !a.dense || !a.thr || !a.count) return RELPOSE_EINVAL;
    if (((uintptr_t)a.src & 15) || ((uintptr_t)a.tgt & 15) || ((uintptr_t)a.dense & 15) || ((uintptr_t)a.thr & 3) || ((uintptr_t)a.count & 3))
        return RELPOSE_EINVAL;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.n_slots < 1 || a.n_slots > (1 << 21) || a.n_points < 1 || a.n_points > (1 << 28)) return RELPOSE_EINVAL;
    RkArgs r{a.src, a.tgt, a.dense, a.pair_valid, a.thr, a.count, a.n_pairs, a.n_slots, a.n_points};
    hipStream_t s = (hipStream_t)a.stream;
    hipLaunchKernelGGL(siftrank_prep_kernel, dim3((r.E + 255) / 256, r.B), dim3(256), 0, s, r);
    RP_CHECK_LAUNCH();
    hipLaunchKernelGGL(siftrank_count_kernel, dim3((r.P + RK_POINTS - 1) / RK_POINTS, (r.E + RK_SLOTS - 1) / RK_SLOTS, r.B), dim3(64 * RK_WAVES), 0, s, r);
    RP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
