// Visibility consistency of relative poses for a batch of directed (query cloud, reference view, pose) triples: every moved query point is
// projected into the reference view's depth panorama with relpose_frames_to_pano's rule (skybox.h) and compared with the depths the view measured
// around that pixel.  In front of them = the point stands in space the view saw through (violation); behind them = hidden (occluded); on
// them = consistent.  The contract is DESIGN.md §4.15 and the comment above relpose_visibility in include/relpose.h;
// tests/visibility_model.py restates it in numpy.  Built with -ffp-contract=off: every f64 operation is rounded on its own.
//
//   vis_window_kernel     one thread per panorama pixel, once per view however many queries name it: (dmin, dmax) of the valid depths in
//                         the (2r+1)^2 window around the pixel, clipped to the pixel's own face (columns) and to the map (rows), as one
//                         interleaved f32 pair; (0, 0) marks a pixel whose own depth is no data.  The <= 25 loads per thread are plain
//                         global loads: neighbouring lanes read neighbouring pixels, so all but the first touch of a line is a cache hit,
//                         and a view (400 KB at h = 160) is read from HBM once; no LDS tile (DESIGN.md §4.15 has the times).  Its
//                         first threads also clear the per-query counters.
//   vis_classify_kernel   256 query points per workgroup.  The point is moved (f64), projected (f64, four slots at most), its pixel's pair
//                         fetched with ONE 8-byte gather, and classified.  The class counts are reduced with ballots inside the wave and
//                         through LDS inside the workgroup, the fixed-point margins with integer shuffles; then one integer atomic per
//                         class per workgroup.  No float atomics: results are repeatable bit for bit.
// Every loop has a bound known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "skybox.h"

namespace {

constexpr int kTile = 256;                       // query points per workgroup, pixels per workgroup of the window pass
constexpr int kClasses = 6;
constexpr double kMaxDepth = 32768.0;            // a point at or beyond it is outside; a margin saturates at it: llrint(m 65536) <= 2^31

struct VisBufs {
    int n_clouds, P, n_views, h, nq, nblk, dataset, radius;
    double tol_abs, tol_rel;
    const double* pc;                            // [n_clouds, P, 3]
    const uint8_t* valid;                        // [n_clouds, P] or NULL
    const float* depth;                          // [n_views, h, 4h]
    const double* pose;                          // [nq, 4, 4]
    const int* qcloud;                           // [nq] device copies
    const int* rview;
    float2* win;                                 // [n_views, h, 4h] (dmin, dmax); workspace
    int* counts;                                 // [nq, 6]
    unsigned long long* margin_sum;              // [nq]
    uint8_t* cls;                                // [nq, P] or NULL
};

__device__ __forceinline__ bool depth_ok(float z) { return z > 0.0f && z <= FLT_MAX; }      // not 0, negative, NaN or inf

// ------------------------------------------------------------------------------------------------------- 1. one window image per view
__global__ __launch_bounds__(kTile) void vis_window_kernel(VisBufs b) {
    const size_t gid = (size_t)blockIdx.x * kTile + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * kTile;
    for (size_t e = gid; e < (size_t)b.nq * kClasses; e += nthreads) b.counts[e] = 0;
    for (size_t e = gid; e < (size_t)b.nq; e += nthreads) b.margin_sum[e] = 0ull;

    const int h = b.h, w = 4 * b.h, r = b.radius;
    const size_t total = (size_t)b.n_views * h * w;
    if (gid >= total) return;
    const unsigned g32 = (unsigned)gid;                              // total < 2^31 (sizes_ok): 32-bit divisions
    const int x = (int)(g32 % (unsigned)w), y = (int)((g32 / (unsigned)w) % (unsigned)h);
    const float* img = b.depth + (gid - (size_t)y * w - x);
    float2 o = make_float2(0.0f, 0.0f);
    if (depth_ok(img[(size_t)y * w + x])) {
        const int f0 = x / h * h;                                    // the first column of the pixel's face
        const int x0 = max(x - r, f0), x1 = min(x + r, f0 + h - 1), y0 = max(y - r, 0), y1 = min(y + r, h - 1);
        float lo = FLT_MAX, hi = 0.0f;
        for (int dy = -r; dy <= r; ++dy) {                          // bounds known at launch: r is an argument of the call
            for (int dx = -r; dx <= r; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= y0 && yy <= y1 && xx >= x0 && xx <= x1) {
                    const float z = img[(size_t)yy * w + xx];
                    if (depth_ok(z)) {
                        lo = fminf(lo, z);
                        hi = fmaxf(hi, z);
                    }
                }
            }
        }
        o = make_float2(lo, hi);
    }
    b.win[gid] = o;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------------- 2. classify every point
__global__ __launch_bounds__(kTile) void vis_classify_kernel(VisBufs b) {
    const int tid = threadIdx.x, lane = rp_lane(), wv = tid >> 6;
    const int q = blockIdx.x / b.nblk, blk = blockIdx.x - q * b.nblk;
    const int qc = b.qcloud[q], rv = b.rview[q];
    const int P = b.P, h = b.h;
    const int i = blk * kTile + tid;
    __shared__ int s_cnt[kTile / 64][kClasses];
    __shared__ unsigned long long s_margin[kTile / 64];

    int c = -1;                                                      // past the cloud: no class
    unsigned long long mfix = 0ull;
    if (i < P) {
        const size_t e = (size_t)qc * P + i;
        c = 0;
        if (!b.valid || b.valid[e]) {
            const double px = b.pc[3 * e], py = b.pc[3 * e + 1], pz = b.pc[3 * e + 2];
            const double* T = b.pose + (size_t)q * 16;
            const double q0 = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
            const double q1 = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
            const double q2 = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
            c = 1;
            int pix = -1, slot, cx, cy;
            double d = 0.0, zz;
            // relpose_frames_to_pano's projection (skybox.h): the first slot whose face takes the point
            if (isfinite(q0) && isfinite(q1) && isfinite(q2) && rp_skybox_project(b.dataset, h, q0, q1, q2, slot, cx, cy, zz)) {
                pix = cy * 4 * h + slot * h + cx;
                d = -zz;
            }
            if (pix >= 0 && d < kMaxDepth) {
                const float2 wn = b.win[(size_t)rv * h * 4 * h + pix];
                if (!(wn.x > 0.0f)) {
                    c = 2;
                } else {
                    const double dmin = (double)wn.x, dmax = (double)wn.y;
                    const double lo = dmin - (b.tol_abs + b.tol_rel * dmin);
                    const double hi = dmax + (b.tol_abs + b.tol_rel * dmax);
                    if (d < lo) {
                        c = 4;
                        mfix = (unsigned long long)llrint(fmin(lo - d, kMaxDepth) * 65536.0);
                    } else {
                        c = d > hi ? 5 : 3;
                    }
                }
            }
        }
        if (b.cls) b.cls[(size_t)q * P + i] = (uint8_t)c;
    }

#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
        const int n = __popcll(__ballot(c == k));
        if (lane == 0) s_cnt[wv][k] = n;
    }
    mfix = wave_sum_u64(mfix);
    if (lane == 0) s_margin[wv] = mfix;
    __syncthreads();
    if (tid < kClasses) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < kTile / 64; ++k) n += s_cnt[k][tid];
        if (n) atomicAdd(b.counts + (size_t)q * kClasses + tid, n);
    } else if (tid == 64) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int k = 0; k < kTile / 64; ++k) m += s_margin[k];
        if (m) atomicAdd(b.margin_sum + q, m);
    }
}

bool sizes_ok(long long n_views, long long h, long long nq) {
    if (n_views < 1 || nq < 1 || h < 2 || h > 8192 || (h & 1)) return false;
    return n_views * h * 4 * h < (1ll << 31);                        // pixel indices and the window pass's grid fit 31 bits
}

bool points_ok(long long n_clouds, long long P, long long nq) {
    if (n_clouds < 1 || P < 1 || P > (1ll << 24)) return false;
    return nq * ((P + kTile - 1) / kTile) < (1ll << 31);
}

// carve the workspace; returns the bytes used
size_t carve(VisBufs& k, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    k.win = (float2*)take((size_t)k.n_views * k.h * 4 * k.h * sizeof(float2));
    k.qcloud = (const int*)take((size_t)k.nq * sizeof(int));
    k.rview = (const int*)take((size_t)k.nq * sizeof(int));
    return off;
}

}  // namespace

extern "C" size_t relpose_visibility_workspace_bytes(int32_t n_views, int32_t h, int32_t n_queries) {
    if (!sizes_ok(n_views, h, n_queries)) return 0;
    VisBufs k{};
    k.n_views = n_views; k.h = h; k.nq = n_queries;
    return carve(k, nullptr);
}

extern "C" int relpose_visibility(const RelposeVisibilityArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeVisibilityArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeVisibilityArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeVisibilityArgs)));
    if (!a.pc || !a.depth || !a.query_cloud_host || !a.ref_view_host || !a.pose || !a.counts || !a.margin_sum || !a.workspace) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    if (a.radius < 0 || a.radius > 2) return RELPOSE_EINVAL;
    if (!std::isfinite(a.tol_abs) || !(a.tol_abs >= 0.0) || !std::isfinite(a.tol_rel) || !(a.tol_rel >= 0.0)) return RELPOSE_EINVAL;
    if (!sizes_ok(a.n_views, a.h, a.n_queries) || !points_ok(a.n_clouds, a.n_points, a.n_queries)) return RELPOSE_EINVAL;
    if (a.h < 2 * a.radius + 1) return RELPOSE_EINVAL;
    for (int q = 0; q < a.n_queries; ++q)
        if (a.query_cloud_host[q] < 0 || a.query_cloud_host[q] >= a.n_clouds || a.ref_view_host[q] < 0 || a.ref_view_host[q] >= a.n_views)
            return RELPOSE_EINVAL;
    VisBufs k{};
    k.n_clouds = a.n_clouds; k.P = a.n_points; k.n_views = a.n_views; k.h = a.h; k.nq = a.n_queries;
    k.nblk = (a.n_points + kTile - 1) / kTile;
    k.dataset = a.dataset; k.radius = a.radius;
    if (a.workspace_bytes < carve(k, nullptr) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve(k, (char*)a.workspace);
    k.tol_abs = a.tol_abs; k.tol_rel = a.tol_rel;
    k.pc = a.pc; k.valid = a.valid; k.depth = a.depth; k.pose = a.pose;
    k.counts = a.counts; k.margin_sum = (unsigned long long*)a.margin_sum; k.cls = a.cls;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.qcloud, a.query_cloud_host, (size_t)k.nq * sizeof(int), hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.rview, a.ref_view_host, (size_t)k.nq * sizeof(int), hipMemcpyHostToDevice, s));
    const size_t npix = (size_t)k.n_views * k.h * 4 * k.h;
    hipLaunchKernelGGL(vis_window_kernel, dim3((unsigned)((npix + kTile - 1) / kTile)), dim3(kTile), 0, s, k);
    hipLaunchKernelGGL(vis_classify_kernel, dim3((unsigned)((size_t)k.nq * k.nblk)), dim3(kTile), 0, s, k);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the two index arrays are the caller's again
    return 0;
}
