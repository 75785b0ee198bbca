// Frame-to-model alignment of depth panoramas to TSDF volumes (the contract stands above relpose_tsdf_align in
// include/relpose.h, tests/align_model.py restates it in numpy).  Built with -ffp-contract=off: every f64 operation is rounded on its own.
// Nothing is accumulated across points but integers, so the sums do not depend on the order, on the block decomposition or on the batch.
//
//   align_accumulate_kernel   grid (view, chunk of kChunk sampled pixels), 256 threads.  The view's pose is read once per workgroup and
//                             inverted through LDS; each thread unprojects kChunk / 256 pixels (consecutive lanes take consecutive pixels: the
//                             depth loads coalesce and the gathers of a wave fall on neighbouring cells), classifies them, gathers the 8
//                             corners and adds the 28 integer products and its class count to 32 int64 registers.  The 32 sums are reduced
//                             across the wave by shuffles, across the four waves through LDS, and stored as one slab per workgroup.
//   align_step_kernel         one wave per view: lanes 0..31 each sum one of the 32 values over the view's slabs in ascending order; lane 0
//                             then runs tsdfalign_math.h's step (Jacobi, floor, Cayley update) and writes the pose of the next evaluation, the
//                             trace row and, at the last evaluation, the outputs.
// iters + 1 evaluations, two launches each, whatever the number of views; no atomics.  Every loop has a bound known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "skybox.h"
#include "tsdf_surf.h"
#include "tsdfalign_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kChunk = kThreads * kPerThread;     // sampled pixels per workgroup
constexpr int kMaxIters = 64;
constexpr int kMaxDim = 2048;                     // |lever arm| <= 1024 voxels: see the overflow bound in include/relpose.h
constexpr long long kMaxPoints = 1ll << 22;       // sampled pixels per view

struct AlignBufs {
    int h, dataset, nx, ny, nz, min_weight, stride, iters;
    unsigned npts, nblk, nvox;                    // sampled pixels per view, workgroups per view, voxels per scene
    double voxel, eig_min;
    const float* depth;                           // [V, h, 4h]
    const int* tsdf;                              // [S, nz, ny, nx]
    const int* weight;
    const double* origin;                         // [S, 3] device copy
    const int* scene_of_view;                     // [V] device copy
    long long* slabs;                             // [V, nblk, 32]
    double* pose_out;                             // [V, 4, 4]
    double* eig;                                  // [V, 6]
    int* held;                                    // [V]
    long long* sums;                              // [V, 32]
    double* rms;                                  // [V, 2]
    double* trace_pose;                           // [V, iters + 1, 4, 4] or NULL
    long long* trace_sums;                        // [V, iters + 1, 32] or NULL
};

__device__ __forceinline__ bool depth_ok(float z) { return z > 0.0f && z <= FLT_MAX; }      // not 0, negative, NaN or inf

__device__ __forceinline__ AlignVolume volume_of(const AlignBufs& b, int s) {
    AlignVolume g;
    g.nx = b.nx; g.ny = b.ny; g.nz = b.nz; g.min_weight = b.min_weight;
    g.voxel = b.voxel;
    const int n[3] = {b.nx, b.ny, b.nz};
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = b.origin[3 * s + a];
        g.centre[a] = g.origin[a] + ((double)n[a] * 0.5) * b.voxel;
    }
    g.tsdf = b.tsdf + (size_t)s * b.nvox;
    g.weight = b.weight + (size_t)s * b.nvox;
    return g;
}

__device__ __forceinline__ long long shfl_xor_ll(long long v, int m) {
    int lo = (int)(v & 0xffffffffll), hi = (int)(v >> 32);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}

// ------------------------------------------------------------------------------------------------------- 1. accumulate
__global__ __launch_bounds__(kThreads) void align_accumulate_kernel(AlignBufs b, const double* pose) {
    __shared__ double s_W[12];
    __shared__ long long s_red[kThreads / RP_WAVE][kAlignSums];
    const int tid = threadIdx.x;
    const unsigned v = blockIdx.x / b.nblk, blk = blockIdx.x - v * b.nblk;
    if (tid == 0) {
        double T[12];
        for (int e = 0; e < 12; ++e) T[e] = pose[(size_t)v * 16 + e];
        align_inverse(T, s_W);
    }
    __syncthreads();
    double W[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) W[e] = s_W[e];
    const AlignVolume g = volume_of(b, b.scene_of_view[v]);
    const int h = b.h;
    const size_t npix = (size_t)h * 4 * h;
    const float* depth = b.depth + (size_t)v * npix;
    long long sums[kAlignSums];
#pragma unroll
    for (int e = 0; e < kAlignSums; ++e) sums[e] = 0;
#pragma unroll 1
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned idx = blk * kChunk + k * kThreads + tid;      // npts <= 2^22: no wrap
        if (idx < b.npts) {
            const unsigned pix = idx * (unsigned)b.stride;           // < 4 h^2 < 2^31
            const float zf = depth[pix];
            if (depth_ok(zf)) {
                const unsigned row = pix / (4u * h), col = pix - row * (4u * h), slot = col / (unsigned)h, px = col - slot * h;
                const double D = (double)zf;
                const double xn = (2.0 * (double)px) / (double)h - 1.0;
                const double yn = 1.0 - (2.0 * (double)row) / (double)h;
                double x, y, z;
                rp_face_rot(rp_face_index(b.dataset, (int)slot), xn * D, yn * D, -D, x, y, z);
                long long Jq[6], rq;
                const int cls = align_row(g, W, x, y, z, Jq, rq);
                if (cls == kAlignUsed) align_add_row(sums, Jq, rq);
#pragma unroll
                for (int c = kAlignOutside; c <= kAlignUsed; ++c) sums[c] += cls == c;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kAlignSums; ++e) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sums[e] += shfl_xor_ll(sums[e], m);
    }
    if (rp_lane() == 0) {
#pragma unroll
        for (int e = 0; e < kAlignSums; ++e) s_red[tid >> 6][e] = sums[e];
    }
    __syncthreads();
    if (tid < kAlignSums) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < kThreads / RP_WAVE; ++w) t += s_red[w][tid];
        b.slabs[((size_t)v * b.nblk + blk) * kAlignSums + tid] = t;
    }
}

// ------------------------------------------------------------------------------------------------------- 2. step
__global__ __launch_bounds__(RP_WAVE) void align_step_kernel(AlignBufs b, const double* pose, int e) {
    __shared__ long long s_sums[kAlignSums];
    const unsigned v = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < kAlignSums) {
        const long long* slab = b.slabs + (size_t)v * b.nblk * kAlignSums + tid;
        long long t = 0;
        for (unsigned k = 0; k < b.nblk; ++k) t += slab[(size_t)k * kAlignSums];     // nblk is the call's
        s_sums[tid] = t;
        if (b.trace_sums) b.trace_sums[((size_t)v * (b.iters + 1) + e) * kAlignSums + tid] = t;
        if (e == b.iters) b.sums[(size_t)v * kAlignSums + tid] = t;
    }
    __syncthreads();
    if (tid != 0) return;
    const AlignVolume g = volume_of(b, b.scene_of_view[v]);
    double T[16], Tn[16], eig[6];
    for (int i = 0; i < 16; ++i) T[i] = pose[(size_t)v * 16 + i];
    int held;
    align_step(s_sums, T, g, b.eig_min, e < b.iters, Tn, eig, held);
    for (int i = 0; i < 16; ++i) b.pose_out[(size_t)v * 16 + i] = Tn[i];
    if (b.trace_pose)
        for (int i = 0; i < 16; ++i) b.trace_pose[((size_t)v * (b.iters + 1) + e) * 16 + i] = T[i];
    if (e == 0) b.rms[2 * v] = align_rms(s_sums);
    if (e == b.iters) {
        b.rms[2 * v + 1] = align_rms(s_sums);
        for (int i = 0; i < 6; ++i) b.eig[6 * v + i] = eig[i];
        b.held[v] = held;
    }
}

// ------------------------------------------------------------------------------------------------------- host
bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

long long points_of(long long h, long long stride) { return (4 * h * h + stride - 1) / stride; }

bool shapes_ok(long long S, long long V, long long h, long long nx, long long ny, long long nz, long long stride) {
    if (!tsdf_volume_ok(S, nx, ny, nz) || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim) return false;
    if (V < 1 || h < 2 || h > 8192 || (h & 1) || V * h * 4 * h >= (1ll << 31) || stride < 1) return false;
    const long long npts = points_of(h, stride);
    return npts <= kMaxPoints && V * ((npts + kChunk - 1) / kChunk) < (1ll << 31);
}

size_t carve(int S, int V, unsigned nblk, char* base, long long*& slabs, const double*& origin, const int*& sov) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    origin = (const double*)take((size_t)S * 3 * sizeof(double));
    sov = (const int*)take((size_t)V * sizeof(int));
    slabs = (long long*)take((size_t)V * nblk * kAlignSums * sizeof(long long));
    return off;
}

}  // namespace

extern "C" size_t relpose_tsdf_align_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz, int32_t stride) {
    if (!shapes_ok(n_scenes, n_views, h, nx, ny, nz, stride)) return 0;
    long long* slabs;
    const double* org;
    const int* sov;
    return carve(n_scenes, n_views, (unsigned)((points_of(h, stride) + kChunk - 1) / kChunk), nullptr, slabs, org, sov);
}

extern "C" int relpose_tsdf_align(const RelposeTsdfAlignArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeTsdfAlignArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeTsdfAlignArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeTsdfAlignArgs)));
    if (!a.tsdf_sum || !a.weight || !a.depth || !a.pose || !a.origin_host || !a.scene_of_view_host || !a.workspace) return RELPOSE_EINVAL;
    if (!a.pose_out || !a.eig || !a.held || !a.sums || !a.rms) return RELPOSE_EINVAL;
    if ((a.trace_pose == nullptr) != (a.trace_sums == nullptr)) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    if (a.reserved0 != 0 || a.min_weight < 1 || a.iters < 0 || a.iters > kMaxIters) return RELPOSE_EINVAL;
    if (!finite_pos(a.voxel) || !std::isfinite(a.eig_min) || a.eig_min < 0.0) return RELPOSE_EINVAL;
    if (!shapes_ok(a.n_scenes, a.n_views, a.h, a.nx, a.ny, a.nz, a.stride)) return RELPOSE_EINVAL;
    for (int v = 0; v < a.n_views; ++v)
        if (a.scene_of_view_host[v] < 0 || a.scene_of_view_host[v] >= a.n_scenes) return RELPOSE_EINVAL;
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    AlignBufs k{};
    k.npts = (unsigned)points_of(a.h, a.stride);
    k.nblk = (k.npts + kChunk - 1) / kChunk;
    if (a.workspace_bytes < carve(a.n_scenes, a.n_views, k.nblk, nullptr, k.slabs, k.origin, k.scene_of_view) || ((uintptr_t)a.workspace & 255))
        return RELPOSE_EINVAL;
    carve(a.n_scenes, a.n_views, k.nblk, (char*)a.workspace, k.slabs, k.origin, k.scene_of_view);
    k.h = a.h; k.dataset = a.dataset; k.nx = a.nx; k.ny = a.ny; k.nz = a.nz; k.min_weight = a.min_weight; k.stride = a.stride; k.iters = a.iters;
    k.nvox = (unsigned)((long long)a.nx * a.ny * a.nz);
    k.voxel = a.voxel; k.eig_min = a.eig_min;
    k.depth = a.depth; k.tsdf = a.tsdf_sum; k.weight = a.weight;
    k.pose_out = a.pose_out; k.eig = a.eig; k.held = a.held; k.sums = (long long*)a.sums; k.rms = a.rms;
    k.trace_pose = a.trace_pose; k.trace_sums = (long long*)a.trace_sums;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.origin, a.origin_host, (size_t)a.n_scenes * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.scene_of_view, a.scene_of_view_host, (size_t)a.n_views * sizeof(int), hipMemcpyHostToDevice, s));
    for (int e = 0; e <= a.iters; ++e) {
        const double* cur = e == 0 ? a.pose : a.pose_out;            // the step writes the next evaluation's pose to pose_out
        hipLaunchKernelGGL(align_accumulate_kernel, dim3((unsigned)a.n_views * k.nblk), dim3(kThreads), 0, s, k, cur);
        hipLaunchKernelGGL(align_step_kernel, dim3((unsigned)a.n_views), dim3(RP_WAVE), 0, s, k, cur, e);
    }
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the two host arrays are the caller's again
    return 0;
}
