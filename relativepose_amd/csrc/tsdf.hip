// TSDF fusion of posed depth panoramas and the surface of the fused volume (the contract stands above relpose_tsdf_fuse and
// relpose_tsdf_surface in include/relpose.h, tests/tsdf_model.py restates it in numpy).  Built with -ffp-contract=off: every f64 operation
// is rounded on its own.  Everything that is accumulated is an integer, and every voxel is owned by one thread: no atomics, the volume
// does not depend on the order of the views, and a scene's result does not depend on the batch around it.
//
//   tsdf_fuse_kernel      one thread per voxel, a workgroup = 256 consecutive voxels of one scene in the x-fastest order: the lanes of a
//                         wave are neighbours in x (a row's end continues in the next row, so no lane idles whatever nx is), the two or
//                         three stores coalesce and a wave's depth gathers fall on neighbouring pixels.  The scene's poses (three rows
//                         each) are staged through LDS in chunks of kChunk views; every lane reads the same LDS word (a broadcast).  Per
//                         view: move (f64), project (skybox.h, four slots at most), one 4-byte gather, the integer update in registers.
//   tsdf_count_kernel     256 voxels per workgroup: the crossings of every voxel with its three positive-axis neighbours (0..3), summed
//                         over the workgroup.
//   tsdf_scan_kernel      one workgroup per scene: the exclusive scan of the workgroups' counts in place, and the scene's total.
//   tsdf_write_kernel     the count pass again, an ordered scan inside the workgroup, and the points, normals and colours of the first
//                         `cap` crossings; its threads also write `valid`.
// The surface's device code (a voxel's value and gradient, its crossings, the scan and the write body) stands in tsdf_surf.h, which
// mesh.hip shares: relpose_tsdf_mesh's vertices are this cloud bit for bit.
// Every loop has a bound known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "cloud_prims.h"
#include "common.h"
#include "skybox.h"
#include "tsdf_surf.h"

namespace {

constexpr int kTile = kTsdfTile;                 // voxels per workgroup
constexpr int kChunk = 32;                       // views whose poses are in LDS at a time
constexpr int kScanThreads = kTsdfScanThreads;
constexpr int kMaxViews = 4096;                  // per scene per call: 4096 * 32768 = 2^27 fits the int a thread sums in
constexpr double kMaxDepth = 32768.0;            // visibility.hip's: a voxel at or beyond it is outside the view
constexpr double kFix = kTsdfFix;

struct FuseBufs {
    int h, dataset, nx, ny, accumulate;
    unsigned nvox, nblk;                         // voxels and workgroups per scene
    double voxel, trunc;
    const float* depth;                          // [V, h, 4h]
    const float* rgb;                            // [V, 3, h, 4h] or NULL
    const double* pose;                          // [V, 4, 4]
    const int* view_begin;                       // [S + 1] device copy
    const double* origin;                        // [S, 3] device copy
    int* tsdf;                                   // [S, nz, ny, nx]
    int* weight;
    unsigned* color;                             // [S, 3, nz, ny, nx] or NULL
};

__device__ __forceinline__ bool depth_ok(float z) { return z > 0.0f && z <= FLT_MAX; }      // not 0, negative, NaN or inf

// ------------------------------------------------------------------------------------------------------- 1. integrate
__global__ __launch_bounds__(kTile) void tsdf_fuse_kernel(FuseBufs b) {
    __shared__ double s_pose[kChunk * 12];
    const int tid = threadIdx.x;
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const unsigned e = blk * kTile + tid;                            // nvox < 2^31: no wrap
    const bool in = e < b.nvox;
    const unsigned i = e % (unsigned)b.nx, r = e / (unsigned)b.nx, j = r % (unsigned)b.ny, k = r / (unsigned)b.ny;
    const double cx = b.origin[3 * s] + ((double)i + 0.5) * b.voxel;
    const double cy = b.origin[3 * s + 1] + ((double)j + 0.5) * b.voxel;
    const double cz = b.origin[3 * s + 2] + ((double)k + 0.5) * b.voxel;
    const int v0 = b.view_begin[s], v1 = b.view_begin[s + 1];
    const int h = b.h;
    const size_t npix = (size_t)h * 4 * h;
    int ts = 0, w = 0;
    unsigned c0 = 0, c1 = 0, c2 = 0;
    for (int vb = v0; vb < v1; vb += kChunk) {                       // v0, v1 are the call's arguments
        const int n = min(kChunk, v1 - vb);
        __syncthreads();                                             // the previous chunk has been read
        for (int x = tid; x < n * 12; x += kTile) s_pose[x] = b.pose[(size_t)(vb + x / 12) * 16 + x % 12];
        __syncthreads();
        if (in) {
            for (int u = 0; u < n; ++u) {
                const double* T = s_pose + u * 12;
                const double q0 = ((T[0] * cx + T[1] * cy) + T[2] * cz) + T[3];
                const double q1 = ((T[4] * cx + T[5] * cy) + T[6] * cz) + T[7];
                const double q2 = ((T[8] * cx + T[9] * cy) + T[10] * cz) + T[11];
                int slot, px, py;
                double zz;
                if (isfinite(q0) && isfinite(q1) && isfinite(q2) && rp_skybox_project(b.dataset, h, q0, q1, q2, slot, px, py, zz)) {
                    const double d = -zz;
                    const size_t pix = (size_t)py * 4 * h + (size_t)slot * h + px;
                    if (d < kMaxDepth) {
                        const float z = b.depth[(size_t)(vb + u) * npix + pix];
                        if (depth_ok(z)) {
                            const double sdf = (double)z - d;
                            if (!(sdf < -b.trunc)) {
                                const double t = fmin(sdf / b.trunc, 1.0);
                                ts += (int)llrint(t * kFix);
                                w += 1;
                                if (b.rgb) {
                                    const float* c = b.rgb + (size_t)(vb + u) * 3 * npix + pix;
                                    c0 += (unsigned)rintf(fminf(fmaxf(c[0], 0.0f), 1.0f) * 255.0f);
                                    c1 += (unsigned)rintf(fminf(fmaxf(c[npix], 0.0f), 1.0f) * 255.0f);
                                    c2 += (unsigned)rintf(fminf(fmaxf(c[2 * npix], 0.0f), 1.0f) * 255.0f);
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (in) {
        const size_t o = (size_t)s * b.nvox + e;
        const size_t oc = (size_t)s * 3 * b.nvox + e;
        if (b.accumulate) {
            b.tsdf[o] += ts;
            b.weight[o] += w;
            if (b.color) {
                b.color[oc] += c0;
                b.color[oc + b.nvox] += c1;
                b.color[oc + 2 * (size_t)b.nvox] += c2;
            }
        } else {
            b.tsdf[o] = ts;
            b.weight[o] = w;
            if (b.color) {
                b.color[oc] = c0;
                b.color[oc + b.nvox] = c1;
                b.color[oc + 2 * (size_t)b.nvox] = c2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- 2. surface
__global__ __launch_bounds__(kTile) void tsdf_count_kernel(SurfBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const unsigned e = blk * kTile + threadIdx.x;
    const unsigned i = e % (unsigned)b.nx, r = e / (unsigned)b.nx, j = r % (unsigned)b.ny, k = r / (unsigned)b.ny;
    double ta, tb[3];
    const int mask = tsdf_crossings(b, (size_t)s * b.nvox, e < b.nvox, (int)i, (int)j, (int)k, ta, tb);
    int total;
    rp_block_excl_scan(__popc(mask), s_wsum, total);
    if (threadIdx.x == 0) b.blk[(size_t)s * b.nblk + blk] = total;
}

__global__ __launch_bounds__(kScanThreads) void tsdf_scan_kernel(SurfBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int run = tsdf_scan_counts(b.blk + (size_t)s * b.nblk, b.nblk, s_wsum);
    if (threadIdx.x == 0) b.n_points[s] = run;                       // <= 3 nvox < 2^31
}

__global__ __launch_bounds__(kTile) void tsdf_write_kernel(SurfBufs b) {
    __shared__ int s_wsum[16];
    int first;
    tsdf_write_body(b, s_wsum, first);
}

// ------------------------------------------------------------------------------------------------------- host
bool views_ok(long long V, long long h) {
    if (V < 1 || h < 2 || h > 8192 || (h & 1)) return false;
    return V * h * 4 * h < (1ll << 31);
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

size_t carve_fuse(int S, char* base, const int*& view_begin, const double*& origin) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    origin = (const double*)take((size_t)S * 3 * sizeof(double));
    view_begin = (const int*)take(((size_t)S + 1) * sizeof(int));
    return off;
}

size_t carve_surface(int S, unsigned nblk, char* base, int*& blk, const double*& origin) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    origin = (const double*)take((size_t)S * 3 * sizeof(double));
    blk = (int*)take((size_t)S * nblk * sizeof(int));
    return off;
}

}  // namespace

extern "C" size_t relpose_tsdf_fuse_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz) {
    if (!tsdf_volume_ok(n_scenes, nx, ny, nz) || !views_ok(n_views, h)) return 0;
    const int* vb;
    const double* org;
    return carve_fuse(n_scenes, nullptr, vb, org);
}

extern "C" int relpose_tsdf_fuse(const RelposeTsdfFuseArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeTsdfFuseArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeTsdfFuseArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeTsdfFuseArgs)));
    if (!a.depth || !a.pose || !a.view_begin_host || !a.origin_host || !a.tsdf_sum || !a.weight || !a.workspace) return RELPOSE_EINVAL;
    if ((a.rgb == nullptr) != (a.color_sum == nullptr)) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    if ((a.accumulate != 0 && a.accumulate != 1) || a.reserved0 != 0) return RELPOSE_EINVAL;
    if (!finite_pos(a.voxel) || !finite_pos(a.trunc)) return RELPOSE_EINVAL;
    if (!tsdf_volume_ok(a.n_scenes, a.nx, a.ny, a.nz) || !views_ok(a.n_views, a.h)) return RELPOSE_EINVAL;
    if (a.view_begin_host[0] != 0 || a.view_begin_host[a.n_scenes] != a.n_views) return RELPOSE_EINVAL;
    for (int s = 0; s < a.n_scenes; ++s) {
        const long long n = (long long)a.view_begin_host[s + 1] - a.view_begin_host[s];
        if (n < 0 || n > kMaxViews) return RELPOSE_EINVAL;
    }
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    FuseBufs k{};
    if (a.workspace_bytes < carve_fuse(a.n_scenes, nullptr, k.view_begin, k.origin) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_fuse(a.n_scenes, (char*)a.workspace, k.view_begin, k.origin);
    k.h = a.h; k.dataset = a.dataset; k.nx = a.nx; k.ny = a.ny; k.accumulate = a.accumulate;
    k.nvox = (unsigned)((long long)a.nx * a.ny * a.nz);
    k.nblk = tsdf_blocks_of(k.nvox);
    k.voxel = a.voxel; k.trunc = a.trunc;
    k.depth = a.depth; k.rgb = a.rgb; k.pose = a.pose;
    k.tsdf = a.tsdf_sum; k.weight = a.weight; k.color = a.color_sum;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.origin, a.origin_host, (size_t)a.n_scenes * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.view_begin, a.view_begin_host, ((size_t)a.n_scenes + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(tsdf_fuse_kernel, dim3((unsigned)a.n_scenes * k.nblk), dim3(kTile), 0, s, k);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the two host arrays are the caller's again
    return 0;
}

extern "C" size_t relpose_tsdf_surface_workspace_bytes(int32_t n_scenes, int32_t nx, int32_t ny, int32_t nz) {
    if (!tsdf_volume_ok(n_scenes, nx, ny, nz) || 3ll * nx * ny * nz >= (1ll << 31)) return 0;
    int* blk;
    const double* org;
    return carve_surface(n_scenes, tsdf_blocks_of((long long)nx * ny * nz), nullptr, blk, org);
}

extern "C" int relpose_tsdf_surface(const RelposeTsdfSurfaceArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeTsdfSurfaceArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeTsdfSurfaceArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeTsdfSurfaceArgs)));
    if (!a.tsdf_sum || !a.weight || !a.origin_host || !a.points || !a.normals || !a.valid || !a.n_points || !a.workspace) return RELPOSE_EINVAL;
    if (a.colors && !a.color_sum) return RELPOSE_EINVAL;
    if (a.min_weight < 1 || a.cap < 1 || a.reserved0 != 0 || !finite_pos(a.voxel)) return RELPOSE_EINVAL;
    if (!tsdf_volume_ok(a.n_scenes, a.nx, a.ny, a.nz) || 3ll * a.nx * a.ny * a.nz >= (1ll << 31)) return RELPOSE_EINVAL;
    if ((long long)a.n_scenes * a.cap >= (1ll << 29)) return RELPOSE_EINVAL;
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    SurfBufs k{};
    k.nvox = (unsigned)((long long)a.nx * a.ny * a.nz);
    k.nblk = tsdf_blocks_of(k.nvox);
    if (a.workspace_bytes < carve_surface(a.n_scenes, k.nblk, nullptr, k.blk, k.origin) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_surface(a.n_scenes, k.nblk, (char*)a.workspace, k.blk, k.origin);
    k.nx = a.nx; k.ny = a.ny; k.nz = a.nz; k.min_weight = a.min_weight; k.cap = a.cap;
    k.voxel = a.voxel;
    k.tsdf = a.tsdf_sum; k.weight = a.weight; k.color = a.color_sum;
    k.points = a.points; k.normals = a.normals; k.colors = a.colors; k.valid = a.valid; k.n_points = a.n_points;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.origin, a.origin_host, (size_t)a.n_scenes * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    const unsigned grid = (unsigned)a.n_scenes * k.nblk;
    hipLaunchKernelGGL(tsdf_count_kernel, dim3(grid), dim3(kTile), 0, s, k);
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3((unsigned)a.n_scenes), dim3(kScanThreads), 0, s, k);
    hipLaunchKernelGGL(tsdf_write_kernel, dim3(grid), dim3(kTile), 0, s, k);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the host origin is the caller's again
    return 0;
}
