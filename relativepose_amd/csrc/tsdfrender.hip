// Depth, normal and colour panoramas rendered from TSDF volumes (the contract stands above relpose_tsdf_render in
// include/relpose.h, tests/render_model.py restates it in numpy).  Built with -ffp-contract=off: every f64 operation is rounded on its own.
// A pixel's outputs depend on its own ray and the volume alone: nothing is shared between pixels, no atomics, no dependence on the batch.
//
//   render_flag_kernel   (skip = 1) grid (scene, 256 voxels): a known voxel with tsdf_sum < 0 stores 1 to the brick of each of the up to 8
//                        cells it is a corner of.  Many threads may store the same 1: plain byte stores into a zeroed array.
//   render_kernel        grid (view, 256 consecutive pixels of the panorama in row-major order), one thread per pixel: the 64 lanes of a wave are
//                        neighbouring columns of one row (adjacent slots are adjacent cube faces, so the rays stay neighbours across a slot
//                        boundary) and their gathers fall on neighbouring cells.  The pose is read once per workgroup and inverted through
//                        LDS.  Each thread clips its ray against the box and runs tsdfrender_math.h's march: one cell lookup (and, with
//                        skip, one flag byte) per sample, the sixteen corner loads of an evaluation issued together, one carried value.
//                        A hit evaluates its two samples again with gradient and colour, after the loop, so the loop does not hold them
//                        in registers (120 VGPRs, 4 waves per SIMD).  Measured: bound by float64 VALU issue, not by the gathers (§4.20).
// Every loop has a bound known at launch (n_steps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "tsdf_surf.h"
#include "tsdfrender_math.h"

namespace {

constexpr int kThreads = 256;

struct RenderBufs {
    int h, suncg, nx, ny, nz, min_weight, n_steps, skip;
    int bx, by, bz;
    unsigned nblk, nvox, nbrick;                  // workgroups per view, voxels and bricks per scene
    double voxel, d_min, step;
    const int* tsdf;                              // [S, nz, ny, nx]
    const int* weight;
    const unsigned* color;                        // [S, 3, nz, ny, nx] or NULL
    const double* pose;                           // [V, 4, 4]
    const double* origin;                         // [S, 3] device copy
    const int* scene_of_view;                     // [V] device copy
    uint8_t* flags;                               // [S, nbrick]
    float* depth;                                 // [V, h, 4h]
    uint8_t* cls;
    float* normal;                                // [V, 3, h, 4h] or NULL
    float* out_color;                             // [V, 3, h, 4h] or NULL
    int* n_evaluated;                             // [V, h, 4h] or NULL
};

// ------------------------------------------------------------------------------------------------------- 1. brick flags
__global__ __launch_bounds__(kThreads) void render_flag_kernel(RenderBufs b, unsigned vblk) {
    const unsigned s = blockIdx.x / vblk, e = (blockIdx.x - s * vblk) * kThreads + threadIdx.x;
    if (e >= b.nvox) return;
    const size_t lin = (size_t)s * b.nvox + e;
    if (b.weight[lin] < b.min_weight || b.tsdf[lin] >= 0) return;
    const int i = (int)(e % (unsigned)b.nx), r = (int)(e / (unsigned)b.nx), j = r % b.ny, k = r / b.ny;
    uint8_t* flags = b.flags + (size_t)s * b.nbrick;
    for (int dk = -1; dk <= 0; ++dk)
        for (int dj = -1; dj <= 0; ++dj)
            for (int di = -1; di <= 0; ++di) {
                const int ci = i + di, cj = j + dj, ck = k + dk;                     // a cell this voxel is a corner of
                if (ci < 0 || ci > b.nx - 2 || cj < 0 || cj > b.ny - 2 || ck < 0 || ck > b.nz - 2) continue;
                flags[((size_t)(ck / kRenderBrick) * (size_t)b.by + (size_t)(cj / kRenderBrick)) * (size_t)b.bx + (size_t)(ci / kRenderBrick)] = 1;
            }
}

// ------------------------------------------------------------------------------------------------------- 2. the march
__global__ __launch_bounds__(kThreads) void render_kernel(RenderBufs b) {
    __shared__ double s_W[12];
    const int tid = threadIdx.x;
    const unsigned v = blockIdx.x / b.nblk, blk = blockIdx.x - v * b.nblk;
    if (tid == 0) {
        double T[12];
        for (int e = 0; e < 12; ++e) T[e] = b.pose[(size_t)v * 16 + e];
        align_inverse(T, s_W);
    }
    __syncthreads();
    const int h = b.h;
    const unsigned npix = (unsigned)h * 4u * (unsigned)h, pix = blk * kThreads + tid;       // V * npix < 2^31
    if (pix >= npix) return;
    double W[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) W[e] = s_W[e];
    const int s = b.scene_of_view[v];
    RenderVolume g;
    g.nx = b.nx; g.ny = b.ny; g.nz = b.nz; g.min_weight = b.min_weight;
    g.bx = b.bx; g.by = b.by; g.bz = b.bz;
    g.nvox = b.nvox;
    g.voxel = b.voxel;
#pragma unroll
    for (int a = 0; a < 3; ++a) g.origin[a] = b.origin[3 * s + a];
    g.tsdf = b.tsdf + (size_t)s * b.nvox;
    g.weight = b.weight + (size_t)s * b.nvox;
    g.color = b.color ? b.color + (size_t)s * 3 * b.nvox : nullptr;
    g.flags = b.skip ? b.flags + (size_t)s * b.nbrick : nullptr;
    const unsigned row = pix / (4u * h), col = pix - row * (4u * h);
    double dir[3];
    render_ray(b.suncg != 0, h, (int)row, (int)col, dir);
    int k0, k1;
    render_clip(g, W, dir, b.d_min, b.step, b.n_steps, k0, k1);
    RenderPixel o;
    render_march(g, W, dir, b.d_min, b.step, k0, k1, b.normal != nullptr, b.out_color != nullptr, o);
    const size_t at = (size_t)v * npix + pix;
    b.depth[at] = o.depth;
    b.cls[at] = (uint8_t)o.cls;
    if (b.n_evaluated) b.n_evaluated[at] = o.n_evaluated;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (b.normal) b.normal[((size_t)v * 3 + c) * npix + pix] = o.normal[c];
        if (b.out_color) b.out_color[((size_t)v * 3 + c) * npix + pix] = o.color[c];
    }
}

// ------------------------------------------------------------------------------------------------------- host
bool shapes_ok(long long S, long long V, long long h, long long nx, long long ny, long long nz) {
    if (!tsdf_volume_ok(S, nx, ny, nz) || 3 * nx * ny * nz >= (1ll << 31)) return false;
    return V >= 1 && h >= 2 && h <= 8192 && !(h & 1) && V * h * 4 * h < (1ll << 31);
}

size_t bricks_of(int nx, int ny, int nz) { return (size_t)render_bricks(nx) * render_bricks(ny) * render_bricks(nz); }

size_t carve(int S, int V, size_t nbrick, char* base, const double*& origin, const int*& sov, uint8_t*& flags) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    origin = (const double*)take((size_t)S * 3 * sizeof(double));
    sov = (const int*)take((size_t)V * sizeof(int));
    flags = (uint8_t*)take(std::max<size_t>((size_t)S * nbrick, 1));
    return off;
}

}  // namespace

extern "C" size_t relpose_tsdf_render_workspace_bytes(int32_t n_scenes, int32_t n_views, int32_t h, int32_t nx, int32_t ny, int32_t nz) {
    if (!shapes_ok(n_scenes, n_views, h, nx, ny, nz)) return 0;
    const double* org;
    const int* sov;
    uint8_t* flags;
    return carve(n_scenes, n_views, bricks_of(nx, ny, nz), nullptr, org, sov, flags);
}

extern "C" int relpose_tsdf_render(const RelposeTsdfRenderArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeTsdfRenderArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeTsdfRenderArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeTsdfRenderArgs)));
    if (!a.tsdf_sum || !a.weight || !a.pose || !a.origin_host || !a.scene_of_view_host || !a.depth || !a.cls || !a.workspace) return RELPOSE_EINVAL;
    if (a.color && !a.color_sum) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    if (a.reserved0 != 0 || a.min_weight < 1 || a.n_steps < 1 || a.n_steps > kRenderMaxSteps || (a.skip != 0 && a.skip != 1)) return RELPOSE_EINVAL;
    if (!(std::isfinite(a.voxel) && a.voxel > 0.0) || !(std::isfinite(a.d_min) && a.d_min >= 0.0) || !(std::isfinite(a.step) && a.step > 0.0))
        return RELPOSE_EINVAL;
    if (!shapes_ok(a.n_scenes, a.n_views, a.h, a.nx, a.ny, a.nz)) return RELPOSE_EINVAL;
    for (int v = 0; v < a.n_views; ++v)
        if (a.scene_of_view_host[v] < 0 || a.scene_of_view_host[v] >= a.n_scenes) return RELPOSE_EINVAL;
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    RenderBufs k{};
    const size_t nbrick = bricks_of(a.nx, a.ny, a.nz);
    if (a.workspace_bytes < carve(a.n_scenes, a.n_views, nbrick, nullptr, k.origin, k.scene_of_view, k.flags) || ((uintptr_t)a.workspace & 255))
        return RELPOSE_EINVAL;
    carve(a.n_scenes, a.n_views, nbrick, (char*)a.workspace, k.origin, k.scene_of_view, k.flags);
    k.h = a.h; k.suncg = a.dataset == RELPOSE_SUNCG; k.nx = a.nx; k.ny = a.ny; k.nz = a.nz; k.min_weight = a.min_weight;
    k.n_steps = a.n_steps; k.skip = a.skip;
    k.bx = render_bricks(a.nx); k.by = render_bricks(a.ny); k.bz = render_bricks(a.nz);
    k.nvox = (unsigned)((long long)a.nx * a.ny * a.nz);
    k.nbrick = (unsigned)nbrick;
    k.nblk = (unsigned)(((long long)a.h * 4 * a.h + kThreads - 1) / kThreads);
    k.voxel = a.voxel; k.d_min = a.d_min; k.step = a.step;
    k.tsdf = a.tsdf_sum; k.weight = a.weight; k.color = a.color_sum; k.pose = a.pose;
    k.depth = a.depth; k.cls = a.cls; k.normal = a.normal; k.out_color = a.color; k.n_evaluated = a.n_evaluated;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.origin, a.origin_host, (size_t)a.n_scenes * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.scene_of_view, a.scene_of_view_host, (size_t)a.n_views * sizeof(int), hipMemcpyHostToDevice, s));
    if (a.skip && nbrick > 0) {
        const unsigned vblk = tsdf_blocks_of(k.nvox);                 // S * vblk < 2^31 / 256 + S
        RP_HIP(hipMemsetAsync(k.flags, 0, (size_t)a.n_scenes * nbrick, s));
        hipLaunchKernelGGL(render_flag_kernel, dim3((unsigned)a.n_scenes * vblk), dim3(kThreads), 0, s, k, vblk);
    }
    hipLaunchKernelGGL(render_kernel, dim3((unsigned)a.n_views * k.nblk), dim3(kThreads), 0, s, k);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the two host arrays are the caller's again
    return 0;
}
