// Indexed triangle meshes from TSDF volumes: marching cubes over relpose_tsdf_fuse's state (the contract stands above
// relpose_tsdf_mesh in include/relpose.h, tests/mesh_model.py restates it in numpy).  The vertices are relpose_tsdf_surface's crossings,
// written by the same device text (tsdf_surf.h), so they are that cloud bit for bit; the triangles are integers.  Built with
// -ffp-contract=off.  One thread per voxel, a workgroup = kTsdfTile consecutive voxels of one scene in the x-fastest order; the thread of
// voxel (i, j, k) owns the voxel's crossings and the cell whose lowest corner the voxel is.  The lanes of a wave are neighbours in x, so
// each of a cell's eight corner loads is one coalesced load of the wave, and the corners a cell shares with its neighbours come from the
// caches: staging the four runs of voxels a workgroup's cells touch (rows j, j + 1 of slabs k, k + 1) in LDS first measured 6 % to 9 %
// SLOWER than these plain loads (DESIGN.md §4.18 has the numbers), so the simpler kernels stay.  No atomics: the order of the vertices
// and of the triangles is the voxel order, and a scene's result does not depend on the batch around it.
//
//   mesh_count_kernel     per thread the crossings of its voxel (0..3) and the triangles of its cell (0..5), from one flag (known, negative)
//                         per corner voxel read from tsdf_sum and weight; both summed over the workgroup.  The case table (2 KiB) is read
//                         from memory where it stands: a copy in LDS measured no faster (0.7 % slower on the larger workload).
//   mesh_scan_kernel      one workgroup per scene: the exclusive scans of both count arrays in place, n_points and n_triangles.
//   mesh_vertex_kernel    tsdf_surf.h's write body; leaves the index of every voxel's first vertex and its flag byte (crossing mask, known,
//                         negative) in the workspace.
//   mesh_triangle_kernel  the cell's case from the eight flag bytes; an ordered scan of the cells' triangle counts; a table entry (edge id)
//                         becomes the owning corner voxel's first index plus the number of lower axes set in its mask.
// Every loop has a bound known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "mc_table.h"
#include "tsdf_surf.h"

namespace {

constexpr int kKnown = 8, kNeg = 16;             // flag byte: bits 0..2 the crossing mask, bit 3 known, bit 4 t < 0

struct MeshBufs {
    SurfBufs v;                                  // the vertex pass; v.blk = the crossings per workgroup
    int cap_tri;
    int* tri;                                    // [S, cap_tri, 3]
    int* n_tri;                                  // [S]
    int* blk_tri;                                // [S, nblk]
    int* first;                                  // [S, nvox]: the index of the voxel's first vertex
    uint8_t* flag;                               // [S, nvox]
};

struct Cell {
    unsigned e, i, j, k;                         // the thread's voxel: linear index in the scene and coordinates
    bool cell;                                   // the voxel is inside the volume and the lowest corner of a cell
};

__device__ __forceinline__ Cell cell_of(const SurfBufs& b, unsigned blk) {
    Cell c;
    c.e = blk * kTsdfTile + threadIdx.x;                             // nvox < 2^31: no wrap
    const unsigned r = c.e / (unsigned)b.nx;
    c.i = c.e % (unsigned)b.nx; c.j = r % (unsigned)b.ny; c.k = r / (unsigned)b.ny;
    c.cell = c.e < b.nvox && (int)c.i < b.nx - 1 && (int)c.j < b.ny - 1 && (int)c.k < b.nz - 1;
    return c;
}

// the linear offset of corner c (0..7) from the cell's lowest voxel
__device__ __forceinline__ size_t corner_offset(const SurfBufs& b, int c) {
    return (size_t)(c & 1) + (size_t)(c >> 1 & 1) * (unsigned)b.nx + (size_t)(c >> 2 & 1) * ((size_t)(unsigned)b.nx * (unsigned)b.ny);
}

// known and negative of the voxel at o, from the volume (t < 0 iff tsdf_sum < 0: a known voxel's weight is >= 1)
__device__ __forceinline__ int flag_of(const SurfBufs& b, size_t o) {
    return b.weight[o] >= b.min_weight ? kKnown | (b.tsdf[o] < 0 ? kNeg : 0) : 0;
}

// the case of a cell from its corners' flags f[8], or -1 where a corner is unknown
__device__ __forceinline__ int case_of(const int f[8]) {
    int known = kKnown, cs = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        known &= f[c];
        cs |= (f[c] >> 4 & 1) << c;
    }
    return known ? cs : -1;
}

__global__ __launch_bounds__(kTsdfTile) void mesh_count_kernel(MeshBufs m) {
    __shared__ int s_wsum[16];
    const SurfBufs& b = m.v;
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const Cell c = cell_of(b, blk);
    const size_t o = (size_t)s * b.nvox + c.e;
    int f[8] = {0, 0, 0, 0, 0, 0, 0, 0};                             // the corners, where they are inside the volume
    if (c.e < b.nvox) {
        const bool px = (int)c.i + 1 < b.nx, py = (int)c.j + 1 < b.ny, pz = (int)c.k + 1 < b.nz;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if ((px || !(q & 1)) && (py || !(q & 2)) && (pz || !(q & 4))) f[q] = flag_of(b, o + corner_offset(b, q));
    }
    int nv = 0;                                                      // a crossing: both ends known, one negative
    if (f[0] & kKnown) nv = ((f[1] & kKnown) && ((f[1] ^ f[0]) & kNeg)) + ((f[2] & kKnown) && ((f[2] ^ f[0]) & kNeg)) + ((f[4] & kKnown) && ((f[4] ^ f[0]) & kNeg));
    const int cs = c.cell ? case_of(f) : -1;
    const int nt = cs < 0 ? 0 : (int)(rp_mc_table[cs] >> 60);
    int tv, tt;
    rp_block_excl_scan(nv, s_wsum, tv);
    rp_block_excl_scan(nt, s_wsum, tt);
    if (threadIdx.x == 0) {
        b.blk[(size_t)s * b.nblk + blk] = tv;
        m.blk_tri[(size_t)s * b.nblk + blk] = tt;
    }
}

__global__ __launch_bounds__(kTsdfScanThreads) void mesh_scan_kernel(MeshBufs m) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int nv = tsdf_scan_counts(m.v.blk + (size_t)s * m.v.nblk, m.v.nblk, s_wsum);
    const int nt = tsdf_scan_counts(m.blk_tri + (size_t)s * m.v.nblk, m.v.nblk, s_wsum);
    if (threadIdx.x == 0) {
        m.v.n_points[s] = nv;                                        // <= 3 nvox < 2^31
        m.n_tri[s] = nt;                                             // <= 5 cells < 2^31
    }
}

__global__ __launch_bounds__(kTsdfTile) void mesh_vertex_kernel(MeshBufs m) {
    __shared__ int s_wsum[16];
    const SurfBufs& b = m.v;
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const unsigned e = blk * kTsdfTile + threadIdx.x;
    const size_t o = (size_t)s * b.nvox + e;
    const int f = e < b.nvox ? flag_of(b, o) : 0;
    int first;
    const int mask = tsdf_write_body(b, s_wsum, first);
    if (e < b.nvox) {
        m.first[o] = first;
        m.flag[o] = (uint8_t)(f | mask);
    }
}

__global__ __launch_bounds__(kTsdfTile) void mesh_triangle_kernel(MeshBufs m) {
    __shared__ int s_wsum[16];
    const SurfBufs& b = m.v;
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const Cell c = cell_of(b, blk);
    const size_t o = (size_t)s * b.nvox + c.e;
    int f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c.cell) {
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = m.flag[o + corner_offset(b, q)];
    }
    const int cs = c.cell ? case_of(f) : -1;
    const unsigned long long w = cs < 0 ? 0ull : rp_mc_table[cs];
    const int nt = (int)(w >> 60);
    int total;
    int at = m.blk_tri[(size_t)s * b.nblk + blk] + rp_block_excl_scan(nt, s_wsum, total);
    int* out = m.tri + (size_t)s * m.cap_tri * 3;
    for (int q = 0; q < nt && at < m.cap_tri; ++q, ++at) {           // nt <= 5
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const int ed = (int)(w >> 4 * (3 * q + x)) & 15, a = ed >> 2, u = ed & 1, v = ed >> 1 & 1;
            const int corner = a == 0 ? 2 * u + 4 * v : (a == 1 ? u + 4 * v : u + 2 * v);                  // the edge's owner
            const size_t oc = o + corner_offset(b, corner);
            out[(size_t)at * 3 + x] = m.first[oc] + __popc(m.flag[oc] & ((1 << a) - 1));
        }
    }
}

size_t carve_mesh(int S, unsigned nblk, long long nvox, char* base, MeshBufs& m) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    m.v.origin = (const double*)take((size_t)S * 3 * sizeof(double));
    m.v.blk = (int*)take((size_t)S * nblk * sizeof(int));
    m.blk_tri = (int*)take((size_t)S * nblk * sizeof(int));
    m.first = (int*)take((size_t)S * (size_t)nvox * sizeof(int));
    m.flag = (uint8_t*)take((size_t)S * (size_t)nvox);
    return off;
}

bool mesh_sizes_ok(long long S, long long nx, long long ny, long long nz) {
    if (!tsdf_volume_ok(S, nx, ny, nz) || 3ll * nx * ny * nz >= (1ll << 31)) return false;
    return 5ll * (nx - 1) * (ny - 1) * (nz - 1) < (1ll << 31);
}

}  // namespace

extern "C" size_t relpose_tsdf_mesh_workspace_bytes(int32_t n_scenes, int32_t nx, int32_t ny, int32_t nz) {
    if (!mesh_sizes_ok(n_scenes, nx, ny, nz)) return 0;
    MeshBufs m{};
    const long long nvox = (long long)nx * ny * nz;
    return carve_mesh(n_scenes, tsdf_blocks_of(nvox), nvox, nullptr, m);
}

extern "C" int relpose_tsdf_mesh(const RelposeTsdfMeshArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeTsdfMeshArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeTsdfMeshArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeTsdfMeshArgs)));
    if (!a.tsdf_sum || !a.weight || !a.origin_host || !a.points || !a.normals || !a.valid || !a.n_points || !a.triangles || !a.n_triangles ||
        !a.workspace)
        return RELPOSE_EINVAL;
    if (a.colors && !a.color_sum) return RELPOSE_EINVAL;
    if (a.min_weight < 1 || a.cap < 1 || a.cap_tri < 1 || !(std::isfinite(a.voxel) && a.voxel > 0.0)) return RELPOSE_EINVAL;
    if (!mesh_sizes_ok(a.n_scenes, a.nx, a.ny, a.nz)) return RELPOSE_EINVAL;
    if ((long long)a.n_scenes * a.cap >= (1ll << 29) || (long long)a.n_scenes * a.cap_tri >= (1ll << 29)) return RELPOSE_EINVAL;
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    MeshBufs m{};
    SurfBufs& k = m.v;
    const long long nvox = (long long)a.nx * a.ny * a.nz;
    k.nvox = (unsigned)nvox;
    k.nblk = tsdf_blocks_of(nvox);
    if (a.workspace_bytes < carve_mesh(a.n_scenes, k.nblk, nvox, nullptr, m) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_mesh(a.n_scenes, k.nblk, nvox, (char*)a.workspace, m);
    k.nx = a.nx; k.ny = a.ny; k.nz = a.nz; k.min_weight = a.min_weight; k.cap = a.cap;
    k.voxel = a.voxel;
    k.tsdf = a.tsdf_sum; k.weight = a.weight; k.color = a.color_sum;
    k.points = a.points; k.normals = a.normals; k.colors = a.colors; k.valid = a.valid; k.n_points = a.n_points;
    m.cap_tri = a.cap_tri; m.tri = a.triangles; m.n_tri = a.n_triangles;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemcpyAsync((void*)k.origin, a.origin_host, (size_t)a.n_scenes * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    const unsigned grid = (unsigned)a.n_scenes * k.nblk;
    hipLaunchKernelGGL(mesh_count_kernel, dim3(grid), dim3(kTsdfTile), 0, s, m);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3((unsigned)a.n_scenes), dim3(kTsdfScanThreads), 0, s, m);
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(grid), dim3(kTsdfTile), 0, s, m);
    hipLaunchKernelGGL(mesh_triangle_kernel, dim3(grid), dim3(kTsdfTile), 0, s, m);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the host origin is the caller's again
    return 0;
}
