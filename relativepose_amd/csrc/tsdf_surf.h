// Device code shared by the two readers of a TSDF volume, tsdf.hip (relpose_tsdf_surface) and mesh.hip (relpose_tsdf_mesh): a voxel's value,
// its gradient, the crossings it owns, the per-scene scan of the workgroups' counts and the body that writes the crossings as points.  The
// mesh's vertices must be the surface cloud bit for bit, so both kernels run this one text.  Every function is force-inlined: a kernel's
// code is what it was when the text stood in its own file.  The contract is DESIGN.md §4.16; the including files are built with
// -ffp-contract=off.
#pragma once
#include "cloud_prims.h"
#include "common.h"

constexpr int kTsdfTile = 256;                   // voxels per workgroup of the surface and mesh kernels
constexpr int kTsdfScanThreads = 1024;
constexpr double kTsdfFix = 32768.0;             // tsdf_sum counts t in 1 / 32768

struct SurfBufs {
    int nx, ny, nz, min_weight, cap;
    unsigned nvox, nblk;
    double voxel;
    const int* tsdf;
    const int* weight;
    const unsigned* color;                       // or NULL
    const double* origin;                        // [S, 3] device copy
    double* points;                              // [S, cap, 3]
    double* normals;
    float* colors;                               // [S, cap, 3] or NULL
    uint8_t* valid;                              // [S, cap]
    int* n_points;                               // [S]
    int* blk;                                    // [S, nblk]: the workgroups' counts, then their exclusive scan
};

// t of voxel (i, j, k) of the scene whose first voxel is `base`; false for a voxel outside the volume or below min_weight
__device__ __forceinline__ bool tsdf_value(const SurfBufs& b, size_t base, int i, int j, int k, double& t, unsigned& local) {
    if (i < 0 || i >= b.nx || j < 0 || j >= b.ny || k < 0 || k >= b.nz) return false;
    local = ((unsigned)k * (unsigned)b.ny + (unsigned)j) * (unsigned)b.nx + (unsigned)i;
    const int w = b.weight[base + local];
    if (w < b.min_weight) return false;
    t = (double)b.tsdf[base + local] / (kTsdfFix * (double)w);
    return true;
}

// central differences where both neighbours are known, one-sided where one is, 0 where none is
__device__ __forceinline__ void tsdf_gradient(const SurfBufs& b, size_t base, int i, int j, int k, double t, double g[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int di = c == 0, dj = c == 1, dk = c == 2;
        double tp = 0.0, tm = 0.0;
        unsigned l;
        const bool kp = tsdf_value(b, base, i + di, j + dj, k + dk, tp, l), km = tsdf_value(b, base, i - di, j - dj, k - dk, tm, l);
        g[c] = kp && km ? (tp - tm) * 0.5 : (kp ? tp - t : (km ? t - tm : 0.0));
    }
}

// the crossings of voxel e with its positive-axis neighbours as a 3-bit mask (bit = axis)
__device__ __forceinline__ int tsdf_crossings(const SurfBufs& b, size_t base, bool in, int i, int j, int k, double& ta, double tb[3]) {
    int mask = 0;
    unsigned l;
    if (in && tsdf_value(b, base, i, j, k, ta, l)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            tb[c] = 0.0;
            if (tsdf_value(b, base, i + (c == 0), j + (c == 1), k + (c == 2), tb[c], l) && ((ta >= 0 && tb[c] < 0) || (ta < 0 && tb[c] >= 0)))
                mask |= 1 << c;
        }
    }
    return mask;
}

// One workgroup of kTsdfScanThreads threads: the exclusive scan of cnt[0 .. nblk) in place -> the total (in every thread)
__device__ __forceinline__ int tsdf_scan_counts(int* cnt, unsigned nblk, int* s_wsum) {
    int run = 0;
    for (unsigned b0 = 0; b0 < nblk; b0 += kTsdfScanThreads) {       // nblk is the call's
        const unsigned x = b0 + threadIdx.x;
        const int v = x < nblk ? cnt[x] : 0;
        int total;
        const int ex = rp_block_excl_scan(v, s_wsum, total);
        if (x < nblk) cnt[x] = run + ex;
        run += total;
    }
    return run;
}

// The write pass of one workgroup of kTsdfTile threads (blockIdx.x = scene * nblk + workgroup): `valid`, the count pass again, an ordered
// scan inside the workgroup, and the points, normals and colours of the first `cap` crossings.  -> this thread's crossing mask, and in
// `first` the scene-wide index of its first crossing (the true index, whatever cap is).  Every barrier lies before the first return.
__device__ __forceinline__ int tsdf_write_body(const SurfBufs& b, int* s_wsum, int& first) {
    const unsigned s = blockIdx.x / b.nblk, blk = blockIdx.x - s * b.nblk;
    const unsigned e = blk * kTsdfTile + threadIdx.x;
    const unsigned iu = e % (unsigned)b.nx, r = e / (unsigned)b.nx;
    const int i = (int)iu, j = (int)(r % (unsigned)b.ny), k = (int)(r / (unsigned)b.ny);
    const size_t base = (size_t)s * b.nvox;
    const int cap = b.cap, n = b.n_points[s];
    for (unsigned x = e; x < (unsigned)cap; x += b.nblk * kTsdfTile) b.valid[(size_t)s * cap + x] = (uint8_t)((int)x < n);
    double ta = 0.0, tb[3];
    const int mask = tsdf_crossings(b, base, e < b.nvox, i, j, k, ta, tb);
    int total;
    int off = b.blk[(size_t)s * b.nblk + blk] + rp_block_excl_scan(__popc(mask), s_wsum, total);
    first = off;
    if (!mask) return 0;                                             // (no barrier follows)
    const double* org = b.origin + 3 * s;
    const double ctr[3] = {org[0] + ((double)i + 0.5) * b.voxel, org[1] + ((double)j + 0.5) * b.voxel, org[2] + ((double)k + 0.5) * b.voxel};
    double ga[3];
    tsdf_gradient(b, base, i, j, k, ta, ga);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!(mask >> c & 1)) continue;
        const int o = off++;
        if (o >= cap) continue;
        const int bi = i + (c == 0), bj = j + (c == 1), bk = k + (c == 2);
        const double sc = ta / (ta - tb[c]);
        double gb[3];
        tsdf_gradient(b, base, bi, bj, bk, tb[c], gb);
        double nv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) nv[a] = ga[a] + sc * (gb[a] - ga[a]);
        const double nn = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
        const int idx = c == 0 ? i : (c == 1 ? j : k);
        double* pt = b.points + ((size_t)s * cap + o) * 3;
        double* nm = b.normals + ((size_t)s * cap + o) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pt[a] = a == c ? org[a] + (((double)idx + 0.5) + sc) * b.voxel : ctr[a];
            nm[a] = nn > 0.0 ? nv[a] / nn : nv[a];
        }
        if (b.colors) {
            const unsigned la = ((unsigned)k * (unsigned)b.ny + (unsigned)j) * (unsigned)b.nx + iu;
            const unsigned lb = ((unsigned)bk * (unsigned)b.ny + (unsigned)bj) * (unsigned)b.nx + (unsigned)bi;
            const double wa = 255.0 * (double)b.weight[base + la], wb = 255.0 * (double)b.weight[base + lb];
            const unsigned* col = b.color + (size_t)s * 3 * b.nvox;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double ca = (double)col[(size_t)ch * b.nvox + la] / wa, cb = (double)col[(size_t)ch * b.nvox + lb] / wb;
                b.colors[((size_t)s * cap + o) * 3 + ch] = (float)(ca + sc * (cb - ca));
            }
        }
    }
    return mask;
}

// ------------------------------------------------------------------------------------------------------- host
inline bool tsdf_volume_ok(long long S, long long nx, long long ny, long long nz) {
    if (S < 1 || nx < 1 || ny < 1 || nz < 1) return false;
    const long long lim = 1ll << 31;
    if (nx >= lim || ny >= lim || nz >= lim || nx * ny >= lim || nx * ny * nz >= lim) return false;
    return S * (nx * ny * nz) < lim;
}

inline unsigned tsdf_blocks_of(long long nvox) { return (unsigned)((nvox + kTsdfTile - 1) / kTsdfTile); }
