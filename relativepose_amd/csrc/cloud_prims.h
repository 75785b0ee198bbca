// Device code shared by the point-cloud kernels (fgr.hip, ransac.hip, cicp.hip, overlap.hip): the lane mask, the ordered block scans, the
// xor-tree reductions, the stable block radix sort, the voxel downsample around it and the normal of a neighbour list.  Every function is
// force-inlined or a template, so a kernel's code is what it was when the function's text stood in the kernel's own file.  The contracts
// that pin every rounded operation and every order here are DESIGN.md §4.6 (voxels, normals), §4.7 / §4.8 (reductions) and §4.14 (sort);
// the including files are built with -ffp-contract=off.
#pragma once
#include <cfloat>

#include "common.h"
#include "rp_math.h"

// ------------------------------------------------------------------------------------------------------- small helpers
// the lanes of the wave below this one, as a ballot mask
__device__ __forceinline__ unsigned long long rp_lanes_below() { return (1ull << rp_lane()) - 1ull; }

__device__ __forceinline__ bool rp_lex_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// (rp_dot3 = (a0 b0 + a1 b1) + a2 b2 is rp_math.h's)
__device__ __forceinline__ void rp_cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// |a - b| with d = a - b and (d0^2 + d1^2) + d2^2
__device__ __forceinline__ double rp_dist3(const double* a, const double* b) {
    const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    return sqrt(rp_dot3(d, d));
}

// the first index of ascending a[0..n) whose element is not below v
template <class T>
__device__ __forceinline__ int rp_lower_bound(const T* a, int n, T v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------- xor-tree reductions
// Over the 64 lanes by the xor-shuffle butterfly (32, 16, .., 1), result in every lane.  The sum is the one DESIGN.md §4.6 stage 8, §4.7
// step 7 and §4.8 name; common.h's rp_wave_sum adds in another order and rounds differently.
__device__ __forceinline__ double rp_wave_xor_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += rp_shfl_xor_d(v, m);
    return v;
}
__device__ __forceinline__ double rp_wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, rp_shfl_xor_d(v, m));
    return v;
}
__device__ __forceinline__ double rp_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, rp_shfl_xor_d(v, m));
    return v;
}

// Over a workgroup of NW waves, in every thread: the wave results, then the NW partials in wave order.  `red` holds NW doubles and may be
// shared by back-to-back calls (the leading barrier ends the previous call's reads).  fmin / fmax drop NaN operands.
template <int NW>
__device__ __forceinline__ double rp_block_xor_sum(double v, double* red) {
    v = rp_wave_xor_sum(v);
    __syncthreads();
    if (rp_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) r += red[k];
    return r;
}
template <int NW>
__device__ __forceinline__ double rp_block_min(double v, double* red) {
    v = rp_wave_min(v);
    __syncthreads();
    if (rp_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) r = fmin(r, red[k]);
    return r;
}
template <int NW>
__device__ __forceinline__ double rp_block_max(double v, double* red) {
    v = rp_wave_max(v);
    __syncthreads();
    if (rp_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) r = fmax(r, red[k]);
    return r;
}

// ------------------------------------------------------------------------------------------------------- ordered block scans
// Block-wide ordered scan of one flag per thread (blockDim a multiple of 64, at most 1024): exclusive prefix and total.  Write, barrier,
// read, barrier: the trailing barrier lets back-to-back calls share `wsum` (16 ints).  Before the FIRST call of a sequence nothing may
// still read `wsum`: a barrier must lie between the last read of the scratch by other code and this call.  (overlap.hip shares the
// scratch with its integer block sum; the six block minima between that sum and the first scan bring twelve barriers.)
__device__ __forceinline__ int rp_block_rank(bool f, int* wsum, int& total) {
    const unsigned long long m = __ballot(f);
    const int w = threadIdx.x >> 6;
    if (rp_lane() == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = 0, tot = 0;
    const int nw = blockDim.x >> 6;
    for (int k = 0; k < nw; ++k) {
        const int v = wsum[k];
        before += k < w ? v : 0;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return before + __popcll(m & rp_lanes_below());
}

// Block-wide exclusive scan of one int per thread (blockDim a multiple of 64, at most 1024) and the total; barriers as rp_block_rank.
__device__ __forceinline__ int rp_block_excl_scan(int v, int* wsum, int& total) {
    const int lane = rp_lane(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = 0, tot = 0;
    for (int k = 0; k < nw; ++k) {
        const int s = wsum[k];
        before += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return before + x - v;
}

// ------------------------------------------------------------------------------------------------------- block radix sort
constexpr int kRpSortThreads = 1024;

struct RpSortScratch {
    int digit_cnt[kRpSortThreads / 64][16];      // per wave, per digit: the wave's keys with that digit in the current round
    int base[16];                                // per digit: where its next key goes
};

// Stable LSD radix sort of (key, idx)[0..nv) on the low `bits` bits of the keys, 4-bit digits, by a workgroup of kRpSortThreads threads that
// has passed a barrier since the arrays were written.  Every pass scatters (key0, idx0) into (key1, idx1) and swaps the four pointers:
// on return (key0, idx0) hold the sorted order behind a barrier, and the result says which buffer that is (passes & 1: 0 = the
// caller's key0).  bits == 0: no pass.
__device__ __forceinline__ int rp_block_radix_sort(long long*& key0, int*& idx0, long long*& key1, int*& idx1, int nv, int bits,
                                                   RpSortScratch& lds) {
    constexpr int nt = kRpSortThreads;
    const int tid = threadIdx.x, w = tid >> 6, lane = rp_lane();
    int which = 0;
    for (int sh = 0; sh < bits; sh += 4) {
        if (tid < 16) lds.base[tid] = 0;
        __syncthreads();
        for (int e = tid; e < nv; e += nt) atomicAdd(&lds.base[(key0[e] >> sh) & 15], 1);
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int d = 0; d < 16; ++d) { const int v = lds.base[d]; lds.base[d] = s; s += v; }
        }
        __syncthreads();
        for (int t0 = 0; t0 < nv; t0 += nt) {
            const int e = t0 + tid;
            const bool in = e < nv;
            const long long k = in ? key0[e] : 0;
            const int d = in ? (int)((k >> sh) & 15) : -1;
            int rank = 0;
            for (int dd = 0; dd < 16; ++dd) {
                const unsigned long long m = __ballot(d == dd);
                if (d == dd) rank = __popcll(m & rp_lanes_below());
                if (lane == 0) lds.digit_cnt[w][dd] = __popcll(m);
            }
            __syncthreads();
            if (in) {
                int off = lds.base[d] + rank;
                for (int k2 = 0; k2 < w; ++k2) off += lds.digit_cnt[k2][d];
                key1[off] = k;
                idx1[off] = idx0[e];
            }
            __syncthreads();
            if (tid < 16) {
                int s = 0;
                for (int k2 = 0; k2 < nt / 64; ++k2) s += lds.digit_cnt[k2][tid];
                lds.base[tid] += s;
            }
            __syncthreads();
        }
        long long* tk = key0; key0 = key1; key1 = tk;
        int* ti = idx0; idx0 = idx1; idx1 = ti;
        which ^= 1;
    }
    return which;
}

// ------------------------------------------------------------------------------------------------------- voxel downsample
struct RpVoxelScratch {
    double smin[3][kRpSortThreads];
    long long smax[3][kRpSortThreads];
    int wsum[16];
    RpSortScratch sort;
};

// The voxel downsample of DESIGN.md §4.6 stage 1 by one workgroup of kRpSortThreads threads: the minimum of the valid points, min bound =
// minimum - voxel / 2, key = (kx ny + ky) nz + kz with k = floor((p - min bound) / voxel), compaction in input order, the stable sort,
// then one thread per voxel: the sum of its points in input order, s / (double)m, into out[3 o ..] for the first `cap` voxels in key
// order.  Returns the true voxel count (0 without a valid point).  key / idx are the [P] ping-pong buffers.  The policy `pol` has
//   static constexpr bool kExtra   a second per-point channel (pol.extra_in [P, 3]) is averaged like the points into pol.extra_out [cap, 3]
//   pol.lattice(mb, nx, ny, nz)    thread 0, once: the min bound and the cells per axis
//   pol.voxel(o, key, ny, nz)      the owning thread of voxel o < cap
template <class Policy>
__device__ __forceinline__ int rp_voxel_downsample(const double* pc, const uint8_t* valid, long long P, double vox, long long* key0, int* idx0,
                                                   long long* key1, int* idx1, double* out, int cap, RpVoxelScratch& lds, const Policy& pol) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX};
    for (long long e = tid; e < P; e += nt)
        if (valid[e])
            for (int a = 0; a < 3; ++a) mn[a] = fmin(mn[a], pc[3 * e + a]);
    for (int a = 0; a < 3; ++a) lds.smin[a][tid] = mn[a];
    __syncthreads();
    for (int s = nt / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int a = 0; a < 3; ++a) lds.smin[a][tid] = fmin(lds.smin[a][tid], lds.smin[a][tid + s]);
        __syncthreads();
    }
    if (lds.smin[0][0] == DBL_MAX) return 0;      // no valid point
    const double mb[3] = {lds.smin[0][0] - 0.5 * vox, lds.smin[1][0] - 0.5 * vox, lds.smin[2][0] - 0.5 * vox};
    long long mx[3] = {0, 0, 0};
    for (long long e = tid; e < P; e += nt)
        if (valid[e])
            for (int a = 0; a < 3; ++a) mx[a] = max(mx[a], (long long)floor((pc[3 * e + a] - mb[a]) / vox));
    for (int a = 0; a < 3; ++a) lds.smax[a][tid] = mx[a];
    __syncthreads();
    for (int s = nt / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int a = 0; a < 3; ++a) lds.smax[a][tid] = max(lds.smax[a][tid], lds.smax[a][tid + s]);
        __syncthreads();
    }
    const long long dx = lds.smax[0][0] + 1, dy = lds.smax[1][0] + 1, dz = lds.smax[2][0] + 1, total_keys = dx * dy * dz;
    const int bits = total_keys > 1 ? 64 - __clzll((unsigned long long)(total_keys - 1)) : 0;
    if (tid == 0) pol.lattice(mb, dx, dy, dz);
    // compaction of the valid points, input order kept
    int nv = 0;
    for (long long t0 = 0; t0 < P; t0 += nt) {
        const long long e = t0 + tid;
        const bool v = e < P && valid[e];
        int tot;
        const int r = rp_block_rank(v, lds.wsum, tot);
        if (v) {
            long long k[3];
            for (int a = 0; a < 3; ++a) k[a] = (long long)floor((pc[3 * e + a] - mb[a]) / vox);
            key0[nv + r] = (k[0] * dy + k[1]) * dz + k[2];
            idx0[nv + r] = (int)e;
        }
        nv += tot;
    }
    __syncthreads();
    rp_block_radix_sort(key0, idx0, key1, idx1, nv, bits, lds.sort);
    // segmented means: one thread per voxel start, summing its points (and the extra channel) sequentially in input order
    int nvox = 0;
    for (int t0 = 0; t0 < nv; t0 += nt) {
        const int e = t0 + tid;
        const bool st = e < nv && (e == 0 || key0[e] != key0[e - 1]);
        int tot;
        const int r = rp_block_rank(st, lds.wsum, tot);
        const int o = nvox + r;
        if (st && o < cap) {
            const long long k = key0[e];
            double s[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
            int m = 0;
            for (int j = e; j < nv && key0[j] == k; ++j, ++m) {
                const long long i = idx0[j];
                for (int a = 0; a < 3; ++a) {
                    s[a] += pc[3 * i + a];
                    if constexpr (Policy::kExtra) u[a] += pol.extra_in[3 * i + a];
                }
            }
            for (int a = 0; a < 3; ++a) {
                out[3 * o + a] = s[a] / (double)m;
                if constexpr (Policy::kExtra) pol.extra_out[3 * o + a] = u[a] / (double)m;
            }
            pol.voxel(o, k, dy, dz);
        }
        nvox += tot;
    }
    return nvox;
}

// ------------------------------------------------------------------------------------------------------- normal of a neighbour list
constexpr int kRpJacobiSweeps = 6;

// Normal at the point p from its neighbour list nb[0..m) into pts (DESIGN.md §4.6 stage 3): (0, 0, 1) below 3 neighbours; else the mean,
// the six covariance sums / m, kRpJacobiSweeps cyclic Jacobi sweeps (rotations (0,1), (0,2), (1,2), fully unrolled: A and V stay in
// registers), the column of the smallest eigenvalue (ties to the lower index), normalised; then turned toward the origin.
__device__ __forceinline__ void rp_normal_from_neighbors(const double* pts, const int* nb, int m, const double* p, double nv[3]) {
    nv[0] = 0.0; nv[1] = 0.0; nv[2] = 1.0;
    if (m >= 3) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < m; ++j)
            for (int a = 0; a < 3; ++a) s[a] += pts[3 * nb[j] + a];
        const double mf = (double)m;
        const double mean[3] = {s[0] / mf, s[1] / mf, s[2] / mf};
        double C[6] = {0, 0, 0, 0, 0, 0};       // 00 01 02 11 12 22
        for (int j = 0; j < m; ++j) {
            const double d0 = pts[3 * nb[j]] - mean[0], d1 = pts[3 * nb[j] + 1] - mean[1], d2 = pts[3 * nb[j] + 2] - mean[2];
            C[0] += d0 * d0; C[1] += d0 * d1; C[2] += d0 * d2; C[3] += d1 * d1; C[4] += d1 * d2; C[5] += d2 * d2;
        }
        double A[3][3];
        A[0][0] = C[0] / mf; A[0][1] = A[1][0] = C[1] / mf; A[0][2] = A[2][0] = C[2] / mf;
        A[1][1] = C[3] / mf; A[1][2] = A[2][1] = C[4] / mf; A[2][2] = C[5] / mf;
        double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
        for (int sw = 0; sw < kRpJacobiSweeps; ++sw) {
#pragma unroll
            for (int rot = 0; rot < 3; ++rot) {
                const int pp = rot == 2 ? 1 : 0, qq = rot == 0 ? 1 : 2, r = 3 - pp - qq;
                const double apq = A[pp][qq];
                if (apq != 0.0) {
                    const double theta = (A[qq][qq] - A[pp][pp]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0) t = -t;
                    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                    const double app = A[pp][pp] - t * apq, aqq = A[qq][qq] + t * apq;
                    const double arp = A[r][pp], arq = A[r][qq];
                    const double nrp = cs * arp - sn * arq, nrq = sn * arp + cs * arq;
                    A[pp][pp] = app; A[qq][qq] = aqq; A[pp][qq] = A[qq][pp] = 0.0;
                    A[r][pp] = A[pp][r] = nrp; A[r][qq] = A[qq][r] = nrq;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double vkp = V[k][pp], vkq = V[k][qq];
                        V[k][pp] = cs * vkp - sn * vkq;
                        V[k][qq] = sn * vkp + cs * vkq;
                    }
                }
            }
        }
        int k = A[1][1] < A[0][0] ? 1 : 0;
        const double ek = k == 1 ? A[1][1] : A[0][0];
        if (A[2][2] < ek) k = 2;
        const double v0 = k == 0 ? V[0][0] : (k == 1 ? V[0][1] : V[0][2]);
        const double v1 = k == 0 ? V[1][0] : (k == 1 ? V[1][1] : V[1][2]);
        const double v2 = k == 0 ? V[2][0] : (k == 1 ? V[2][1] : V[2][2]);
        const double nn = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        nv[0] = v0 / nn; nv[1] = v1 / nn; nv[2] = v2 / nn;
    }
    const double w[3] = {0.0 - p[0], 0.0 - p[1], 0.0 - p[2]};
    if (rp_dot3(nv, w) < 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
}
