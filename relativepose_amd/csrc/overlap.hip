// Overlap statistics of point clouds for a batch of directed (query cloud, reference cloud, pose) triples: per query the number of moved
// query points with a reference point nearer than max_dist, and the clouds' closest-pair distance.  The values are nn_dist_kernel's
// (geometry.hip: the same expressions, every operation rounded on its own, built with -ffp-contract=off); the contract is DESIGN.md §4.14
// and the comment above relpose_overlap in include/relpose.h; tests/overlap_model.py restates it in numpy.
//
//   overlap_build_kernel    one workgroup of 1024 threads per cloud, once per call, whatever names the cloud afterwards.  Bounds of the
//                           valid points with finite coordinates, the cell of every such point (edge = max_dist (1 + 2^-10), cell =
//                           floor((x - min) / edge) per axis, key = (cx ny + cy) nz + cz), compaction in input order, a stable LSD radix
//                           sort of (key, index) on 4-bit digits over just the bits the cloud's cell count needs, then the coordinates in
//                           key order and the bounding box of every tile of 256 consecutive sorted points.  Block 0 .. also reset the
//                           per-query accumulators.
//   overlap_grid_kernel     256 sorted query points per workgroup.  A point is moved, its cell in the REFERENCE grid computed, and the nine
//                           (x, y) columns around it searched: one binary search for the first key of the column's z-run, then a walk.  The
//                           minimum d2 is exact whenever it is below max_dist^2 (DESIGN.md §4.14 proves the 27 cells suffice).  Hits and the
//                           minimum are reduced in the workgroup, then one integer atomic each.
//   overlap_closest_kernel  only for queries whose hit count is still 0, read on the device: the closest pair of two clouds that do not
//                           touch.  A workgroup holds 256 moved query points and their bounding box and walks the reference tiles; a tile
//                           whose box-to-box bound cannot beat the running bound is skipped, and inside a tile a point whose point-to-box
//                           bound cannot either.  The bounds are evaluated with d2's own expression on per-axis gaps, and rounding is
//                           monotone, so bound <= every d2 of the tile: nothing is lost (no slack factor).  The running bound is shared by
//                           the query's workgroups through atomicMin on the bit pattern; the tile nearest to the block goes first.
//   overlap_finalize_kernel accumulators -> hits, nn_min = sqrt(min d2), n_valid.
// A cloud whose extent cannot be keyed raises a flag in the build kernel; the later kernels then return at once and the host reports it.
// The ordered scan of the compaction, the radix sort and the wave / block minima are cloud_prims.h's, shared with fgr.hip and cicp.hip; the
// bound and cell pass is this file's own (finite-point filter, origin at the minimum, tile boxes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "cloud_prims.h"
#include "common.h"

namespace {

constexpr int kTile = 256;                       // query points per workgroup and reference points per tile
constexpr int kBuildThreads = 1024;
constexpr double kMaxCells = 1048576.0;          // per axis: three axes stay below 2^60
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;

struct CloudHdr {
    double mn[3];                                // the minimum over the finite valid points
    long long nx, ny, nz;                        // cells per axis
    int nv;                                      // finite valid points = length of the sorted arrays
    int n_valid;                                 // valid points
    int which;                                   // which of the two key / index buffers holds the sorted order
    int pad;
};

struct OverlapBufs {
    int n_clouds, P, nq, nblk;
    double edge, max_dist;
    const double* pc;
    const uint8_t* valid;
    const int* qcloud;                           // [nq] device copies
    const int* rcloud;
    const double* pose;
    int* hits;
    double* nn_min;
    int* n_valid;
    uint8_t* hit;
    CloudHdr* hdr;                               // [n_clouds]
    long long* key[2];                           // [n_clouds, P]
    int* idx[2];                                 // [n_clouds, P]
    double* sx;                                  // [n_clouds, P] coordinates in key order
    double* sy;
    double* sz;
    double* box;                                 // [n_clouds, nblk, 6] lo xyz, hi xyz of every tile
    int* acc_hits;                               // [nq]
    unsigned long long* acc_d2;                  // [nq] bits of the smallest d2 seen
    int* bad;
};

__device__ int block_sum_i(int v, int* red) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = rp_wave_sum_i(v);
    __syncthreads();
    if (rp_lane() == 0) red[w] = v;
    __syncthreads();
    int r = 0;
    for (int k = 0; k < nw; ++k) r += red[k];
    return r;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ------------------------------------------------------------------------------------------------------- 1. one grid per cloud
__global__ __launch_bounds__(kBuildThreads) void overlap_build_kernel(OverlapBufs b) {
    const int c = blockIdx.x, tid = threadIdx.x, nt = kBuildThreads, lane = rp_lane(), w = tid >> 6;
    static_assert(kBuildThreads == kRpSortThreads, "rp_block_radix_sort");
    const int P = b.P;
    __shared__ double red[16];
    __shared__ int ired[16];
    __shared__ RpSortScratch sort_lds;

    for (long long q = (long long)c * nt + tid; q < b.nq; q += (long long)gridDim.x * nt) {
        b.acc_hits[q] = 0;
        b.acc_d2[q] = kInfBits;
    }

    const double* pc = b.pc + (size_t)c * P * 3;
    const uint8_t* va = b.valid ? b.valid + (size_t)c * P : nullptr;
    CloudHdr* hdr = b.hdr + c;

    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int nval = 0;
    for (int e = tid; e < P; e += nt) {
        const bool v = !va || va[e];
        nval += v ? 1 : 0;
        const double x = pc[3 * (size_t)e], y = pc[3 * (size_t)e + 1], z = pc[3 * (size_t)e + 2];
        if (v && finite3(x, y, z)) {
            lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
            hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y); hi[2] = fmax(hi[2], z);
        }
    }
    nval = block_sum_i(nval, ired);
    for (int a = 0; a < 3; ++a) {
        lo[a] = rp_block_min<kBuildThreads / 64>(lo[a], red);
        hi[a] = -rp_block_min<kBuildThreads / 64>(-hi[a], red);
    }
    double cells[3];
    bool bad = false;
    for (int a = 0; a < 3; ++a) {
        cells[a] = floor((hi[a] - lo[a]) / b.edge) + 1.0;          // no point's cell index exceeds the maximum's: rounding is monotone
        bad = bad || !(cells[a] <= kMaxCells);
    }
    const bool empty = !(lo[0] <= hi[0]);                           // no finite valid point
    if (empty || bad) {
        if (tid == 0) {
            hdr->mn[0] = hdr->mn[1] = hdr->mn[2] = 0.0;
            hdr->nx = hdr->ny = hdr->nz = 0;
            hdr->nv = 0; hdr->n_valid = nval; hdr->which = 0; hdr->pad = 0;
            if (bad && !empty) atomicMax(b.bad, 1);
        }
        return;
    }
    const long long ny = (long long)cells[1], nz = (long long)cells[2];
    const unsigned long long total = (unsigned long long)cells[0] * (unsigned long long)ny * (unsigned long long)nz;
    const int bits = total > 1 ? 64 - __clzll(total - 1) : 0;

    long long* key0 = b.key[0] + (size_t)c * P;
    long long* key1 = b.key[1] + (size_t)c * P;
    int* idx0 = b.idx[0] + (size_t)c * P;
    int* idx1 = b.idx[1] + (size_t)c * P;

    // compaction of the finite valid points, input order kept
    int nv = 0;
    for (int t0 = 0; t0 < P; t0 += nt) {
        const int e = t0 + tid;
        double x = 0.0, y = 0.0, z = 0.0;
        bool v = false;
        if (e < P) {
            x = pc[3 * (size_t)e]; y = pc[3 * (size_t)e + 1]; z = pc[3 * (size_t)e + 2];
            v = (!va || va[e]) && finite3(x, y, z);
        }
        int tot;
        const int r = rp_block_rank(v, ired, tot);
        if (v) {
            const long long cx = (long long)floor((x - lo[0]) / b.edge), cy = (long long)floor((y - lo[1]) / b.edge),
                            cz = (long long)floor((z - lo[2]) / b.edge);
            key0[nv + r] = (cx * ny + cy) * nz + cz;
            idx0[nv + r] = e;
        }
        nv += tot;
    }
    __syncthreads();

    const int which = rp_block_radix_sort(key0, idx0, key1, idx1, nv, bits, sort_lds);

    // coordinates in key order
    double* sx = b.sx + (size_t)c * P;
    double* sy = b.sy + (size_t)c * P;
    double* sz = b.sz + (size_t)c * P;
    for (int e = tid; e < nv; e += nt) {
        const size_t i = (size_t)idx0[e];
        sx[e] = pc[3 * i]; sy[e] = pc[3 * i + 1]; sz[e] = pc[3 * i + 2];
    }
    __syncthreads();
    // the bounding box of every tile: one wave per tile, four points per lane
    double* box = b.box + (size_t)c * b.nblk * 6;
    const int ntiles = (nv + kTile - 1) / kTile;
    for (int t = w; t < ntiles; t += nt / 64) {
        double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = lane; k < kTile; k += 64) {
            const int e = t * kTile + k;
            if (e < nv) {
                const double x = sx[e], y = sy[e], z = sz[e];
                l[0] = fmin(l[0], x); l[1] = fmin(l[1], y); l[2] = fmin(l[2], z);
                h[0] = fmax(h[0], x); h[1] = fmax(h[1], y); h[2] = fmax(h[2], z);
            }
        }
        for (int a = 0; a < 3; ++a) {
            l[a] = rp_wave_min(l[a]);
            h[a] = rp_wave_max(h[a]);
        }
        if (lane == 0)
            for (int a = 0; a < 3; ++a) { box[(size_t)t * 6 + a] = l[a]; box[(size_t)t * 6 + 3 + a] = h[a]; }
    }
    if (tid == 0) {
        for (int a = 0; a < 3; ++a) hdr->mn[a] = lo[a];
        hdr->nx = (long long)cells[0]; hdr->ny = ny; hdr->nz = nz;
        hdr->nv = nv; hdr->n_valid = nval; hdr->which = which; hdr->pad = 0;
    }
}

// the moved point of sorted slot i of cloud qc; NaN when the slot is past the cloud's sorted points
__device__ __forceinline__ void moved_point(const OverlapBufs& b, int qc, int q, int i, int nvq, double& x, double& y, double& z) {
    x = y = z = __builtin_nan("");
    if (i < nvq) {
        const size_t o = (size_t)qc * b.P + i;
        const double a = b.sx[o], bb = b.sy[o], c = b.sz[o];
        const double* T = b.pose + (size_t)q * 16;
        x = ((T[0] * a + T[1] * bb) + T[2] * c) + T[3];
        y = ((T[4] * a + T[5] * bb) + T[6] * c) + T[7];
        z = ((T[8] * a + T[9] * bb) + T[10] * c) + T[11];
    }
}

// ------------------------------------------------------------------------------------------------------- 2. the 27 cells
__global__ __launch_bounds__(kTile) void overlap_grid_kernel(OverlapBufs b) {
    if (*b.bad) return;
    const int tid = threadIdx.x, lane = rp_lane();
    const int q = blockIdx.x / b.nblk, blk = blockIdx.x - q * b.nblk;
    const int qc = b.qcloud[q], rc = b.rcloud[q];
    const int P = b.P;
    const int i = blk * kTile + tid;
    __shared__ int s_hits;
    __shared__ unsigned long long s_d2;
    if (tid == 0) { s_hits = 0; s_d2 = kInfBits; }
    __syncthreads();

    if (b.hit && i < P) {               // the points that are not in the sorted list never hit
        const double* p = b.pc + ((size_t)qc * P + i) * 3;
        const bool v = !b.valid || b.valid[(size_t)qc * P + i];
        if (!(v && finite3(p[0], p[1], p[2]))) b.hit[(size_t)q * P + i] = 0;
    }

    const CloudHdr hq = b.hdr[qc];
    const CloudHdr hr = b.hdr[rc];
    const int nvq = hq.nv, nvr = hr.nv;
    double x, y, z;
    moved_point(b, qc, q, i, nvq, x, y, z);
    double best = INFINITY;
    if (i < nvq && nvr > 0 && finite3(x, y, z)) {
        const double fx = floor((x - hr.mn[0]) / b.edge), fy = floor((y - hr.mn[1]) / b.edge), fz = floor((z - hr.mn[2]) / b.edge);
        if (fx >= -1.0 && fx <= (double)hr.nx && fy >= -1.0 && fy <= (double)hr.ny && fz >= -1.0 && fz <= (double)hr.nz) {
            const long long cx = (long long)fx, cy = (long long)fy, cz = (long long)fz;
            const long long z0 = cz - 1 < 0 ? 0 : cz - 1, z1 = cz + 1 > hr.nz - 1 ? hr.nz - 1 : cz + 1;
            const long long* keys = b.key[hr.which] + (size_t)rc * P;
            const double* rx = b.sx + (size_t)rc * P;
            const double* ry = b.sy + (size_t)rc * P;
            const double* rz = b.sz + (size_t)rc * P;
            if (z0 <= z1) {
                for (long long ax = cx - 1; ax <= cx + 1; ++ax) {
                    if (ax < 0 || ax >= hr.nx) continue;
                    for (long long ay = cy - 1; ay <= cy + 1; ++ay) {
                        if (ay < 0 || ay >= hr.ny) continue;
                        const long long k0 = (ax * hr.ny + ay) * hr.nz + z0, k1 = (ax * hr.ny + ay) * hr.nz + z1;
                        for (int e = rp_lower_bound(keys, nvr, k0); e < nvr && keys[e] <= k1; ++e) {
                            const double dx = x - rx[e], dy = y - ry[e], dz = z - rz[e];
                            const double d2 = (dx * dx + dy * dy) + dz * dz;
                            best = d2 < best ? d2 : best;
                        }
                    }
                }
            }
        }
    }
    const bool h = i < nvq && sqrt(best) < b.max_dist;
    if (i < nvq && b.hit) b.hit[(size_t)q * P + b.idx[hq.which][(size_t)qc * P + i]] = h ? 1 : 0;
    const int cnt = __popcll(__ballot(h));
    const double wmin = rp_wave_min(best);
    if (lane == 0) {
        if (cnt) atomicAdd(&s_hits, cnt);
        if (wmin < INFINITY) atomicMin(&s_d2, (unsigned long long)__double_as_longlong(wmin));
    }
    __syncthreads();
    if (tid == 0) {
        if (s_hits) atomicAdd(b.acc_hits + q, s_hits);
        if (s_d2 != kInfBits) atomicMin(b.acc_d2 + q, s_d2);
    }
}

// ------------------------------------------------------------------------------------------------------- 3. clouds that do not touch
// d2's expression on the per-axis gaps between two boxes (or a point and a box): <= the d2 of any pair of points inside them, because
// every rounded operation is monotone in its operands
__device__ __forceinline__ double gap(double lo_a, double hi_a, double lo_b, double hi_b) {
    const double g = fmax(lo_a - hi_b, lo_b - hi_a);
    return g > 0.0 ? g : 0.0;
}

__global__ __launch_bounds__(kTile) void overlap_closest_kernel(OverlapBufs b) {
    if (*b.bad) return;
    const int tid = threadIdx.x, lane = rp_lane();
    const int q = blockIdx.x / b.nblk, blk = blockIdx.x - q * b.nblk;
    if (b.acc_hits[q] > 0) return;                       // the grid pass found the closest pair already
    const int qc = b.qcloud[q], rc = b.rcloud[q];
    const int P = b.P;
    const int nvq = b.hdr[qc].nv, nvr = b.hdr[rc].nv;
    if (blk * kTile >= nvq || nvr == 0) return;
    __shared__ double red[kTile / 64];
    __shared__ double tx[kTile], ty[kTile], tz[kTile];
    __shared__ double s_lb[kTile];
    __shared__ int s_lt[kTile];
    __shared__ unsigned long long s_bound;

    double x, y, z;
    moved_point(b, qc, q, blk * kTile + tid, nvq, x, y, z);
    if (!finite3(x, y, z)) x = y = z = __builtin_nan("");    // never nearer than anything, and outside the block's box
    double blo[3], bhi[3];
    blo[0] = rp_block_min<kTile / 64>(x, red); blo[1] = rp_block_min<kTile / 64>(y, red); blo[2] = rp_block_min<kTile / 64>(z, red);
    bhi[0] = -rp_block_min<kTile / 64>(-x, red); bhi[1] = -rp_block_min<kTile / 64>(-y, red); bhi[2] = -rp_block_min<kTile / 64>(-z, red);
    if (!(blo[0] <= bhi[0])) return;                     // no finite moved point in this block

    const double* box = b.box + (size_t)rc * b.nblk * 6;
    const double* rx = b.sx + (size_t)rc * P;
    const double* ry = b.sy + (size_t)rc * P;
    const double* rz = b.sz + (size_t)rc * P;
    const int ntiles = (nvr + kTile - 1) / kTile;

    // the tile whose box is nearest to this block's goes first: it sets a bound that most other tiles cannot beat
    double lb0 = INFINITY;
    int t0 = 0x7fffffff;
    for (int t = tid; t < ntiles; t += kTile) {
        const double* bx = box + (size_t)t * 6;
        const double gx = gap(blo[0], bhi[0], bx[0], bx[3]), gy = gap(blo[1], bhi[1], bx[1], bx[4]), gz = gap(blo[2], bhi[2], bx[2], bx[5]);
        const double lb = (gx * gx + gy * gy) + gz * gz;
        if (lb < lb0) { lb0 = lb; t0 = t; }
    }
    s_lb[tid] = lb0; s_lt[tid] = t0;
    __syncthreads();
    for (int s = kTile / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double o = s_lb[tid + s];
            const int ot = s_lt[tid + s];
            if (o < s_lb[tid] || (o == s_lb[tid] && ot < s_lt[tid])) { s_lb[tid] = o; s_lt[tid] = ot; }
        }
        __syncthreads();
    }
    const int first = s_lt[0] < ntiles ? s_lt[0] : 0;
    if (tid == 0) s_bound = __hip_atomic_load(b.acc_d2 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    double bound = __longlong_as_double((long long)s_bound);        // uniform over the workgroup
    double best = INFINITY;

    for (int it = 0; it <= ntiles; ++it) {
        const int t = it == 0 ? first : it - 1;
        if (it > 0 && t == first) continue;
        const double* bx = box + (size_t)t * 6;
        const double gx = gap(blo[0], bhi[0], bx[0], bx[3]), gy = gap(blo[1], bhi[1], bx[1], bx[4]), gz = gap(blo[2], bhi[2], bx[2], bx[5]);
        const double lb = (gx * gx + gy * gy) + gz * gz;
        if (!(lb < bound)) continue;                     // uniform: every d2 of the tile is >= lb >= bound
        __syncthreads();
        const int e = t * kTile + tid;
        const bool in = e < nvr;
        tx[tid] = in ? rx[e] : __builtin_nan("");
        ty[tid] = in ? ry[e] : 0.0;
        tz[tid] = in ? rz[e] : 0.0;
        __syncthreads();
        const double px = gap(x, x, bx[0], bx[3]), py = gap(y, y, bx[1], bx[4]), pz = gap(z, z, bx[2], bx[5]);
        const double plb = (px * px + py * py) + pz * pz;
        const double mine = best < bound ? best : bound;
        if (plb < mine) {
            for (int k = 0; k < kTile; ++k) {
                const double dx = x - tx[k], dy = y - ty[k], dz = z - tz[k];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                best = d2 < best ? d2 : best;
            }
        }
        const double wmin = rp_wave_min(best);
        if (lane == 0 && wmin < bound) atomicMin(b.acc_d2 + q, (unsigned long long)__double_as_longlong(wmin));
        __syncthreads();
        if (tid == 0) s_bound = __hip_atomic_load(b.acc_d2 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        bound = __longlong_as_double((long long)s_bound);
    }
}

// ------------------------------------------------------------------------------------------------------- 4. outputs
__global__ void overlap_finalize_kernel(OverlapBufs b) {
    if (*b.bad) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b.nq) {
        b.hits[i] = b.acc_hits[i];
        b.nn_min[i] = sqrt(__longlong_as_double((long long)b.acc_d2[i]));
    }
    if (i < b.n_clouds) b.n_valid[i] = b.hdr[i].n_valid;
}

bool sizes_ok(long long n_clouds, long long P, long long nq) {
    if (n_clouds < 1 || nq < 1 || P < 1 || P > (1ll << 24)) return false;
    const long long nblk = (P + kTile - 1) / kTile;
    return nq * nblk < (1ll << 31) && n_clouds < (1ll << 24);
}

// carve the workspace; returns the bytes used
size_t carve(OverlapBufs& k, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    const size_t n = (size_t)k.n_clouds, P = (size_t)k.P, nq = (size_t)k.nq;
    k.bad = (int*)take(sizeof(int));
    k.hdr = (CloudHdr*)take(n * sizeof(CloudHdr));
    k.qcloud = (const int*)take(nq * sizeof(int));
    k.rcloud = (const int*)take(nq * sizeof(int));
    k.acc_hits = (int*)take(nq * sizeof(int));
    k.acc_d2 = (unsigned long long*)take(nq * sizeof(unsigned long long));
    for (int s = 0; s < 2; ++s) k.key[s] = (long long*)take(n * P * sizeof(long long));
    for (int s = 0; s < 2; ++s) k.idx[s] = (int*)take(n * P * sizeof(int));
    k.sx = (double*)take(n * P * sizeof(double));
    k.sy = (double*)take(n * P * sizeof(double));
    k.sz = (double*)take(n * P * sizeof(double));
    k.box = (double*)take(n * (size_t)k.nblk * 6 * sizeof(double));
    return off;
}

}  // namespace

extern "C" size_t relpose_overlap_workspace_bytes(int32_t n_clouds, int32_t n_points, int32_t n_queries) {
    if (!sizes_ok(n_clouds, n_points, n_queries)) return 0;
    OverlapBufs k{};
    k.n_clouds = n_clouds; k.P = n_points; k.nq = n_queries; k.nblk = (n_points + kTile - 1) / kTile;
    return carve(k, nullptr);
}

extern "C" int relpose_overlap(const RelposeOverlapArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeOverlapArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeOverlapArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeOverlapArgs)));
    if (!a.pc || !a.query_cloud_host || !a.ref_cloud_host || !a.pose || !a.hits || !a.nn_min || !a.n_valid || !a.workspace) return RELPOSE_EINVAL;
    if (!std::isfinite(a.max_dist) || !(a.max_dist > 0.0)) return RELPOSE_EINVAL;
    if (!sizes_ok(a.n_clouds, a.n_points, a.n_queries)) return RELPOSE_EINVAL;
    for (int q = 0; q < a.n_queries; ++q)
        if (a.query_cloud_host[q] < 0 || a.query_cloud_host[q] >= a.n_clouds || a.ref_cloud_host[q] < 0 || a.ref_cloud_host[q] >= a.n_clouds)
            return RELPOSE_EINVAL;
    OverlapBufs k{};
    k.n_clouds = a.n_clouds; k.P = a.n_points; k.nq = a.n_queries; k.nblk = (a.n_points + kTile - 1) / kTile;
    if (a.workspace_bytes < carve(k, nullptr) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve(k, (char*)a.workspace);
    k.edge = a.max_dist * (1.0 + 1.0 / 1024.0);
    k.max_dist = a.max_dist;
    k.pc = a.pc; k.valid = a.valid; k.pose = a.pose;
    k.hits = a.hits; k.nn_min = a.nn_min; k.n_valid = a.n_valid; k.hit = a.hit;
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemsetAsync(k.bad, 0, sizeof(int), s));
    RP_HIP(hipMemcpyAsync((void*)k.qcloud, a.query_cloud_host, (size_t)k.nq * sizeof(int), hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.rcloud, a.ref_cloud_host, (size_t)k.nq * sizeof(int), hipMemcpyHostToDevice, s));
    const unsigned nwork = (unsigned)((size_t)k.nq * k.nblk);
    const int nfin = std::max(k.nq, k.n_clouds);
    hipLaunchKernelGGL(overlap_build_kernel, dim3(k.n_clouds), dim3(kBuildThreads), 0, s, k);
    hipLaunchKernelGGL(overlap_grid_kernel, dim3(nwork), dim3(kTile), 0, s, k);
    hipLaunchKernelGGL(overlap_closest_kernel, dim3(nwork), dim3(kTile), 0, s, k);
    hipLaunchKernelGGL(overlap_finalize_kernel, dim3((nfin + 255) / 256), dim3(256), 0, s, k);
    RP_CHECK_LAUNCH();
    int bad = 0;
    RP_HIP(hipMemcpyAsync(&bad, k.bad, sizeof(int), hipMemcpyDeviceToHost, s));
    RP_HIP(hipStreamSynchronize(s));
    return bad ? RELPOSE_OVERLAP_EXTENT : 0;
}
