// Decimation of indexed triangle meshes by vertex clustering on a regular grid (the contract stands above
// relpose_mesh_decimate in include/relpose.h, tests/decimate_model.py restates it in numpy).  Built with -ffp-contract=off: a vertex's cell
// and the means round as the model's.  Whatever is summed across vertices is an integer, a cluster's representative is its smallest vertex
// index and of a set of duplicate triangles the lowest row survives, so every output is bitwise independent of the order the hardware works
// in, of the batch and of repeats.  Nothing waits on another thread; a launch sees all that earlier launches wrote.
//   dc_origin_kernel      the host origins, eight scenes per launch as a kernel argument (nothing is read from host memory after the call)
//   dc_init_kernel        the cell table to INT_MAX, the two hash tables to empty, the four counters to 0
//   dc_cell_kernel        per vertex its cell (or -1: dropped) and atomicMin of its index into the cell's table entry
//   dc_rep_count / dc_rep_scan / dc_rep_write   representatives (table[cell] == own index) flagged, counted per workgroup, scanned per scene,
//                         numbered in ascending order; a representative's accumulator row is cleared, out_valid written whole
//   dc_accumulate_kernel  vertex_map and the ten integers of every vertex (3 position, 3 normal, 3 colour, 1 count) added to its cluster's
//                         row: a run of equal clusters in consecutive lanes is summed inside the wave first (as meshcc.hip's cc_run_add)
//                         and added once with int64 atomics
//   dc_finalize_kernel    per cluster the mean position, the normalised normal sum, the mean colour and the count
//   dc_tri_kernel         per row its class (bad, outside, degenerate, beyond the count, or a candidate) and the three counters; with
//                         dedupe the candidate, rotated to its smallest index (a, b, c), takes the slot of (a, b) in one open-addressing
//                         table and the slot of (slot, c) in a second (CAS insert, linear probing, every probe loop bounded by the table
//                         size), and lowers that slot's row with atomicMin
//   dc_tri_count / dc_tri_scan / dc_tri_write   survivors (candidates that hold their slot's minimum) flagged, scanned, scattered in order
// Slot numbers depend on the order of insertion; which row survives does not (DESIGN.md §4.22 has the argument).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "cloud_prims.h"
#include "common.h"

namespace {

constexpr int kDcTile = 256;                     // vertices or triangles per workgroup
constexpr int kDcScanThreads = 1024;
constexpr int kDcAcc = 10;                       // int64 per cluster: 3 position, 3 normal, 3 colour, the count
constexpr int kDcOriginScenes = 8;               // origins per dc_origin_kernel launch
constexpr int kDcInitBlocks = 2048;              // dc_init_kernel strides over its tables
constexpr unsigned long long kDcEmpty = ~0ull;   // no key: a packed key's high word is below 2^31
constexpr int kDcNoSlot = INT_MAX;               // a candidate whose insert found no slot (a table at least twice the keys never fills)
constexpr int kDcBad = -1, kDcOutside = -2, kDcDegenerate = -3, kDcDuplicate = -4, kDcBeyond = -5;

struct DcBufs {
    int cap, cap_tri, gx, gy, gz, dedupe;
    unsigned G;                                  // cells per scene
    unsigned P;                                  // slots per scene in each hash table: a power of two >= 2 cap_tri
    unsigned nblk_v, nblk_t;                     // workgroups per scene over the vertices and over the triangles
    double cell;
    const double* points;                        // [S, cap, 3]
    const double* normals;
    const float* colors;                         // or null
    const int* n_pts;
    const int* tri;                              // [S, cap_tri, 3]
    const int* n_tri;
    double* o_points;
    double* o_normals;
    float* o_colors;
    uint8_t* o_valid;
    int* o_n_pts;
    int* o_count;
    int* o_tri;
    int* o_n_tri;
    int* vmap;                                   // [S, cap]
    int* tmap;                                   // [S, cap_tri] or null
    int* bad;                                    // [S] each
    int* outside;
    int* degenerate;
    int* duplicate;
    // the workspace
    double* origin;                              // [S, 3]
    int* table;                                  // [S, G]: the smallest vertex index of the cell, INT_MAX for none
    int* cellof;                                 // [S, cap]: the vertex's cell, -1 for a dropped vertex
    long long* acc;                              // [S, cap, kDcAcc]: row k of a scene belongs to its cluster k
    int* blk_v;                                  // [S, nblk_v]
    int* blk_t;                                  // [S, nblk_t]
    int* tstate;                                 // [S, cap_tri]: a negative class, or the candidate's slot in row_key (0 without dedupe)
    unsigned long long* pair_key;                // [S, P]: (a, b) of the rotated candidates
    unsigned long long* row_key;                 // [S, P]: (slot of (a, b), c)
    int* row_min;                                // [S, P]: the lowest row with that key
};

struct DcOrigin {
    double v[kDcOriginScenes * 3];
};

__device__ __forceinline__ int dc_clamp(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__global__ __launch_bounds__(64) void dc_origin_kernel(double* dst, DcOrigin o, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = o.v[threadIdx.x];
}

__global__ __launch_bounds__(kDcTile) void dc_init_kernel(DcBufs b, unsigned S) {
    const size_t first = (size_t)blockIdx.x * kDcTile + threadIdx.x, stride = (size_t)gridDim.x * kDcTile;
    const size_t n_table = (size_t)S * b.G, n_hash = b.dedupe ? (size_t)S * b.P : 0;
    for (size_t i = first; i < n_table; i += stride) b.table[i] = INT_MAX;
    for (size_t i = first; i < n_hash; i += stride) {
        b.pair_key[i] = kDcEmpty;
        b.row_key[i] = kDcEmpty;
        b.row_min[i] = INT_MAX;
    }
    for (size_t i = first; i < S; i += stride) {
        b.bad[i] = 0; b.outside[i] = 0; b.degenerate[i] = 0; b.duplicate[i] = 0;
    }
}

// u_a = (p_a - origin_a) / cell; inside iff every u_a is finite and 0 <= floor(u_a) < g_a -> the cell's index in the scene's table
__device__ __forceinline__ bool dc_cell_of(const DcBufs& b, unsigned s, const double* p, double u[3], int& cell) {
    const double* org = b.origin + 3 * s;
    const int g[3] = {b.gx, b.gy, b.gz};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = (p[a] - org[a]) / b.cell;
        const double f = floor(u[a]);
        if (!(isfinite(u[a]) && f >= 0.0 && f < (double)g[a])) return false;
        c[a] = (int)f;
    }
    cell = (c[2] * b.gy + c[1]) * b.gx + c[0];                                   // < G < 2^27
    return true;
}

__global__ __launch_bounds__(kDcTile) void dc_cell_kernel(DcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kDcTile + threadIdx.x;
    if (e >= (unsigned)b.cap) return;
    const size_t o = (size_t)s * b.cap + e;
    double u[3];
    int cell = -1;
    if (e >= (unsigned)dc_clamp(b.n_pts[s], b.cap) || !dc_cell_of(b, s, b.points + o * 3, u, cell)) cell = -1;
    b.cellof[o] = cell;
    if (cell >= 0) atomicMin(b.table + (size_t)s * b.G + cell, (int)e);
}

__device__ __forceinline__ bool dc_is_rep(const DcBufs& b, unsigned s, unsigned e) {
    if (e >= (unsigned)b.cap) return false;
    const int c = b.cellof[(size_t)s * b.cap + e];
    return c >= 0 && b.table[(size_t)s * b.G + c] == (int)e;
}

__global__ __launch_bounds__(kDcTile) void dc_rep_count_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    int total;
    rp_block_rank(dc_is_rep(b, s, blk * kDcTile + threadIdx.x), s_wsum, total);
    if (threadIdx.x == 0) b.blk_v[(size_t)s * b.nblk_v + blk] = total;
}

// One workgroup of kDcScanThreads threads: the exclusive scan of cnt[0 .. n) in place -> the total (in every thread)
__device__ __forceinline__ int dc_scan_counts(int* cnt, unsigned n, int* s_wsum) {
    int run = 0;
    for (unsigned b0 = 0; b0 < n; b0 += kDcScanThreads) {
        const unsigned x = b0 + threadIdx.x;
        const int v = x < n ? cnt[x] : 0;
        int total;
        const int ex = rp_block_excl_scan(v, s_wsum, total);
        if (x < n) cnt[x] = run + ex;
        run += total;
    }
    return run;
}

__global__ __launch_bounds__(kDcScanThreads) void dc_rep_scan_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int n = dc_scan_counts(b.blk_v + (size_t)s * b.nblk_v, b.nblk_v, s_wsum);
    if (threadIdx.x == 0) b.o_n_pts[s] = n;                                      // <= cap
}

// vertex_map of the representatives (their rank), their accumulator rows cleared; out_valid
__global__ __launch_bounds__(kDcTile) void dc_rep_write_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kDcTile + threadIdx.x;
    const bool rep = dc_is_rep(b, s, e);
    int total;
    const int rank = b.blk_v[(size_t)s * b.nblk_v + blk] + rp_block_rank(rep, s_wsum, total);
    if (e >= (unsigned)b.cap) return;
    b.o_valid[(size_t)s * b.cap + e] = (uint8_t)((int)e < b.o_n_pts[s]);         // the scan's launch wrote it
    if (!rep) return;
    b.vmap[(size_t)s * b.cap + e] = rank;                                        // rank <= e < cap
    long long* row = b.acc + ((size_t)s * b.cap + rank) * kDcAcc;
#pragma unroll
    for (int k = 0; k < kDcAcc; ++k) row[k] = 0;
}

// Adds v[0 .. n) of every lane whose cluster c is >= 0 to row c of acc.  All 64 lanes call.  A run of equal c in consecutive lanes is summed
// by a segmented scan and added once, by its last lane.  The sums are integers: the result does not depend on where the runs fall.
__device__ __forceinline__ void dc_run_add(int c, long long (&v)[kDcAcc], int n, long long* acc) {
    const int lane = rp_lane();
    const int prev = __shfl_up(c, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != c);          // bit 0 is set
    if (heads != ~0ull) {                                                        // (wave-uniform) some run is longer than one lane
        const int start = 63 - __clzll((long long)(heads & (rp_lanes_below() | 1ull << lane)));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int k = 0; k < kDcAcc; ++k) {
                const long long y = __shfl_up(v[k], o, 64);
                if (lane - o >= start) v[k] += y;
            }
        }
    }
    const bool last = lane == 63 || (heads >> (lane + 1) & 1ull);
    if (!last || c < 0) return;
    unsigned long long* row = (unsigned long long*)acc + (size_t)c * kDcAcc;
#pragma unroll
    for (int k = 0; k < kDcAcc; ++k)
        if (k < n || k == kDcAcc - 1) atomicAdd(row + k, (unsigned long long)v[k]);
}

__global__ __launch_bounds__(kDcTile) void dc_accumulate_kernel(DcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kDcTile + threadIdx.x;
    long long v[kDcAcc] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int c = -1;
    if (e < (unsigned)b.cap) {
        const size_t o = (size_t)s * b.cap + e;
        const int cell = b.cellof[o];
        if (cell >= 0) {
            const int rep = b.table[(size_t)s * b.G + cell];                     // in [0, e]
            c = b.vmap[(size_t)s * b.cap + rep];                                 // a representative's entry: written by the launch before
            if (rep != (int)e) b.vmap[o] = c;
            double u[3];
            int again;
            dc_cell_of(b, s, b.points + o * 3, u, again);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[a] = llrint(u[a] * 65536.0);                                   // 0 <= u < 1024
                const double nn = b.normals[o * 3 + a];
                v[3 + a] = (isfinite(nn) && fabs(nn) <= 65536.0) ? llrint(nn * 32768.0) : 0;
                if (b.colors) {
                    const double cc = (double)b.colors[o * 3 + a];
                    v[6 + a] = isnan(cc) ? 0 : llrint((cc < 0.0 ? 0.0 : (cc > 1.0 ? 1.0 : cc)) * 65535.0);
                }
            }
            v[9] = 1;
        } else {
            b.vmap[o] = -1;
        }
    }
    dc_run_add(c, v, b.colors ? 9 : 6, b.acc + (size_t)s * b.cap * kDcAcc);
}

__global__ __launch_bounds__(kDcTile) void dc_finalize_kernel(DcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned k = blk * kDcTile + threadIdx.x;
    if (k >= (unsigned)b.cap || (int)k >= b.o_n_pts[s]) return;
    const size_t o = (size_t)s * b.cap + k;
    const long long* row = b.acc + o * kDcAcc;
    const double* org = b.origin + 3 * s;
    const double n = (double)row[9];                                             // >= 1
    const double sn[3] = {(double)row[3], (double)row[4], (double)row[5]};
    const double len = sqrt((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.o_points[o * 3 + a] = org[a] + ((double)row[a] / (65536.0 * n)) * b.cell;
        b.o_normals[o * 3 + a] = len == 0.0 ? 0.0 : sn[a] / len;
        if (b.o_colors) b.o_colors[o * 3 + a] = (float)((double)row[6 + a] / (65535.0 * n));
    }
    b.o_count[o] = (int)row[9];
}

__device__ __forceinline__ unsigned dc_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k;
}

// The slot of `key` in an open-addressing table of P slots (a power of two): the first slot from the key's hash on that is empty (it is
// taken) or holds the key.  At most P probes; -1 if none is found, which a table with fewer keys than slots does not do.
__device__ __forceinline__ int dc_slot(unsigned long long* tab, unsigned P, unsigned long long key) {
    unsigned h = dc_hash(key) & (P - 1);
    for (unsigned i = 0; i < P; ++i) {
        const unsigned long long was = atomicCAS(tab + h, kDcEmpty, key);
        if (was == kDcEmpty || was == key) return (int)h;
        h = (h + 1) & (P - 1);
    }
    return -1;
}

__global__ __launch_bounds__(kDcTile) void dc_tri_kernel(DcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_t, blk = blockIdx.x - s * b.nblk_t;
    const unsigned t = blk * kDcTile + threadIdx.x;
    const int nt = dc_clamp(b.n_tri[s], b.cap_tri), nv = dc_clamp(b.n_pts[s], b.cap);
    int state = kDcBeyond;
    if (t < (unsigned)nt) {
        const int* r = b.tri + ((size_t)s * b.cap_tri + t) * 3;
        const int i0 = r[0], i1 = r[1], i2 = r[2];
        if (!((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv)) {
            state = kDcBad;
        } else {
            const int* m = b.vmap + (size_t)s * b.cap;
            const int m0 = m[i0], m1 = m[i1], m2 = m[i2];
            if (m0 < 0 || m1 < 0 || m2 < 0) {
                state = kDcOutside;
            } else if (m0 == m1 || m1 == m2 || m0 == m2) {
                state = kDcDegenerate;
            } else if (!b.dedupe) {
                state = 0;
            } else {
                int x, y, z;                                                     // the rotation that puts the smallest index first
                if (m0 < m1 && m0 < m2) { x = m0; y = m1; z = m2; }
                else if (m1 < m2) { x = m1; y = m2; z = m0; }
                else { x = m2; y = m0; z = m1; }
                state = kDcNoSlot;
                const int p = dc_slot(b.pair_key + (size_t)s * b.P, b.P, (unsigned long long)(unsigned)x << 32 | (unsigned)y);
                if (p >= 0) {
                    const int q = dc_slot(b.row_key + (size_t)s * b.P, b.P, (unsigned long long)(unsigned)p << 32 | (unsigned)z);
                    if (q >= 0) {
                        atomicMin(b.row_min + (size_t)s * b.P + q, (int)t);
                        state = q;
                    }
                }
            }
        }
    }
    if (t < (unsigned)b.cap_tri) b.tstate[(size_t)s * b.cap_tri + t] = state;
    const int n_bad = __popcll(__ballot(state == kDcBad)), n_out = __popcll(__ballot(state == kDcOutside));
    const int n_deg = __popcll(__ballot(state == kDcDegenerate));
    if (rp_lane() == 0) {
        if (n_bad) atomicAdd(b.bad + s, n_bad);
        if (n_out) atomicAdd(b.outside + s, n_out);
        if (n_deg) atomicAdd(b.degenerate + s, n_deg);
    }
}

// -> the row survives; dup: it is a candidate that lost to a lower row
__device__ __forceinline__ bool dc_tri_survives(const DcBufs& b, unsigned s, unsigned t, int& state, bool& dup) {
    dup = false;
    state = kDcBeyond;
    if (t >= (unsigned)b.cap_tri) return false;
    state = b.tstate[(size_t)s * b.cap_tri + t];
    if (state < 0) return false;
    if (!b.dedupe || state == kDcNoSlot) return true;
    dup = b.row_min[(size_t)s * b.P + state] != (int)t;
    return !dup;
}

__global__ __launch_bounds__(kDcTile) void dc_tri_count_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_t, blk = blockIdx.x - s * b.nblk_t;
    int state, total;
    bool dup;
    rp_block_rank(dc_tri_survives(b, s, blk * kDcTile + threadIdx.x, state, dup), s_wsum, total);
    if (threadIdx.x == 0) b.blk_t[(size_t)s * b.nblk_t + blk] = total;
    const int n_dup = __popcll(__ballot(dup));
    if (n_dup && rp_lane() == 0) atomicAdd(b.duplicate + s, n_dup);
}

__global__ __launch_bounds__(kDcScanThreads) void dc_tri_scan_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int n = dc_scan_counts(b.blk_t + (size_t)s * b.nblk_t, b.nblk_t, s_wsum);
    if (threadIdx.x == 0) b.o_n_tri[s] = n;                                      // <= cap_tri
}

__global__ __launch_bounds__(kDcTile) void dc_tri_write_kernel(DcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_t, blk = blockIdx.x - s * b.nblk_t;
    const unsigned t = blk * kDcTile + threadIdx.x;
    int state, total;
    bool dup;
    const bool stays = dc_tri_survives(b, s, t, state, dup);
    const int at = b.blk_t[(size_t)s * b.nblk_t + blk] + rp_block_rank(stays, s_wsum, total);
    if (t >= (unsigned)b.cap_tri) return;
    if (b.tmap) b.tmap[(size_t)s * b.cap_tri + t] = stays ? at : (dup ? kDcDuplicate : state);
    if (!stays) return;
    const int* r = b.tri + ((size_t)s * b.cap_tri + t) * 3;                       // a candidate: its indices are in [0, nv)
    int* o = b.o_tri + ((size_t)s * b.cap_tri + at) * 3;                          // at <= t < cap_tri
#pragma unroll
    for (int x = 0; x < 3; ++x) o[x] = b.vmap[(size_t)s * b.cap + r[x]];
}

unsigned dc_blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

bool dc_sizes_ok(long long S, long long cap, long long cap_tri, long long gx, long long gy, long long gz) {
    if (!(S >= 1 && cap >= 1 && cap_tri >= 1 && S * cap < (1ll << 29) && S * cap_tri < (1ll << 29))) return false;
    if (gx < 1 || gy < 1 || gz < 1 || gx > 1024 || gy > 1024 || gz > 1024) return false;
    return S * gx * gy * gz < (1ll << 27);
}

unsigned dc_slots(int cap_tri) {                                                  // the power of two >= 2 cap_tri (cap_tri < 2^29)
    unsigned p = 2;
    while (p < 2u * (unsigned)cap_tri) p <<= 1;
    return p;
}

size_t carve_dc(int S, int cap, int cap_tri, long long G, char* base, DcBufs& b) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    const size_t P = dc_slots(cap_tri);
    b.origin = (double*)take((size_t)S * 3 * sizeof(double));
    b.table = (int*)take((size_t)S * G * sizeof(int));
    b.cellof = (int*)take((size_t)S * cap * sizeof(int));
    b.acc = (long long*)take((size_t)S * cap * kDcAcc * sizeof(long long));
    b.blk_v = (int*)take((size_t)S * dc_blocks_of(cap, kDcTile) * sizeof(int));
    b.blk_t = (int*)take((size_t)S * dc_blocks_of(cap_tri, kDcTile) * sizeof(int));
    b.tstate = (int*)take((size_t)S * cap_tri * sizeof(int));
    b.pair_key = (unsigned long long*)take((size_t)S * P * sizeof(unsigned long long));
    b.row_key = (unsigned long long*)take((size_t)S * P * sizeof(unsigned long long));
    b.row_min = (int*)take((size_t)S * P * sizeof(int));
    return off;
}

}  // namespace

extern "C" size_t relpose_mesh_decimate_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri, int32_t gx, int32_t gy, int32_t gz) {
    if (!dc_sizes_ok(n_scenes, cap, cap_tri, gx, gy, gz)) return 0;
    DcBufs b{};
    return carve_dc(n_scenes, cap, cap_tri, (long long)gx * gy * gz, nullptr, b);
}

extern "C" int relpose_mesh_decimate(const RelposeMeshDecimateArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeMeshDecimateArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeMeshDecimateArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeMeshDecimateArgs)));
    if (!a.points || !a.normals || !a.n_points || !a.triangles || !a.n_triangles || !a.origin_host || !a.out_points || !a.out_normals ||
        !a.out_valid || !a.out_n_points || !a.out_count || !a.out_triangles || !a.out_n_triangles || !a.vertex_map || !a.bad_triangles ||
        !a.outside_triangles || !a.degenerate_triangles || !a.duplicate_triangles || !a.workspace)
        return RELPOSE_EINVAL;
    if ((a.colors == nullptr) != (a.out_colors == nullptr)) return RELPOSE_EINVAL;
    if (!dc_sizes_ok(a.n_scenes, a.cap, a.cap_tri, a.gx, a.gy, a.gz)) return RELPOSE_EINVAL;
    if (!(std::isfinite(a.cell) && a.cell > 0.0) || (a.dedupe != 0 && a.dedupe != 1)) return RELPOSE_EINVAL;
    for (int e = 0; e < 3 * a.n_scenes; ++e)
        if (!std::isfinite(a.origin_host[e])) return RELPOSE_EINVAL;
    if (a.out_points == a.points || a.out_normals == a.normals || a.out_points == a.normals || a.out_normals == a.points ||
        (a.colors && a.out_colors == a.colors) || a.out_triangles == a.triangles || a.out_n_points == a.n_points ||
        a.out_n_triangles == a.n_triangles || a.out_n_points == a.n_triangles || a.out_n_triangles == a.n_points)
        return RELPOSE_EINVAL;                                                    // the outputs are buffers of their own
    DcBufs b{};
    const long long G = (long long)a.gx * a.gy * a.gz;
    if (a.workspace_bytes < carve_dc(a.n_scenes, a.cap, a.cap_tri, G, nullptr, b) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_dc(a.n_scenes, a.cap, a.cap_tri, G, (char*)a.workspace, b);
    b.cap = a.cap; b.cap_tri = a.cap_tri; b.gx = a.gx; b.gy = a.gy; b.gz = a.gz; b.dedupe = a.dedupe;
    b.G = (unsigned)G; b.P = dc_slots(a.cap_tri);
    b.nblk_v = dc_blocks_of(a.cap, kDcTile); b.nblk_t = dc_blocks_of(a.cap_tri, kDcTile);
    b.cell = a.cell;
    b.points = a.points; b.normals = a.normals; b.colors = a.colors; b.n_pts = a.n_points; b.tri = a.triangles; b.n_tri = a.n_triangles;
    b.o_points = a.out_points; b.o_normals = a.out_normals; b.o_colors = a.out_colors; b.o_valid = a.out_valid; b.o_n_pts = a.out_n_points;
    b.o_count = a.out_count; b.o_tri = a.out_triangles; b.o_n_tri = a.out_n_triangles; b.vmap = a.vertex_map; b.tmap = a.tri_map;
    b.bad = a.bad_triangles; b.outside = a.outside_triangles; b.degenerate = a.degenerate_triangles; b.duplicate = a.duplicate_triangles;
    hipStream_t s = (hipStream_t)a.stream;
    const unsigned S = (unsigned)a.n_scenes, grid_v = S * b.nblk_v, grid_t = S * b.nblk_t;
    for (int s0 = 0; s0 < a.n_scenes; s0 += kDcOriginScenes) {
        DcOrigin o{};
        const int n = 3 * std::min(kDcOriginScenes, a.n_scenes - s0);
        memcpy(o.v, a.origin_host + 3 * (size_t)s0, n * sizeof(double));
        hipLaunchKernelGGL(dc_origin_kernel, dim3(1), dim3(64), 0, s, b.origin + 3 * (size_t)s0, o, n);
    }
    const size_t n_init = std::max((size_t)S * b.G, b.dedupe ? (size_t)S * b.P : (size_t)S);
    hipLaunchKernelGGL(dc_init_kernel, dim3(std::min(dc_blocks_of((long long)n_init, kDcTile), (unsigned)kDcInitBlocks)), dim3(kDcTile), 0, s, b, S);
    hipLaunchKernelGGL(dc_cell_kernel, dim3(grid_v), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_rep_count_kernel, dim3(grid_v), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_rep_scan_kernel, dim3(S), dim3(kDcScanThreads), 0, s, b);
    hipLaunchKernelGGL(dc_rep_write_kernel, dim3(grid_v), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_accumulate_kernel, dim3(grid_v), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_finalize_kernel, dim3(grid_v), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_tri_kernel, dim3(grid_t), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_tri_count_kernel, dim3(grid_t), dim3(kDcTile), 0, s, b);
    hipLaunchKernelGGL(dc_tri_scan_kernel, dim3(S), dim3(kDcScanThreads), 0, s, b);
    hipLaunchKernelGGL(dc_tri_write_kernel, dim3(grid_t), dim3(kDcTile), 0, s, b);
    RP_CHECK_LAUNCH();
    return 0;
}
