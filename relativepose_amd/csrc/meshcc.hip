// Connected components of indexed triangle meshes, and the compaction that drops the ones a caller does not keep (the
// contract stands above relpose_mesh_components / relpose_mesh_filter in include/relpose.h, tests/components_model.py restates it in numpy).
// Built with -ffp-contract=off: the area of a triangle rounds as the model's.  Every result is an integer, and a component's label is its
// smallest vertex index, so the outputs are bitwise independent of the order the hardware works in, of the batch and of repeats.
//
// Labelling is monotone lowering, NOT a single-launch union-find: L[v] starts at v and is only ever written by a device-scope atomicMin of a
// label of v's own component, so L[v] <= v and L[v] stays inside the component whatever a thread read.  A read that returns an older value
// returns a larger label of the same component: it can cost a round, never a wrong answer.  Nothing waits on another workgroup; a launch
// sees all that earlier launches wrote.  One round is two launches:
//   cc_hook_kernel    per good triangle m = min(L[a], L[b], L[c]); atomicMin of m into L[a], L[b], L[c] and L[L[a]], L[L[b]], L[L[c]] (an
//                     entry read as m already is skipped: it cannot be above m)
//   cc_jump_kernel    per vertex L[v] <- the end of the chain L[L[...]] as far as it descends
// A thread whose atomicMin returned more than it wrote sets the round's flag; the host reads the flags of kCcGroup rounds at a time and
// stops at the first round that set none.  If the state at a round's start is not the fixpoint some atomicMin of the round lowers an entry
// (reads within the first launch see at least what the launches before wrote), so an unset flag means: equal labels on every good triangle
// and L[v] == L[L[v]], which is L constant on every component and equal to its smallest index.
//   cc_init_kernel    L[v] = v, used = 0, the statistics cleared        cc_mark_kernel   used[] of a good triangle's vertices, bad rows counted
//   cc_root_*         roots (used and L[v] == v) flagged, counted per workgroup, scanned per scene, numbered in ascending order
//   cc_vertex_kernel  vertex_label and comp_vertices                    cc_triangle_kernel  tri_label, comp_triangles and comp_area
// Statistics are integer atomicAdds.  In a room nearly every triangle belongs to one component, so the adds of a run of equal labels are
// summed inside the wave first (cc_run_add), and the runs of the component a workgroup meets first are summed in LDS over the kCcStatTiles
// tiles of the workgroup: one global add per workgroup instead of one per triangle (profiles/components_time.txt has both).
//   filter_count / filter_scan / filter_vertex / filter_triangle   flag, scan per scene, scatter: no atomics, rows copied bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "cloud_prims.h"
#include "common.h"

namespace {

constexpr int kCcTile = 256;                     // vertices or triangles per workgroup
constexpr int kCcScanThreads = 1024;
constexpr int kCcGroup = 4;                      // rounds enqueued between two reads of the flags
constexpr int kCcStatTiles = 8;                  // tiles a workgroup of the two statistics kernels walks

struct CcBufs {
    int cap, cap_tri, cap_comp;
    unsigned nblk_v, nblk_t;                     // workgroups per scene over the vertices and over the triangles
    unsigned nstat_v, nstat_t;                   // the same for the statistics kernels (kCcStatTiles tiles each)
    const int* tri;                              // [S, cap_tri, 3]
    const int* n_tri;                            // [S]
    const int* n_pts;                            // [S]
    const double* points;                        // [S, cap, 3] or null
    double area_scale;
    int* L;                                      // [S, cap]
    uint8_t* used;                               // [S, cap]
    int* blk;                                    // [S, nblk_v]: roots per workgroup, then their exclusive scan
    int* flags;                                  // [kCcGroup]
    int* vlabel;                                 // [S, cap]
    int* tlabel;                                 // [S, cap_tri]
    int* n_comp;                                 // [S]
    int* bad;                                    // [S]
    int* c_root;                                 // [S, cap_comp] each, or null with cap_comp = 0
    int* c_vert;
    int* c_tri;
    unsigned long long* c_area;
};

__device__ __forceinline__ int cc_clamp(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// a label as the L2 holds it (a relaxed device-scope load bypasses this CU's L1: fewer rounds lost to old values)
__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// row t of scene s: 1 = good (v[] its indices, all in [0, nv)), 0 = bad, -1 = beyond the scene's triangles
__device__ __forceinline__ int cc_row(const CcBufs& b, unsigned s, unsigned t, int v[3]) {
    const int nt = cc_clamp(b.n_tri[s], b.cap_tri), nv = cc_clamp(b.n_pts[s], b.cap);
    if (t >= (unsigned)nt) return -1;
    const int* r = b.tri + ((size_t)s * b.cap_tri + t) * 3;
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2];
    return (unsigned)v[0] < (unsigned)nv && (unsigned)v[1] < (unsigned)nv && (unsigned)v[2] < (unsigned)nv;
}

__global__ __launch_bounds__(kCcTile) void cc_init_kernel(CcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kCcTile + threadIdx.x;
    if (e < (unsigned)b.cap) {
        b.L[(size_t)s * b.cap + e] = (int)e;
        b.used[(size_t)s * b.cap + e] = 0;
    }
    for (unsigned c = e; c < (unsigned)b.cap_comp; c += b.nblk_v * kCcTile) {
        const size_t o = (size_t)s * b.cap_comp + c;
        b.c_root[o] = -1; b.c_vert[o] = 0; b.c_tri[o] = 0; b.c_area[o] = 0ull;
    }
    if (e == 0) b.bad[s] = 0;
}

__global__ __launch_bounds__(kCcTile) void cc_mark_kernel(CcBufs b) {
    const unsigned s = blockIdx.x / b.nblk_t, blk = blockIdx.x - s * b.nblk_t;
    int v[3];
    const int g = cc_row(b, s, blk * kCcTile + threadIdx.x, v);
    if (g == 1) {
        uint8_t* u = b.used + (size_t)s * b.cap;
        u[v[0]] = 1; u[v[1]] = 1; u[v[2]] = 1;
    }
    const int nb = __popcll(__ballot(g == 0));
    if (nb && rp_lane() == 0) atomicAdd(b.bad + s, nb);
}

__global__ __launch_bounds__(kCcTile) void cc_hook_kernel(CcBufs b, int* flag) {
    const unsigned s = blockIdx.x / b.nblk_t, blk = blockIdx.x - s * b.nblk_t;
    int v[3];
    if (cc_row(b, s, blk * kCcTile + threadIdx.x, v) != 1) return;
    int* L = b.L + (size_t)s * b.cap;
    const int l[3] = {cc_ld(L + v[0]), cc_ld(L + v[1]), cc_ld(L + v[2])};       // each in [0, v]: an index of this scene
    const int m = min(l[0], min(l[1], l[2]));
    bool lowered = false;
#pragma unroll
    for (int x = 0; x < 3; ++x)
        if (l[x] != m) {                                                          // L[v] <= l and L[l] <= l: nothing to lower where l == m
            lowered |= atomicMin(L + v[x], m) > m;
            lowered |= atomicMin(L + l[x], m) > m;
        }
    if (lowered) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kCcTile) void cc_jump_kernel(CcBufs b, int* flag) {
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kCcTile + threadIdx.x;
    if (e >= (unsigned)cc_clamp(b.n_pts[s], b.cap)) return;
    int* L = b.L + (size_t)s * b.cap;
    const int l0 = cc_ld(L + e);
    int l = l0;
    for (int n = cc_ld(L + l); n < l; n = cc_ld(L + l)) l = n;                   // strictly descending: at most l0 steps
    if (l < l0 && atomicMin(L + e, l) > l) atomicOr(flag, 1);
}

__device__ __forceinline__ bool cc_is_root(const CcBufs& b, unsigned s, unsigned e) {
    if (e >= (unsigned)cc_clamp(b.n_pts[s], b.cap)) return false;
    const size_t o = (size_t)s * b.cap + e;
    return b.used[o] && b.L[o] == (int)e;
}

__global__ __launch_bounds__(kCcTile) void cc_root_count_kernel(CcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    int total;
    rp_block_rank(cc_is_root(b, s, blk * kCcTile + threadIdx.x), s_wsum, total);
    if (threadIdx.x == 0) b.blk[(size_t)s * b.nblk_v + blk] = total;
}

// One workgroup of kCcScanThreads threads: the exclusive scan of cnt[0 .. n) in place -> the total (in every thread)
__device__ __forceinline__ int cc_scan_counts(int* cnt, unsigned n, int* s_wsum) {
    int run = 0;
    for (unsigned b0 = 0; b0 < n; b0 += kCcScanThreads) {
        const unsigned x = b0 + threadIdx.x;
        const int v = x < n ? cnt[x] : 0;
        int total;
        const int ex = rp_block_excl_scan(v, s_wsum, total);
        if (x < n) cnt[x] = run + ex;
        run += total;
    }
    return run;
}

__global__ __launch_bounds__(kCcScanThreads) void cc_root_scan_kernel(CcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int n = cc_scan_counts(b.blk + (size_t)s * b.nblk_v, b.nblk_v, s_wsum);
    if (threadIdx.x == 0) b.n_comp[s] = n;                                       // <= cap
}

// vertex_label of the roots (their rank) and -1 everywhere else; comp_root
__global__ __launch_bounds__(kCcTile) void cc_root_write_kernel(CcBufs b) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / b.nblk_v, blk = blockIdx.x - s * b.nblk_v;
    const unsigned e = blk * kCcTile + threadIdx.x;
    const bool root = cc_is_root(b, s, e);
    int total;
    const int rank = b.blk[(size_t)s * b.nblk_v + blk] + rp_block_rank(root, s_wsum, total);
    if (e < (unsigned)b.cap) b.vlabel[(size_t)s * b.cap + e] = root ? rank : -1;
    if (root && rank < b.cap_comp) b.c_root[(size_t)s * b.cap_comp + rank] = (int)e;
}

struct CcAcc {                                   // LDS: the sums of the component a workgroup met first
    int comp, n;
    unsigned long long w;
};

// Adds (n, w) of every lane whose component c is in [0, cap_comp) to cnt[c] and, where area is not null, area[c].  All 64 lanes call.  A run of
// equal c in consecutive lanes is summed by a segmented scan and added once, by its last lane: into acc if acc's component is c (or acc is
// still free), else into memory.  The sums are integers: the result does not depend on which component acc took.
__device__ __forceinline__ void cc_run_add(int c, int n, long long w, int cap_comp, int* cnt, unsigned long long* area, CcAcc* acc) {
    const int lane = rp_lane();
    const int prev = __shfl_up(c, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != c);          // bit 0 is set
    const int start = 63 - __clzll((long long)(heads & (rp_lanes_below() | 1ull << lane)));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int yn = __shfl_up(n, o, 64);
        const long long yw = __shfl_up(w, o, 64);
        if (lane - o >= start) { n += yn; w += yw; }
    }
    const bool last = lane == 63 || (heads >> (lane + 1) & 1ull);
    if (!last || c < 0 || c >= cap_comp) return;
    const int own = atomicCAS(&acc->comp, -1, c);
    if (own == -1 || own == c) {
        atomicAdd(&acc->n, n);
        if (area) atomicAdd(&acc->w, (unsigned long long)w);
    } else {
        atomicAdd(cnt + c, n);
        if (area) atomicAdd(area + c, (unsigned long long)w);
    }
}

__device__ __forceinline__ void cc_acc_flush(const CcAcc* acc, int* cnt, unsigned long long* area) {
    if (acc->comp < 0) return;
    atomicAdd(cnt + acc->comp, acc->n);
    if (area) atomicAdd(area + acc->comp, acc->w);
}

__global__ __launch_bounds__(kCcTile) void cc_vertex_kernel(CcBufs b) {
    __shared__ CcAcc s_acc;
    const unsigned s = blockIdx.x / b.nstat_v, blk = blockIdx.x - s * b.nstat_v;
    if (threadIdx.x == 0) { s_acc.comp = -1; s_acc.n = 0; s_acc.w = 0ull; }
    __syncthreads();
    const int nv = cc_clamp(b.n_pts[s], b.cap);
    int* lab = b.vlabel + (size_t)s * b.cap;
    for (int q = 0; q < kCcStatTiles; ++q) {
        const unsigned e = (blk * kCcStatTiles + q) * kCcTile + threadIdx.x;
        int c = -1;
        if (e < (unsigned)nv && b.used[(size_t)s * b.cap + e]) {
            const int l = b.L[(size_t)s * b.cap + e];
            c = lab[l];                                                          // a root's entry: written by the launch before, not by this one
            if (l != (int)e) lab[e] = c;
        }
        cc_run_add(c, 1, 0, b.cap_comp, b.c_vert + (size_t)s * b.cap_comp, nullptr, &s_acc);
    }
    __syncthreads();
    if (threadIdx.x == 0) cc_acc_flush(&s_acc, b.c_vert + (size_t)s * b.cap_comp, nullptr);
}

// llrint(min(A area_scale, 2^31)) with A = sqrt((cx cx + cy cy) + cz cz) 0.5 and c = (p1 - p0) x (p2 - p0); 0 where the product is not finite
__device__ __forceinline__ long long cc_area(const double* p, const int v[3], double scale) {
    const double* p0 = p + (size_t)v[0] * 3;
    const double* p1 = p + (size_t)v[1] * 3;
    const double* p2 = p + (size_t)v[2] * 3;
    const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, w[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    double c[3];
    rp_cross3(u, w, c);
    const double a = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) * 0.5;
    const double q = a * scale;
    if (!isfinite(q)) return 0;
    return llrint(fmin(q, 2147483648.0));
}

__global__ __launch_bounds__(kCcTile) void cc_triangle_kernel(CcBufs b) {
    __shared__ CcAcc s_acc;
    const unsigned s = blockIdx.x / b.nstat_t, blk = blockIdx.x - s * b.nstat_t;
    if (threadIdx.x == 0) { s_acc.comp = -1; s_acc.n = 0; s_acc.w = 0ull; }
    __syncthreads();
    const int* lab = b.vlabel + (size_t)s * b.cap;
    unsigned long long* area = b.points ? b.c_area + (size_t)s * b.cap_comp : nullptr;
    for (int q = 0; q < kCcStatTiles; ++q) {
        const unsigned t = (blk * kCcStatTiles + q) * kCcTile + threadIdx.x;
        int v[3], c = -1;
        long long w = 0;
        if (cc_row(b, s, t, v) == 1) {
            c = lab[v[0]];
            if (area && c < b.cap_comp) w = cc_area(b.points + (size_t)s * b.cap * 3, v, b.area_scale);
        }
        if (t < (unsigned)b.cap_tri) b.tlabel[(size_t)s * b.cap_tri + t] = c;
        cc_run_add(c, 1, w, b.cap_comp, b.c_tri + (size_t)s * b.cap_comp, area, &s_acc);
    }
    __syncthreads();
    if (threadIdx.x == 0) cc_acc_flush(&s_acc, b.c_tri + (size_t)s * b.cap_comp, area);
}

unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

size_t carve_cc(int S, int cap, char* base, CcBufs& b) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    b.flags = (int*)take(kCcGroup * sizeof(int));
    b.blk = (int*)take((size_t)S * blocks_of(cap, kCcTile) * sizeof(int));
    b.L = (int*)take((size_t)S * cap * sizeof(int));
    b.used = (uint8_t*)take((size_t)S * cap);
    return off;
}

bool cc_sizes_ok(long long S, long long cap, long long cap_tri) {
    return S >= 1 && cap >= 1 && cap_tri >= 1 && S * cap < (1ll << 29) && S * cap_tri < (1ll << 29);
}

// ---------------------------------------------------------------------------------------------------------------- the filter
struct FilterBufs {
    int cap, cap_tri, cap_comp, drop_unused;
    unsigned nblk_v, nblk_t;
    const double* points;
    const double* normals;
    const float* colors;                         // or null
    const int* n_pts;
    const int* tri;
    const int* n_tri;
    const int* vlabel;
    const int* tlabel;
    const uint8_t* keep;                         // [S, cap_comp]
    double* o_points;
    double* o_normals;
    float* o_colors;
    uint8_t* o_valid;
    int* o_n_pts;
    int* o_tri;
    int* o_n_tri;
    int* map;                                    // [S, cap]: the caller's vertex_map or the workspace's
    int* blk_v;                                  // [S, nblk_v]
    int* blk_t;                                  // [S, nblk_t]
};

__device__ __forceinline__ bool filter_kept(const FilterBufs& f, unsigned s, int label) {
    return (unsigned)label < (unsigned)f.cap_comp && f.keep[(size_t)s * f.cap_comp + label] != 0;
}

__device__ __forceinline__ bool filter_vertex_stays(const FilterBufs& f, unsigned s, unsigned e) {
    if (e >= (unsigned)cc_clamp(f.n_pts[s], f.cap)) return false;
    const int c = f.vlabel[(size_t)s * f.cap + e];
    return c < 0 ? !f.drop_unused : filter_kept(f, s, c);
}

__device__ __forceinline__ bool filter_triangle_stays(const FilterBufs& f, unsigned s, unsigned t) {
    return t < (unsigned)cc_clamp(f.n_tri[s], f.cap_tri) && filter_kept(f, s, f.tlabel[(size_t)s * f.cap_tri + t]);
}

// workgroups [0, nblk_v) of a scene count its surviving vertices, [nblk_v, nblk_v + nblk_t) its surviving triangles
__global__ __launch_bounds__(kCcTile) void filter_count_kernel(FilterBufs f) {
    __shared__ int s_wsum[16];
    const unsigned per = f.nblk_v + f.nblk_t, s = blockIdx.x / per, blk = blockIdx.x - s * per;
    const bool vert = blk < f.nblk_v;
    const unsigned k = vert ? blk : blk - f.nblk_v, e = k * kCcTile + threadIdx.x;
    int total;
    rp_block_rank(vert ? filter_vertex_stays(f, s, e) : filter_triangle_stays(f, s, e), s_wsum, total);
    if (threadIdx.x == 0) (vert ? f.blk_v + (size_t)s * f.nblk_v : f.blk_t + (size_t)s * f.nblk_t)[k] = total;
}

__global__ __launch_bounds__(kCcScanThreads) void filter_scan_kernel(FilterBufs f) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x;
    const int nv = cc_scan_counts(f.blk_v + (size_t)s * f.nblk_v, f.nblk_v, s_wsum);
    const int nt = cc_scan_counts(f.blk_t + (size_t)s * f.nblk_t, f.nblk_t, s_wsum);
    if (threadIdx.x == 0) {
        f.o_n_pts[s] = nv;
        f.o_n_tri[s] = nt;
    }
}

__global__ __launch_bounds__(kCcTile) void filter_vertex_kernel(FilterBufs f) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / f.nblk_v, blk = blockIdx.x - s * f.nblk_v;
    const unsigned e = blk * kCcTile + threadIdx.x;
    const bool stays = filter_vertex_stays(f, s, e);
    int total;
    const int at = f.blk_v[(size_t)s * f.nblk_v + blk] + rp_block_rank(stays, s_wsum, total);
    if (e >= (unsigned)f.cap) return;
    f.map[(size_t)s * f.cap + e] = stays ? at : -1;
    f.o_valid[(size_t)s * f.cap + e] = (uint8_t)((int)e < f.o_n_pts[s]);         // the scan's launch wrote it
    if (!stays) return;
    const size_t i = ((size_t)s * f.cap + e) * 3, o = ((size_t)s * f.cap + at) * 3;  // at <= e < cap
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        f.o_points[o + x] = f.points[i + x];
        f.o_normals[o + x] = f.normals[i + x];
        if (f.colors) f.o_colors[o + x] = f.colors[i + x];
    }
}

__global__ __launch_bounds__(kCcTile) void filter_triangle_kernel(FilterBufs f) {
    __shared__ int s_wsum[16];
    const unsigned s = blockIdx.x / f.nblk_t, blk = blockIdx.x - s * f.nblk_t;
    const unsigned t = blk * kCcTile + threadIdx.x;
    const bool stays = filter_triangle_stays(f, s, t);
    int total;
    const int at = f.blk_t[(size_t)s * f.nblk_t + blk] + rp_block_rank(stays, s_wsum, total);
    if (!stays) return;
    const int nv = cc_clamp(f.n_pts[s], f.cap);
    const int* r = f.tri + ((size_t)s * f.cap_tri + t) * 3;
    int* o = f.o_tri + ((size_t)s * f.cap_tri + at) * 3;                          // at <= t < cap_tri
#pragma unroll
    for (int x = 0; x < 3; ++x) o[x] = (unsigned)r[x] < (unsigned)nv ? f.map[(size_t)s * f.cap + r[x]] : -1;
}

size_t carve_filter(int S, int cap, int cap_tri, char* base, FilterBufs& f) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    f.blk_v = (int*)take((size_t)S * blocks_of(cap, kCcTile) * sizeof(int));
    f.blk_t = (int*)take((size_t)S * blocks_of(cap_tri, kCcTile) * sizeof(int));
    f.map = (int*)take((size_t)S * cap * sizeof(int));
    return off;
}

}  // namespace

extern "C" size_t relpose_mesh_components_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri) {
    if (!cc_sizes_ok(n_scenes, cap, cap_tri)) return 0;
    CcBufs b{};
    return carve_cc(n_scenes, cap, nullptr, b);
}

extern "C" int relpose_mesh_components(const RelposeMeshComponentsArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeMeshComponentsArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeMeshComponentsArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeMeshComponentsArgs)));
    if (!a.triangles || !a.n_triangles || !a.n_points || !a.vertex_label || !a.tri_label || !a.n_components || !a.bad_triangles || !a.workspace)
        return RELPOSE_EINVAL;
    if (!cc_sizes_ok(a.n_scenes, a.cap, a.cap_tri) || a.cap_comp < 0 || (long long)a.n_scenes * a.cap_comp >= (1ll << 29)) return RELPOSE_EINVAL;
    if (a.cap_comp > 0 && (!a.comp_root || !a.comp_vertices || !a.comp_triangles || !a.comp_area)) return RELPOSE_EINVAL;
    if (a.max_rounds < 1 || !(std::isfinite(a.area_scale) && a.area_scale > 0.0)) return RELPOSE_EINVAL;
    CcBufs b{};
    if (a.workspace_bytes < carve_cc(a.n_scenes, a.cap, nullptr, b) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_cc(a.n_scenes, a.cap, (char*)a.workspace, b);
    b.cap = a.cap; b.cap_tri = a.cap_tri; b.cap_comp = a.cap_comp;
    b.nblk_v = blocks_of(a.cap, kCcTile); b.nblk_t = blocks_of(a.cap_tri, kCcTile);
    b.nstat_v = blocks_of(a.cap, kCcTile * kCcStatTiles); b.nstat_t = blocks_of(a.cap_tri, kCcTile * kCcStatTiles);
    b.tri = a.triangles; b.n_tri = a.n_triangles; b.n_pts = a.n_points; b.points = a.points; b.area_scale = a.area_scale;
    b.vlabel = a.vertex_label; b.tlabel = a.tri_label; b.n_comp = a.n_components; b.bad = a.bad_triangles;
    b.c_root = a.comp_root; b.c_vert = a.comp_vertices; b.c_tri = a.comp_triangles; b.c_area = (unsigned long long*)a.comp_area;
    hipStream_t s = (hipStream_t)a.stream;
    const unsigned S = (unsigned)a.n_scenes, grid_v = S * b.nblk_v, grid_t = S * b.nblk_t;
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_v), dim3(kCcTile), 0, s, b);
    hipLaunchKernelGGL(cc_mark_kernel, dim3(grid_t), dim3(kCcTile), 0, s, b);
    RP_CHECK_LAUNCH();
    int rounds = 0;
    bool settled = false;
    while (!settled && rounds < a.max_rounds) {
        const int g = std::min(kCcGroup, a.max_rounds - rounds);
        int set[kCcGroup];
        RP_HIP(hipMemsetAsync(b.flags, 0, kCcGroup * sizeof(int), s));
        for (int r = 0; r < g; ++r) {
            hipLaunchKernelGGL(cc_hook_kernel, dim3(grid_t), dim3(kCcTile), 0, s, b, b.flags + r);
            hipLaunchKernelGGL(cc_jump_kernel, dim3(grid_v), dim3(kCcTile), 0, s, b, b.flags + r);
        }
        RP_CHECK_LAUNCH();
        RP_HIP(hipMemcpyAsync(set, b.flags, g * sizeof(int), hipMemcpyDeviceToHost, s));
        RP_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < g && !settled; ++r) {                                 // rounds behind the first quiet one changed nothing
            ++rounds;
            settled = set[r] == 0;
        }
    }
    if (a.rounds_host) *a.rounds_host = rounds;
    if (!settled) return RELPOSE_EROUNDS;
    hipLaunchKernelGGL(cc_root_count_kernel, dim3(grid_v), dim3(kCcTile), 0, s, b);
    hipLaunchKernelGGL(cc_root_scan_kernel, dim3(S), dim3(kCcScanThreads), 0, s, b);
    hipLaunchKernelGGL(cc_root_write_kernel, dim3(grid_v), dim3(kCcTile), 0, s, b);
    hipLaunchKernelGGL(cc_vertex_kernel, dim3(S * b.nstat_v), dim3(kCcTile), 0, s, b);
    hipLaunchKernelGGL(cc_triangle_kernel, dim3(S * b.nstat_t), dim3(kCcTile), 0, s, b);
    RP_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t relpose_mesh_filter_workspace_bytes(int32_t n_scenes, int32_t cap, int32_t cap_tri) {
    if (!cc_sizes_ok(n_scenes, cap, cap_tri)) return 0;
    FilterBufs f{};
    return carve_filter(n_scenes, cap, cap_tri, nullptr, f);
}

extern "C" int relpose_mesh_filter(const RelposeMeshFilterArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeMeshFilterArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeMeshFilterArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeMeshFilterArgs)));
    if (!a.points || !a.normals || !a.n_points || !a.triangles || !a.n_triangles || !a.vertex_label || !a.tri_label || !a.out_points ||
        !a.out_normals || !a.out_valid || !a.out_n_points || !a.out_triangles || !a.out_n_triangles || !a.workspace)
        return RELPOSE_EINVAL;
    if ((a.colors == nullptr) != (a.out_colors == nullptr)) return RELPOSE_EINVAL;
    if (!cc_sizes_ok(a.n_scenes, a.cap, a.cap_tri) || a.cap_comp < 0 || (long long)a.n_scenes * a.cap_comp >= (1ll << 29)) return RELPOSE_EINVAL;
    if ((a.cap_comp > 0 && !a.keep) || (a.drop_unused != 0 && a.drop_unused != 1)) return RELPOSE_EINVAL;
    if (a.out_points == a.points || a.out_normals == a.normals || (a.colors && a.out_colors == a.colors) || a.out_triangles == a.triangles ||
        a.out_n_points == a.n_points || a.out_n_triangles == a.n_triangles || a.vertex_map == a.vertex_label)
        return RELPOSE_EINVAL;                                                    // the outputs are buffers of their own
    FilterBufs f{};
    if (a.workspace_bytes < carve_filter(a.n_scenes, a.cap, a.cap_tri, nullptr, f) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve_filter(a.n_scenes, a.cap, a.cap_tri, (char*)a.workspace, f);
    f.cap = a.cap; f.cap_tri = a.cap_tri; f.cap_comp = a.cap_comp; f.drop_unused = a.drop_unused;
    f.nblk_v = blocks_of(a.cap, kCcTile); f.nblk_t = blocks_of(a.cap_tri, kCcTile);
    f.points = a.points; f.normals = a.normals; f.colors = a.colors; f.n_pts = a.n_points; f.tri = a.triangles; f.n_tri = a.n_triangles;
    f.vlabel = a.vertex_label; f.tlabel = a.tri_label; f.keep = a.keep;
    f.o_points = a.out_points; f.o_normals = a.out_normals; f.o_colors = a.out_colors; f.o_valid = a.out_valid; f.o_n_pts = a.out_n_points;
    f.o_tri = a.out_triangles; f.o_n_tri = a.out_n_triangles;
    if (a.vertex_map) f.map = a.vertex_map;
    hipStream_t s = (hipStream_t)a.stream;
    const unsigned S = (unsigned)a.n_scenes;
    hipLaunchKernelGGL(filter_count_kernel, dim3(S * (f.nblk_v + f.nblk_t)), dim3(kCcTile), 0, s, f);
    hipLaunchKernelGGL(filter_scan_kernel, dim3(S), dim3(kCcScanThreads), 0, s, f);
    hipLaunchKernelGGL(filter_vertex_kernel, dim3(S * f.nblk_v), dim3(kCcTile), 0, s, f);
    hipLaunchKernelGGL(filter_triangle_kernel, dim3(S * f.nblk_t), dim3(kCcTile), 0, s, f);
    RP_CHECK_LAUNCH();
    return 0;
}
