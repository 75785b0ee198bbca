// RANSAC over FPFH feature correspondences for a batch of point-cloud pairs: the reference's `--method gs` baseline,
// open3d_global_registration (baselines.py:52-81).  The contract -- draws, checks, orders, reductions -- is DESIGN.md §4.7;
// tests/ransac_model.py restates it in numpy.  Built with -ffp-contract=off: the model and these kernels round alike.
//
// Clouds: c = 2b (source of pair b), 2b + 1 (target).  The front end is relpose_fgr's (fgr_internal.h: six launches); the exclusive block
// scan and the xor-tree reductions are cloud_prims.h's.  Then
//   ransac_grid_kernel      one block per pair: the target's dense cell table (cell 0.16 >= 2 x 0.075, doubled until it fits)
//   ransac_screen_kernel    per round, one thread per iteration: draws, edge test, Horn + distance test for the survivors, pass bits
//   ransac_compact_kernel   per round, one block per pair: appends the passing iterations in order until the validated set is full
//   ransac_validate_kernel  one block per (validated hypothesis, pair): inlier count and fixed-order sum of inlier d2
//   ransac_select_kernel    one wave per pair: the best hypothesis in validation order, the pose and the per-pair outputs
// Rounds r = 0, 1, ... cover iterations [64 Ki (2^r - 1), 64 Ki (2^(r+1) - 1)) clipped to max_iterations (6 rounds for 4 M), so the
// number of launches depends on max_iterations only.  A pair whose validated set is full skips the rounds after it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cloud_prims.h"
#include "common.h"
#include "fgr_internal.h"
#include "rp_math.h"

namespace {

constexpr double kMaxDist = 0.075;
constexpr double kEdge = 0.9;
constexpr double kCell = 0.16;           // validation grid cell: > 2 x kMaxDist, so a query's ball meets 2 x 2 x 2 cells
constexpr int kRound0 = 65536;
constexpr int kNnFpfh = 100;
constexpr int kFeat = 33;

struct RansacBufs {
    int B, cap, max_iter, max_val, tcells;
    long long nwords;
    unsigned long long seed;
    const double* pts;       // [2B, cap, 3] (front end)
    const int* count;        // [2B]
    const int* nn;           // [2B, cap]
    double* glo;             // [B, 4] grid origin xyz, cell size
    int* gdim;               // [B, 4] nx, ny, nz
    int* cstart;             // [B, tcells + 1]
    int* cfill;              // [B, tcells]
    double* cpts;            // [B, cap, 3] target voxels in cell order
    unsigned long long* bits;   // [B, nwords] pass bits by iteration
    int* state;              // [B, 4] done, validated so far, n_iterations
    int* val_iter;           // [B, max_val]
    int* val_inl;
    double* val_err;
    double* pose;
    int* status;
    double* fitness;
    double* rmse;
    int* n_iterations;
    int* n_validations;
    int* best_index;
    int* nn_out;             // [B, cap]
};

__device__ __forceinline__ bool pair_live(const RansacBufs& r, int b) {
    const int ns = r.count[2 * b], nt = r.count[2 * b + 1];
    return ns <= r.cap && nt <= r.cap && ns >= 3 && nt >= 3;
}

// Iteration t of pair b: true if it passes both checkers, with R, tr of its estimate.
__device__ bool ransac_hypothesis(const RansacBufs& r, int b, long long t, double R[3][3], double tr[3]) {
    const int ns = r.count[2 * b];
    const double* ps = r.pts + (long long)(2 * b) * r.cap * 3;
    const double* pt = r.pts + (long long)(2 * b + 1) * r.cap * 3;
    const int* nn = r.nn + (long long)(2 * b) * r.cap;
    const unsigned long long base = r.seed * 0x9E3779B97F4A7C15ull;
    double s[4][3], q[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)(fgr_splitmix(base + (unsigned long long)t * 4ull + (unsigned long long)k) % (unsigned long long)ns);
        const int j = nn[i];
        if (j < 0) return false;                     // a source voxel without a feature match (non-finite features only)
#pragma unroll
        for (int a = 0; a < 3; ++a) { s[k][a] = ps[3 * i + a]; q[k][a] = pt[3 * j + a]; }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = j + 1; k < 4; ++k) {
            const double ds = rp_dist3(s[j], s[k]), dt = rp_dist3(q[j], q[k]);
            if (ds < kEdge * dt || dt < kEdge * ds) return false;
        }
    double cs[3], ct[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cs[a] = (((s[0][a] + s[1][a]) + s[2][a]) + s[3][a]) / 4.0;
        ct[a] = (((q[0][a] + q[1][a]) + q[2][a]) + q[3][a]) / 4.0;
    }
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double m = (s[0][a] - cs[a]) * (q[0][c] - ct[c]);
#pragma unroll
            for (int k = 1; k < 4; ++k) m += (s[k][a] - cs[a]) * (q[k][c] - ct[c]);
            M[a][c] = m;
        }
    rp_horn_rotation(M, R);
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = ct[a] - ((R[a][0] * cs[0] + R[a][1] * cs[1]) + R[a][2] * cs[2]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = ((R[a][0] * s[k][0] + R[a][1] * s[k][1]) + R[a][2] * s[k][2]) + tr[a];
        if (rp_dist3(p, q[k]) > kMaxDist) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------- grid + state
__global__ __launch_bounds__(1024) void ransac_grid_kernel(RansacBufs r) {
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    __shared__ double red[6][16];
    __shared__ int wsum[16];
    int* st = r.state + 4 * b;
    const bool live = pair_live(r, b);
    if (tid == 0) {
        st[0] = live ? 0 : 1;
        st[1] = 0;
        st[2] = live ? r.max_iter : 0;
        st[3] = 0;
    }
    if (!live) {
        if (tid < 4) r.gdim[4 * b + tid] = 0;
        return;
    }
    const int n = r.count[2 * b + 1];
    const double* pts = r.pts + (long long)(2 * b + 1) * r.cap * 3;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += nt)
        for (int a = 0; a < 3; ++a) { mn[a] = fmin(mn[a], pts[3 * i + a]); mx[a] = fmax(mx[a], pts[3 * i + a]); }
    for (int a = 0; a < 3; ++a) { mn[a] = rp_wave_min(mn[a]); mx[a] = rp_wave_max(mx[a]); }
    if (rp_lane() == 0)
        for (int a = 0; a < 3; ++a) { red[a][tid >> 6] = mn[a]; red[3 + a][tid >> 6] = mx[a]; }
    __syncthreads();
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = red[a][0]; hi[a] = red[3 + a][0];
        for (int w = 1; w < nt / 64; ++w) { lo[a] = fmin(lo[a], red[a][w]); hi[a] = fmax(hi[a], red[3 + a][w]); }
    }
    double h = kCell;
    double dim[3];
    for (int it = 0; it < 2100; ++it) {             // h doubles until the dense table fits (terminates long before 2100 for finite points)
        for (int a = 0; a < 3; ++a) dim[a] = floor((hi[a] - lo[a]) / h) + 1.0;
        if (dim[0] * dim[1] * dim[2] <= (double)r.tcells) break;
        h *= 2.0;
    }
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const int ncell = nx * ny * nz;
    if (tid == 0) {
        for (int a = 0; a < 3; ++a) r.glo[4 * b + a] = lo[a];
        r.glo[4 * b + 3] = h;
        r.gdim[4 * b] = nx; r.gdim[4 * b + 1] = ny; r.gdim[4 * b + 2] = nz; r.gdim[4 * b + 3] = ncell;
    }
    int* cstart = r.cstart + (long long)b * (r.tcells + 1);
    int* cfill = r.cfill + (long long)b * r.tcells;
    for (int e = tid; e < ncell; e += nt) cfill[e] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int cx = (int)floor((pts[3 * i] - lo[0]) / h), cy = (int)floor((pts[3 * i + 1] - lo[1]) / h), cz = (int)floor((pts[3 * i + 2] - lo[2]) / h);
        atomicAdd(&cfill[(cx * ny + cy) * nz + cz], 1);
    }
    __syncthreads();
    int run = 0;
    for (int e0 = 0; e0 < ncell; e0 += nt) {
        const int e = e0 + tid;
        const int c = e < ncell ? cfill[e] : 0;
        int tot;
        const int before = rp_block_excl_scan(c, wsum, tot);
        if (e < ncell) { cstart[e] = run + before; cfill[e] = run + before; }
        run += tot;
    }
    if (tid == 0) cstart[ncell] = run;
    __syncthreads();
    double* cp = r.cpts + (long long)b * r.cap * 3;
    for (int i = tid; i < n; i += nt) {
        const int cx = (int)floor((pts[3 * i] - lo[0]) / h), cy = (int)floor((pts[3 * i + 1] - lo[1]) / h), cz = (int)floor((pts[3 * i + 2] - lo[2]) / h);
        const int o = atomicAdd(&cfill[(cx * ny + cy) * nz + cz], 1);
        for (int a = 0; a < 3; ++a) cp[3 * o + a] = pts[3 * i + a];
    }
}

// ------------------------------------------------------------------------------------------------------- screen + compaction
__global__ __launch_bounds__(256) void ransac_screen_kernel(RansacBufs r, long long t0, long long t1) {
    const int b = blockIdx.y;
    if (r.state[4 * b] != 0) return;                  // validated set full, or nothing to register
    const long long t = t0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (t < t1) {
        double R[3][3], tr[3];
        ok = ransac_hypothesis(r, b, t, R, tr);
    }
    const unsigned long long m = __ballot(ok);
    if (rp_lane() == 0 && t < t1) r.bits[(long long)b * r.nwords + (t >> 6)] = m;
}

__global__ __launch_bounds__(1024) void ransac_compact_kernel(RansacBufs r, long long t0, long long t1) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int wsum[16];
    int* st = r.state + 4 * b;
    if (st[0] != 0) return;
    int nval = st[1];
    const long long w0 = t0 >> 6, w1 = (t1 + 63) >> 6;
    const unsigned long long* bits = r.bits + (long long)b * r.nwords;
    int* vi = r.val_iter + (long long)b * r.max_val;
    for (long long c0 = w0; c0 < w1 && nval < r.max_val; c0 += blockDim.x) {
        const long long w = c0 + tid;
        unsigned long long m = w < w1 ? bits[w] : 0ull;
        int tot;
        int slot = nval + rp_block_excl_scan(__popcll(m), wsum, tot);
        while (m != 0ull && slot < r.max_val) {
            const long long it = (w << 6) + __builtin_ctzll(m);
            vi[slot] = (int)it;
            if (slot == r.max_val - 1) st[2] = (int)(it + 1);
            ++slot;
            m &= m - 1;
        }
        nval += tot;
    }
    if (tid == 0) {
        st[1] = min(nval, r.max_val);
        if (nval >= r.max_val) st[0] = 1;
    }
}

// ------------------------------------------------------------------------------------------------------- validation
__global__ __launch_bounds__(256) void ransac_validate_kernel(RansacBufs r) {
    const int v = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    __shared__ double red[4];
    __shared__ int redi[4];
    if (v >= r.state[4 * b + 1]) return;
    double R[3][3], tr[3];
    ransac_hypothesis(r, b, r.val_iter[(long long)b * r.max_val + v], R, tr);
    const int ns = r.count[2 * b];
    const double* ps = r.pts + (long long)(2 * b) * r.cap * 3;
    const double* cp = r.cpts + (long long)b * r.cap * 3;
    const int* cstart = r.cstart + (long long)b * (r.tcells + 1);
    const double lo[3] = {r.glo[4 * b], r.glo[4 * b + 1], r.glo[4 * b + 2]}, h = r.glo[4 * b + 3];
    const int dim[3] = {r.gdim[4 * b], r.gdim[4 * b + 1], r.gdim[4 * b + 2]};
    const double r2 = kMaxDist * kMaxDist;
    int cnt = 0;
    double sum = 0.0;
    for (int i = tid; i < ns; i += blockDim.x) {
        double q[3];
        for (int a = 0; a < 3; ++a) q[a] = ((R[a][0] * ps[3 * i] + R[a][1] * ps[3 * i + 1]) + R[a][2] * ps[3 * i + 2]) + tr[a];
        int c0[3];
        bool in = true;
        for (int a = 0; a < 3; ++a) {
            const double f = (q[a] - lo[a]) / h;
            in = in && f >= -1.0 && f < (double)dim[a] + 1.0;
            const double fl = in ? floor(f) : 0.0;
            c0[a] = (int)fl - ((f - fl) < 0.5 ? 1 : 0);     // the two cells the 0.075 ball can reach along this axis: c0, c0 + 1
        }
        if (!in) continue;
        double best = r2;
        bool hit = false;
        for (int cx = max(c0[0], 0); cx <= min(c0[0] + 1, dim[0] - 1); ++cx)
            for (int cy = max(c0[1], 0); cy <= min(c0[1] + 1, dim[1] - 1); ++cy)
                for (int cz = max(c0[2], 0); cz <= min(c0[2] + 1, dim[2] - 1); ++cz) {
                    const int cell = (cx * dim[1] + cy) * dim[2] + cz;
                    const int e1 = cstart[cell + 1];
                    for (int e = cstart[cell]; e < e1; ++e) {
                        const double dx = cp[3 * e] - q[0], dy = cp[3 * e + 1] - q[1], dz = cp[3 * e + 2] - q[2];
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (d2 < best) { best = d2; hit = true; }
                    }
                }
        if (hit) { ++cnt; sum += best; }
    }
    // the fixed reduction of DESIGN.md §4.7 step 7: per-thread sums in point order, xor tree over the wave, the 4 wave sums in order
    sum = rp_wave_xor_sum(sum);
    cnt = rp_wave_sum_i(cnt);
    if (rp_lane() == 0) { red[tid >> 6] = sum; redi[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        const double tot = ((red[0] + red[1]) + red[2]) + red[3];
        const int inl = ((redi[0] + redi[1]) + redi[2]) + redi[3];
        r.val_inl[(long long)b * r.max_val + v] = inl;
        r.val_err[(long long)b * r.max_val + v] = inl > 0 ? sqrt(tot / (double)inl) : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------- selection
__global__ __launch_bounds__(64) void ransac_select_kernel(RansacBufs r) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* st = r.state + 4 * b;
    const int ns = r.count[2 * b], nt = r.count[2 * b + 1];
    if (r.nn_out && ns <= r.cap && nt <= r.cap) {
        for (int e = lane; e < ns; e += 64) r.nn_out[(long long)b * r.cap + e] = r.nn[(long long)(2 * b) * r.cap + e];
    }
    if (lane != 0) return;
    int status = 0;
    if (ns > r.cap || nt > r.cap) status = 3;
    else if (ns < 3 || nt < 3) status = 1;
    const int nval = st[1];
    int best = -1, bi = 0;
    double br = 0.0;
    if (status == 0) {
        for (int v = 0; v < nval; ++v) {
            const int inl = r.val_inl[(long long)b * r.max_val + v];
            const double e = r.val_err[(long long)b * r.max_val + v];
            if (inl > bi || (inl == bi && e < br)) { best = v; bi = inl; br = e; }
        }
        if (best < 0) status = 4;
    }
    double* T = r.pose + (long long)b * 16;
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (status == 0) {
        double R[3][3], tr[3];
        ransac_hypothesis(r, b, r.val_iter[(long long)b * r.max_val + best], R, tr);
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) T[4 * a + c] = R[a][c];
            T[4 * a + 3] = tr[a];
        }
    }
    r.status[b] = status;
    if (r.fitness) r.fitness[b] = status == 0 ? (double)bi / (double)ns : 0.0;
    if (r.rmse) r.rmse[b] = status == 0 ? br : 0.0;
    if (r.n_iterations) r.n_iterations[b] = st[2];
    if (r.n_validations) r.n_validations[b] = nval;
    if (r.best_index) r.best_index[b] = status == 0 ? best : -1;
}

// ------------------------------------------------------------------------------------------------------------------ host
int rounds_for(int max_iter) {
    int n = 0;
    while ((long long)kRound0 * ((1LL << n) - 1) < max_iter) ++n;
    return n;
}

struct RansacPlan {
    int max_iter, max_val, tcells;
    long long nwords;
    size_t off_key0, off_key1, off_idx0, off_idx1, off_pts, off_ix, off_count, off_nbr, off_nd2, off_ncnt, off_normal, off_spfh, off_fpfh,
        off_f32, off_nn, off_glo, off_gdim, off_cstart, off_cfill, off_cpts, off_bits, off_state, off_viter, off_vinl, off_verr, total;
};

bool ransac_plan(int B, int P, int cap, int max_iter, int max_val, RansacPlan& p) {
    if (B <= 0 || B > 32767 || P <= 0 || cap <= 0 || cap > RELPOSE_FGR_MAX_POINTS_LIMIT || (long long)P > (1LL << 30)) return false;
    if (max_iter < 0 || max_iter > RELPOSE_RANSAC_MAX_ITERATIONS_LIMIT || max_val < 0 || max_val > RELPOSE_RANSAC_MAX_VALIDATIONS_LIMIT) return false;
    p.max_iter = max_iter ? max_iter : RELPOSE_RANSAC_MAX_ITERATIONS;
    p.max_val = max_val ? max_val : RELPOSE_RANSAC_MAX_VALIDATIONS;
    p.tcells = 4 * cap + 4096;
    p.nwords = ((long long)p.max_iter + 63) / 64;
    const size_t C = 2 * (size_t)B, N = (size_t)cap, Bs = (size_t)B;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += rp_align(bytes); return o; };
    p.off_key0 = take(C * P * 8);
    p.off_key1 = take(C * P * 8);
    p.off_idx0 = take(C * P * 4);
    p.off_idx1 = take(C * P * 4);
    p.off_pts = take(C * N * 3 * 8);
    p.off_ix = take(C * N * 4);
    p.off_count = take(C * 4);
    p.off_nbr = take(C * N * kNnFpfh * 4);
    p.off_nd2 = take(C * N * kNnFpfh * 8);
    p.off_ncnt = take(C * N * 4);
    p.off_normal = take(C * N * 3 * 8);
    p.off_spfh = take(C * N * kFeat * 8);
    p.off_fpfh = take(C * N * kFeat * 8);
    p.off_f32 = take(C * N * kFeat * 4);
    p.off_nn = take(C * N * 4);
    p.off_glo = take(Bs * 4 * 8);
    p.off_gdim = take(Bs * 4 * 4);
    p.off_cstart = take(Bs * ((size_t)p.tcells + 1) * 4);
    p.off_cfill = take(Bs * (size_t)p.tcells * 4);
    p.off_cpts = take(Bs * N * 3 * 8);
    p.off_bits = take(Bs * (size_t)p.nwords * 8);
    p.off_state = take(Bs * 4 * 4);
    p.off_viter = take(Bs * (size_t)p.max_val * 4);
    p.off_vinl = take(Bs * (size_t)p.max_val * 4);
    p.off_verr = take(Bs * (size_t)p.max_val * 8);
    p.total = off;
    return true;
}

}  // namespace

extern "C" {

size_t relpose_ransac_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points, int32_t max_iterations, int32_t max_validations) {
    RansacPlan p;
    return ransac_plan(n_pairs, n_points, max_points, max_iterations, max_validations, p) ? p.total : 0;
}

int relpose_ransac(const RelposeRansacArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeRansacArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeRansacArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeRansacArgs)));
    RansacPlan p;
    if (!a.pc || !a.valid || !a.pose || !a.status || !a.workspace ||
        !ransac_plan(a.n_pairs, a.n_points, a.max_points, a.max_iterations, a.max_validations, p))
        return RELPOSE_EINVAL;
    if (a.workspace_bytes < p.total) return RELPOSE_ENOMEM;
    hipStream_t s = (hipStream_t)a.stream;
    char* ws = (char*)a.workspace;
    const int B = a.n_pairs, N = a.max_points;
    FgrBufs f{};
    f.n_clouds = 2 * B;
    f.P = a.n_points;
    f.cap = N;
    f.pc = a.pc;
    f.valid = a.valid;
    f.key[0] = (long long*)(ws + p.off_key0);
    f.key[1] = (long long*)(ws + p.off_key1);
    f.idx[0] = (int*)(ws + p.off_idx0);
    f.idx[1] = (int*)(ws + p.off_idx1);
    f.pts = a.down_points ? a.down_points : (double*)(ws + p.off_pts);
    f.ix = (int*)(ws + p.off_ix);
    f.count = a.down_count ? a.down_count : (int*)(ws + p.off_count);
    f.nbr = (int*)(ws + p.off_nbr);
    f.nd2 = (double*)(ws + p.off_nd2);
    f.ncnt = (int*)(ws + p.off_ncnt);
    f.normal = (double*)(ws + p.off_normal);
    f.spfh = (double*)(ws + p.off_spfh);
    f.fpfh = a.fpfh ? a.fpfh : (double*)(ws + p.off_fpfh);
    f.f32 = (float*)(ws + p.off_f32);
    f.nn = (int*)(ws + p.off_nn);
    f.seed = a.seed;
    RansacBufs r{};
    r.B = B;
    r.cap = N;
    r.max_iter = p.max_iter;
    r.max_val = p.max_val;
    r.tcells = p.tcells;
    r.nwords = p.nwords;
    r.seed = a.seed;
    r.pts = f.pts;
    r.count = f.count;
    r.nn = f.nn;
    r.glo = (double*)(ws + p.off_glo);
    r.gdim = (int*)(ws + p.off_gdim);
    r.cstart = (int*)(ws + p.off_cstart);
    r.cfill = (int*)(ws + p.off_cfill);
    r.cpts = (double*)(ws + p.off_cpts);
    r.bits = (unsigned long long*)(ws + p.off_bits);
    r.state = (int*)(ws + p.off_state);
    r.val_iter = a.val_iter ? a.val_iter : (int*)(ws + p.off_viter);
    r.val_inl = a.val_inliers ? a.val_inliers : (int*)(ws + p.off_vinl);
    r.val_err = a.val_err ? a.val_err : (double*)(ws + p.off_verr);
    r.pose = a.pose;
    r.status = a.status;
    r.fitness = a.fitness;
    r.rmse = a.inlier_rmse;
    r.n_iterations = a.n_iterations;
    r.n_validations = a.n_validations;
    r.best_index = a.best_index;
    r.nn_out = a.nn;
    fgr_front_end(f, s);
    hipLaunchKernelGGL(ransac_grid_kernel, dim3(B), dim3(1024), 0, s, r);
    const int nr = rounds_for(p.max_iter);
    for (int k = 0; k < nr; ++k) {
        const long long t0 = (long long)kRound0 * ((1LL << k) - 1);
        const long long t1 = std::min((long long)kRound0 * ((1LL << (k + 1)) - 1), (long long)p.max_iter);
        hipLaunchKernelGGL(ransac_screen_kernel, dim3((unsigned)((t1 - t0 + 255) / 256), B), dim3(256), 0, s, r, t0, t1);
        hipLaunchKernelGGL(ransac_compact_kernel, dim3(B), dim3(1024), 0, s, r, t0, t1);
    }
    hipLaunchKernelGGL(ransac_validate_kernel, dim3(p.max_val, B), dim3(256), 0, s, r);
    hipLaunchKernelGGL(ransac_select_kernel, dim3(B), dim3(64), 0, s, r);
    RP_CHECK_LAUNCH();
    // the one synchronisation: the per-pair statuses tell whether a cloud had more voxels than max_points
    int h_over = 0;
    std::vector<int> hs(B);
    RP_HIP(hipMemcpyAsync(hs.data(), a.status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    RP_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) h_over |= hs[b] == RELPOSE_RANSAC_STATUS_OVERFLOW;
    return h_over ? RELPOSE_RANSAC_OVERFLOW : 0;
}

}  // extern "C"
