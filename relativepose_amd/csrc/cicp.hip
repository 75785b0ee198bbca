// Coloured point-cloud ICP (Park, Zhou, Koltun, ICCV 2017) for a batch of point-cloud pairs: the three refinement levels of the
// reference's `--method cgs` baseline, open3d_color_registration (baselines.py:110-168).  The contract -- every constant, stage and
// order -- is DESIGN.md §4.8; tests/cicp_model.py restates it in numpy.  Built with -ffp-contract=off: the model and these kernels
// round alike.
//
// Clouds: c = 2b (source of pair b), 2b + 1 (target); level l = 0, 1, 2 has voxel size = radius 0.04, 0.02, 0.01.  Per-level arrays are
// indexed by cl = 3 c + l (both clouds) or tl = 3 b + l (target only).  Kernels:
//   cicp_voxel_kernel     one block per (cloud, level): the voxel downsample fgr.hip runs (cloud_prims.h's rp_voxel_downsample) at the
//                         level's voxel size, colours averaged like the points; also keeps every voxel's key and the lattice (min bound,
//                         extents) for the searches below
//   cicp_neighbors_kernel one wave per target voxel: the (d2, index)-ordered hybrid list (r = 2 radius, max 30) from the sorted keys
//   cicp_normals_kernel   one thread per target voxel: normal (§4.6 stage 3: cloud_prims.h's rp_normal_from_neighbors) and the colour gradient
//   cicp_init_kernel      one wave per pair: status, the starting transform, the per-pair state
//   cicp_nn_kernel        per iteration, one thread per source voxel: q = T p and its nearest target voxel below the radius
//   cicp_step_kernel      per iteration, one block per pair: fitness / rmse, the stop test, the 27 sums in the fixed order of §4.7
//                         stage 7, the 6x6 Cholesky solve and the update of T; raises the pair's level-done flag
// The nearest-neighbour search uses that a level's target voxels are stored in ascending key order, key = (kx ny + ky) nz + kz: the
// cells a ball can reach form, for every (kx, ky), one contiguous key range, found by binary search.  Each cell holds one voxel, so the
// search costs O(log n) per query.  The result is the minimum of d2 over every voxel the ball can reach (the ball is inflated by 1e-4
// so that rounding cannot hide one), ties to the lower index: it does not depend on the lattice.
// Launches: 4 + 2 x (50 + 30 + 14), whatever the batch size and the data; a pair whose level has ended skips that level's launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cloud_prims.h"
#include "common.h"

namespace {

constexpr int kLevels = RELPOSE_CICP_LEVELS;
constexpr int kNn = 30;                  // max_nn of the hybrid search
constexpr int kBuf = 256;                // candidates of one query: at most 6 x 6 x 6 cells of one voxel each
constexpr int kSlots = RELPOSE_CICP_TRACE_SLOTS;
constexpr double kRelFitness = 1e-6, kRelRmse = 1e-6;
constexpr double kInflate = 1.0001;      // the searched ball's radius over the true one
constexpr int kMaxIter[kLevels] = {50, 30, 14};
__constant__ double kRadius[kLevels] = {0.04, 0.02, 0.01};

struct CicpBufs {
    int B, P, cap;
    double lambda;
    const double* pc;        // [2B, P, 3]
    const double* color;     // [2B, P, 3]
    const uint8_t* valid;    // [2B, P]
    const double* init;      // [B, 4, 4] or NULL
    long long* key[2];       // [2B * 3, P] ping-pong
    int* idx[2];
    double* pts;             // [2B * 3, cap, 3]
    double* col;             // [2B * 3, cap, 3]
    long long* vkey;         // [2B * 3, cap] key of every voxel, ascending
    double* gmb;             // [2B * 3, 4] min bound
    long long* gdim;         // [2B * 3, 4] cells along x, y, z
    int* count;              // [2B * 3] true voxel count
    int* nbr;                // [B * 3, cap, 30] target only
    int* ncnt;               // [B * 3, cap]
    double* normal;          // [B * 3, cap, 3]
    double* grad;            // [B * 3, cap, 3]
    int* corr;               // [B, cap] this iteration's correspondences
    double* cd2;             // [B, cap]
    double* T;               // [B, 16] the accumulated transform
    double* prev;            // [B, 2] fitness and rmse of the previous evaluation
    int* state;              // [B, 4] dead, level 0 / 1 / 2 done
    double* pose;            // [B, 16]
    int* status;             // [B]
    double* fitness;         // [B, 3]
    double* rmse;            // [B, 3]
    int* n_iterations;       // [B, 3]
    double* level_pose;      // [B, 3, 16]
    double* iter_pose;       // [B, 94, 16]
    int* iter_ncorr;         // [B, 94]
    double* iter_rmse;       // [B, 94]
    int* iter_corr;          // [B, 94, cap]
    double* iter_x;          // [B, 94, 6]
};

// A x = b by Cholesky in the order of tests/fgr_model.py's cholesky_solve (every inner sum accumulated from 0, then subtracted);
// false at a non-positive pivot.  fgr.hip's fgr_optimize_kernel subtracts every product from the running value instead: the two round
// differently and each is pinned by its own numpy model, so they stay apart.
template <int N>
__device__ bool chol_solve(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
    double L[N][N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < j; ++k) acc += L[j][k] * L[j][k];
        const double s = A[j][j] - acc;
        if (!(s > 0)) return false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double a2 = 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) a2 += L[i][k] * L[j][k];
            L[i][j] = (A[i][j] - a2) / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) acc += L[i][k] * y[k];
        y[i] = (b[i] - acc) / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double acc = 0.0;
#pragma unroll
        for (int k = i + 1; k < N; ++k) acc += L[k][i] * x[k];
        x[i] = (y[i] - acc) / L[i][i];
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------- 1. coloured voxel grid
// averages the colours like the points; keeps every voxel's key and the lattice for the searches below
struct CicpVoxelPolicy {
    static constexpr bool kExtra = true;
    const double* extra_in;
    double* extra_out;
    long long* vkey;
    double* gmb;
    long long* gdim;
    __device__ void lattice(const double* mb, long long nx, long long ny, long long nz) const {
        for (int a = 0; a < 3; ++a) gmb[a] = mb[a];
        gdim[0] = nx; gdim[1] = ny; gdim[2] = nz;
    }
    __device__ void voxel(int o, long long key, long long, long long) const { vkey[o] = key; }
};

__global__ __launch_bounds__(1024) void cicp_voxel_kernel(CicpBufs f) {
    const int cl = blockIdx.x, c = cl / kLevels, l = cl % kLevels;
    const long long P = f.P;
    __shared__ RpVoxelScratch lds;
    const CicpVoxelPolicy pol{f.color + (long long)c * P * 3, f.col + (long long)cl * f.cap * 3, f.vkey + (long long)cl * f.cap, f.gmb + 4 * cl,
                              f.gdim + 4 * cl};
    const int nvox = rp_voxel_downsample(f.pc + (long long)c * P * 3, f.valid + (long long)c * P, P, kRadius[l], f.key[0] + (long long)cl * P,
                                         f.idx[0] + (long long)cl * P, f.key[1] + (long long)cl * P, f.idx[1] + (long long)cl * P,
                                         f.pts + (long long)cl * f.cap * 3, f.cap, lds, pol);
    if (threadIdx.x == 0) f.count[cl] = nvox;
}

// ------------------------------------------------------------------------------------------------------- lattice lookups
struct Lattice {
    const double* pts;       // [n, 3]
    const long long* key;    // [n] ascending
    int n;
    double mb[3], vox;
    long long dim[3];
};

__device__ __forceinline__ Lattice lattice_of(const CicpBufs& f, int cl, int l) {
    Lattice g;
    g.pts = f.pts + (long long)cl * f.cap * 3;
    g.key = f.vkey + (long long)cl * f.cap;
    g.n = min(f.count[cl], f.cap);
    g.vox = kRadius[l];
    for (int a = 0; a < 3; ++a) { g.mb[a] = f.gmb[4 * cl + a]; g.dim[a] = f.gdim[4 * cl + a]; }
    return g;
}

// The cells along one axis that the ball of radius rr around q meets, clipped to the lattice; false if none (or q is not finite).
__device__ __forceinline__ bool axis_range(double q, double mb, double vox, double rr, long long dim, long long& lo, long long& hi) {
    double fl = floor((q - rr - mb) / vox), fh = floor((q + rr - mb) / vox);
    if (!(fl <= fh)) return false;
    fl = fmax(fl, 0.0);
    fh = fmin(fh, (double)(dim - 1));
    if (!(fl <= fh)) return false;
    lo = (long long)fl;
    hi = (long long)fh;
    return true;
}

// ------------------------------------------------------------------------------------------------------- 2. neighbours (target)
__global__ __launch_bounds__(64) void cicp_neighbors_kernel(CicpBufs f) {
    const int tl = blockIdx.y, b = tl / kLevels, l = tl % kLevels, lane = threadIdx.x;
    const int cl = (2 * b + 1) * kLevels + l;
    __shared__ double bd[kBuf];
    __shared__ int bi[kBuf];
    const Lattice g = lattice_of(f, cl, l);
    const double rad = 2.0 * g.vox, r2 = rad * rad, rr = rad * kInflate;
    for (int q = blockIdx.x; q < g.n; q += gridDim.x) {
        const double qp[3] = {g.pts[3 * q], g.pts[3 * q + 1], g.pts[3 * q + 2]};
        long long lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
        bool any = true;
        for (int a = 0; a < 3; ++a) any = axis_range(qp[a], g.mb[a], g.vox, rr, g.dim[a], lo[a], hi[a]) && any;
        const int ncy = (int)(hi[1] - lo[1] + 1);
        const int ncol = any ? (int)(hi[0] - lo[0] + 1) * ncy : 0;
        int m = 0;
        for (int c0 = 0; c0 < ncol; c0 += 64) {
            const int col = c0 + lane;
            int s = 0, e = 0;
            if (col < ncol) {
                const long long kb = ((lo[0] + col / ncy) * g.dim[1] + (lo[1] + col % ncy)) * g.dim[2];
                s = rp_lower_bound(g.key, g.n, kb + lo[2]);
                e = s;
                while (e < g.n && g.key[e] <= kb + hi[2]) ++e;
            }
            for (int j = 0; __any(s + j < e); ++j) {
                const int cnd = s + j;
                double d2 = 0.0;
                bool in = false;
                if (cnd < e) {
                    const double dx = g.pts[3 * cnd] - qp[0], dy = g.pts[3 * cnd + 1] - qp[1], dz = g.pts[3 * cnd + 2] - qp[2];
                    d2 = (dx * dx + dy * dy) + dz * dz;
                    in = d2 < r2;
                }
                const unsigned long long msk = __ballot(in);
                const int o = m + __popcll(msk & rp_lanes_below());
                if (in && o < kBuf) { bd[o] = d2; bi[o] = cnd; }
                m = min(m + __popcll(msk), kBuf);
            }
        }
        __syncthreads();
        const long long row = (long long)tl * f.cap + q;
        for (int e = lane; e < m; e += 64) {
            const double de = bd[e];
            const int ie = bi[e];
            int rank = 0;
            for (int k = 0; k < m; ++k) rank += rp_lex_less(bd[k], bi[k], de, ie) ? 1 : 0;
            if (rank < kNn) f.nbr[row * kNn + rank] = ie;
        }
        if (lane == 0) f.ncnt[row] = min(m, kNn);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------- 3. normals + gradients
__device__ __forceinline__ double intensity(const double* c) { return ((c[0] + c[1]) + c[2]) / 3.0; }

__global__ __launch_bounds__(256) void cicp_normals_kernel(CicpBufs f) {
    const int tl = blockIdx.y, b = tl / kLevels, l = tl % kLevels;
    const int cl = (2 * b + 1) * kLevels + l;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(f.count[cl], f.cap);
    if (q >= n) return;
    const double* pts = f.pts + (long long)cl * f.cap * 3;
    const double* col = f.col + (long long)cl * f.cap * 3;
    const long long row = (long long)tl * f.cap + q;
    const int* nb = f.nbr + row * kNn;
    const int m = f.ncnt[row];
    const double p[3] = {pts[3 * q], pts[3 * q + 1], pts[3 * q + 2]};
    double nv[3];
    rp_normal_from_neighbors(pts, nb, m, p, nv);
    for (int a = 0; a < 3; ++a) f.normal[row * 3 + a] = nv[a];
    // colour gradient: least squares over the neighbours projected onto the tangent plane, plus the row that pins the normal component
    double gr[3] = {0.0, 0.0, 0.0};
    if (m >= 4) {
        double ata[6] = {0, 0, 0, 0, 0, 0}, atb[3] = {0, 0, 0};
        const double i0 = intensity(col + 3 * q);
        for (int k = 1; k < m; ++k) {
            const int j = nb[k];
            const double pk[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
            const double d[3] = {pk[0] - p[0], pk[1] - p[1], pk[2] - p[2]};
            const double s = rp_dot3(d, nv);
            const double a[3] = {(pk[0] - s * nv[0]) - p[0], (pk[1] - s * nv[1]) - p[1], (pk[2] - s * nv[2]) - p[2]};
            const double bk = intensity(col + 3 * j) - i0;
            ata[0] += a[0] * a[0]; ata[1] += a[0] * a[1]; ata[2] += a[0] * a[2]; ata[3] += a[1] * a[1]; ata[4] += a[1] * a[2]; ata[5] += a[2] * a[2];
            atb[0] += a[0] * bk; atb[1] += a[1] * bk; atb[2] += a[2] * bk;
        }
        const double wn = (double)(m - 1);
        const double a[3] = {wn * nv[0], wn * nv[1], wn * nv[2]};
        ata[0] += a[0] * a[0]; ata[1] += a[0] * a[1]; ata[2] += a[0] * a[2]; ata[3] += a[1] * a[1]; ata[4] += a[1] * a[2]; ata[5] += a[2] * a[2];
        const double M[3][3] = {{ata[0], ata[1], ata[2]}, {ata[1], ata[3], ata[4]}, {ata[2], ata[4], ata[5]}};
        const double rhs[3] = {atb[0], atb[1], atb[2]};
        double x[3] = {0.0, 0.0, 0.0};
        if (chol_solve<3>(M, rhs, x)) { gr[0] = x[0]; gr[1] = x[1]; gr[2] = x[2]; }
    }
    for (int a = 0; a < 3; ++a) f.grad[row * 3 + a] = gr[a];
}

// ------------------------------------------------------------------------------------------------------- state
__global__ __launch_bounds__(64) void cicp_init_kernel(CicpBufs f) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane != 0) return;
    int status = 0;
    for (int k = 0; k < 2 * kLevels; ++k)
        if (f.count[2 * b * kLevels + k] > f.cap) status = 3;
    if (status == 0)
        for (int k = 0; k < 2 * kLevels; ++k)
            if (f.count[2 * b * kLevels + k] < 3) status = 1;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = (status == 0 && f.init) ? f.init[16 * b + k] : ((k % 5 == 0) ? 1.0 : 0.0);
    for (int k = 0; k < 16; ++k) {
        f.T[16 * b + k] = T[k];
        f.pose[16 * b + k] = T[k];
        if (f.level_pose)
            for (int l = 0; l < kLevels; ++l) f.level_pose[(b * kLevels + l) * 16 + k] = T[k];
    }
    f.status[b] = status;
    f.state[4 * b] = status != 0;
    f.prev[2 * b] = f.prev[2 * b + 1] = 0.0;
    for (int l = 0; l < kLevels; ++l) {
        f.state[4 * b + 1 + l] = 0;
        if (f.fitness) f.fitness[b * kLevels + l] = 0.0;
        if (f.rmse) f.rmse[b * kLevels + l] = 0.0;
        if (f.n_iterations) f.n_iterations[b * kLevels + l] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------- iteration: evaluate
__device__ __forceinline__ void transform(const double* T, const double* p, double* q) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3];
}

__global__ __launch_bounds__(256) void cicp_nn_kernel(CicpBufs f, int l, int slot) {
    const int b = blockIdx.y;
    if (f.state[4 * b] != 0 || f.state[4 * b + 1 + l] != 0) return;
    const int cs = 2 * b * kLevels + l, ct = (2 * b + 1) * kLevels + l;
    const int ns = f.count[cs];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const Lattice g = lattice_of(f, ct, l);
    double q[3];
    transform(f.T + 16 * b, f.pts + ((long long)cs * f.cap + i) * 3, q);
    const double r2 = g.vox * g.vox, rr = g.vox * kInflate;
    long long lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
    bool any = true;
    for (int a = 0; a < 3; ++a) any = axis_range(q[a], g.mb[a], g.vox, rr, g.dim[a], lo[a], hi[a]) && any;
    double best = r2;
    int bi = -1;
    if (any) {
        // ascending (cx, cy, cz) is ascending key and so ascending voxel index: the strict < keeps the lower index of a tie
        for (long long cx = lo[0]; cx <= hi[0]; ++cx)
            for (long long cy = lo[1]; cy <= hi[1]; ++cy) {
                const long long kb = (cx * g.dim[1] + cy) * g.dim[2];
                const long long k1 = kb + hi[2];
                for (int e = rp_lower_bound(g.key, g.n, kb + lo[2]); e < g.n && g.key[e] <= k1; ++e) {
                    const double dx = g.pts[3 * e] - q[0], dy = g.pts[3 * e + 1] - q[1], dz = g.pts[3 * e + 2] - q[2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < best) { best = d2; bi = e; }
                }
            }
    }
    f.corr[(long long)b * f.cap + i] = bi;
    f.cd2[(long long)b * f.cap + i] = bi >= 0 ? best : 0.0;
    if (f.iter_corr) f.iter_corr[((long long)b * kSlots + slot) * f.cap + i] = bi;
}

// ------------------------------------------------------------------------------------------------------- iteration: step
__global__ __launch_bounds__(256) void cicp_step_kernel(CicpBufs f, int l, int k, int slot) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (f.state[4 * b] != 0 || f.state[4 * b + 1 + l] != 0) return;
    __shared__ double red[4][28];
    __shared__ int redi[4];
    const int cs = 2 * b * kLevels + l, ct = (2 * b + 1) * kLevels + l, tl = b * kLevels + l;
    const int ns = f.count[cs];
    const double* ps = f.pts + (long long)cs * f.cap * 3;
    const double* cls = f.col + (long long)cs * f.cap * 3;
    const double* pt = f.pts + (long long)ct * f.cap * 3;
    const double* clt = f.col + (long long)ct * f.cap * 3;
    const double* nrm = f.normal + (long long)tl * f.cap * 3;
    const double* grd = f.grad + (long long)tl * f.cap * 3;
    const int* corr = f.corr + (long long)b * f.cap;
    const double* cd2 = f.cd2 + (long long)b * f.cap;
    double* T = f.T + 16 * b;
    const double sg = sqrt(f.lambda), sc = sqrt(1.0 - f.lambda);
    double acc[28];                       // 21 of JtJ (upper triangle, row-major), 6 of Jtr, the sum of d2
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = 0.0;
    int cnt = 0;
    for (int i = tid; i < ns; i += 256) {
        const int j = corr[i];
        if (j < 0) continue;
        ++cnt;
        acc[27] += cd2[i];
        double vs[3];
        transform(T, ps + 3 * i, vs);
        const double* vt = pt + 3 * j;
        const double* nt = nrm + 3 * j;
        const double* dit = grd + 3 * j;
        const double d[3] = {vs[0] - vt[0], vs[1] - vt[1], vs[2] - vt[2]};
        const double dn = rp_dot3(d, nt);
        double JG[6], JI[6], c3[3];
        rp_cross3(vs, nt, c3);
        for (int a = 0; a < 3; ++a) { JG[a] = sg * c3[a]; JG[3 + a] = sg * nt[a]; }
        const double rG = sg * dn;
        const double pr[3] = {(vs[0] - dn * nt[0]) - vt[0], (vs[1] - dn * nt[1]) - vt[1], (vs[2] - dn * nt[2]) - vt[2]};
        const double is_proj = rp_dot3(dit, pr) + intensity(clt + 3 * j);
        const double dd = rp_dot3(dit, nt);
        const double dm[3] = {-(dit[0] - dd * nt[0]), -(dit[1] - dd * nt[1]), -(dit[2] - dd * nt[2])};
        rp_cross3(vs, dm, c3);
        for (int a = 0; a < 3; ++a) { JI[a] = sc * c3[a]; JI[3 + a] = sc * dm[a]; }
        const double rI = sc * (intensity(cls + 3 * i) - is_proj);
        int e = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = u; v < 6; ++v, ++e) acc[e] += JG[u] * JG[v] + JI[u] * JI[v];
#pragma unroll
        for (int u = 0; u < 6; ++u) acc[21 + u] += JG[u] * rG + JI[u] * rI;
    }
    // the fixed reduction of DESIGN.md §4.7 step 7: per-thread sums in voxel order, xor tree over the wave, the 4 wave sums in order
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = rp_wave_xor_sum(acc[e]);
    cnt = rp_wave_sum_i(cnt);
    if (rp_lane() == 0) {
#pragma unroll
        for (int e = 0; e < 28; ++e) red[tid >> 6][e] = acc[e];
        redi[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[28];
    for (int e = 0; e < 28; ++e) tot[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    const int ncorr = ((redi[0] + redi[1]) + redi[2]) + redi[3];
    const double fit = (double)ncorr / (double)ns;
    const double rmse = ncorr > 0 ? sqrt(tot[27] / (double)ncorr) : 0.0;
    const long long sl = (long long)b * kSlots + slot;
    if (f.iter_pose)
        for (int e = 0; e < 16; ++e) f.iter_pose[sl * 16 + e] = T[e];
    if (f.iter_ncorr) f.iter_ncorr[sl] = ncorr;
    if (f.iter_rmse) f.iter_rmse[sl] = rmse;
    if (f.fitness) f.fitness[tl] = fit;
    if (f.rmse) f.rmse[tl] = rmse;
    if (f.n_iterations) f.n_iterations[tl] = k + 1;
    bool end = k > 0 && fabs(fit - f.prev[2 * b]) < kRelFitness && fabs(rmse - f.prev[2 * b + 1]) < kRelRmse;
    f.prev[2 * b] = fit;
    f.prev[2 * b + 1] = rmse;
    if (!end) {
        double A[6][6], rhs[6], x[6] = {0, 0, 0, 0, 0, 0};
        int e = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v, ++e) A[u][v] = A[v][u] = tot[e];
        for (int u = 0; u < 6; ++u) rhs[u] = tot[21 + u];
        if (ncorr > 0 && chol_solve<6>(A, rhs, x)) {
            for (int u = 0; u < 6; ++u) x[u] = -x[u];
            if (f.iter_x)
                for (int u = 0; u < 6; ++u) f.iter_x[sl * 6 + u] = x[u];
            const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sn = sin(x[2]);
            // Rz(g) Ry(b) Rx(a)
            const double D[9] = {cg * cb, cg * sb * sa - sn * ca, cg * sb * ca + sn * sa,
                                 sn * cb, sn * sb * sa + cg * ca, sn * sb * ca - cg * sa,
                                 -sb, cb * sa, cb * ca};
            double T2[12];
            for (int a = 0; a < 3; ++a) {
                for (int c = 0; c < 3; ++c) T2[4 * a + c] = (D[3 * a] * T[c] + D[3 * a + 1] * T[4 + c]) + D[3 * a + 2] * T[8 + c];
                T2[4 * a + 3] = ((D[3 * a] * T[3] + D[3 * a + 1] * T[7]) + D[3 * a + 2] * T[11]) + x[3 + a];
            }
            for (int c = 0; c < 12; ++c) T[c] = T2[c];
        } else {
            end = true;                   // no step: the level ends with T unchanged
        }
    }
    if (end) f.state[4 * b + 1 + l] = 1;
    for (int e = 0; e < 16; ++e) {
        f.pose[16 * b + e] = T[e];
        if (f.level_pose) f.level_pose[(long long)tl * 16 + e] = T[e];
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct CicpPlan {
    size_t off_key0, off_key1, off_idx0, off_idx1, off_pts, off_col, off_vkey, off_gmb, off_gdim, off_count, off_nbr, off_ncnt, off_normal,
        off_grad, off_corr, off_cd2, off_T, off_prev, off_state, total;
};

bool cicp_plan(int B, int P, int cap, CicpPlan& p) {
    if (B <= 0 || B > 21845 || P <= 0 || cap <= 0 || cap > RELPOSE_FGR_MAX_POINTS_LIMIT || (long long)P > (1LL << 30)) return false;
    const size_t CL = 2 * (size_t)B * kLevels, TL = (size_t)B * kLevels, N = (size_t)cap, Bs = (size_t)B;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += rp_align(bytes); return o; };
    p.off_key0 = take(CL * P * 8);
    p.off_key1 = take(CL * P * 8);
    p.off_idx0 = take(CL * P * 4);
    p.off_idx1 = take(CL * P * 4);
    p.off_pts = take(CL * N * 3 * 8);
    p.off_col = take(CL * N * 3 * 8);
    p.off_vkey = take(CL * N * 8);
    p.off_gmb = take(CL * 4 * 8);
    p.off_gdim = take(CL * 4 * 8);
    p.off_count = take(CL * 4);
    p.off_nbr = take(TL * N * kNn * 4);
    p.off_ncnt = take(TL * N * 4);
    p.off_normal = take(TL * N * 3 * 8);
    p.off_grad = take(TL * N * 3 * 8);
    p.off_corr = take(Bs * N * 4);
    p.off_cd2 = take(Bs * N * 8);
    p.off_T = take(Bs * 16 * 8);
    p.off_prev = take(Bs * 2 * 8);
    p.off_state = take(Bs * 4 * 4);
    p.total = off;
    return true;
}

}  // namespace

extern "C" {

size_t relpose_cicp_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points) {
    CicpPlan p;
    return cicp_plan(n_pairs, n_points, max_points, p) ? p.total : 0;
}

int relpose_cicp(const RelposeCicpArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeCicpArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeCicpArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeCicpArgs)));
    CicpPlan p;
    if (!a.pc || !a.valid || !a.color || !a.pose || !a.status || !a.workspace || !cicp_plan(a.n_pairs, a.n_points, a.max_points, p))
        return RELPOSE_EINVAL;
    if (!(a.lambda_geometric >= 0.0 && a.lambda_geometric <= 1.0)) return RELPOSE_EINVAL;
    if (a.workspace_bytes < p.total) return RELPOSE_ENOMEM;
    hipStream_t s = (hipStream_t)a.stream;
    char* ws = (char*)a.workspace;
    const int B = a.n_pairs, N = a.max_points;
    CicpBufs f{};
    f.B = B;
    f.P = a.n_points;
    f.cap = N;
    f.lambda = a.lambda_geometric;
    f.pc = a.pc;
    f.color = a.color;
    f.valid = a.valid;
    f.init = a.init;
    f.key[0] = (long long*)(ws + p.off_key0);
    f.key[1] = (long long*)(ws + p.off_key1);
    f.idx[0] = (int*)(ws + p.off_idx0);
    f.idx[1] = (int*)(ws + p.off_idx1);
    f.pts = a.down_points ? a.down_points : (double*)(ws + p.off_pts);
    f.col = a.down_colors ? a.down_colors : (double*)(ws + p.off_col);
    f.vkey = (long long*)(ws + p.off_vkey);
    f.gmb = (double*)(ws + p.off_gmb);
    f.gdim = (long long*)(ws + p.off_gdim);
    f.count = a.down_count ? a.down_count : (int*)(ws + p.off_count);
    f.nbr = (int*)(ws + p.off_nbr);
    f.ncnt = (int*)(ws + p.off_ncnt);
    f.normal = a.normals ? a.normals : (double*)(ws + p.off_normal);
    f.grad = a.gradient ? a.gradient : (double*)(ws + p.off_grad);
    f.corr = (int*)(ws + p.off_corr);
    f.cd2 = (double*)(ws + p.off_cd2);
    f.T = (double*)(ws + p.off_T);
    f.prev = (double*)(ws + p.off_prev);
    f.state = (int*)(ws + p.off_state);
    f.pose = a.pose;
    f.status = a.status;
    f.fitness = a.fitness;
    f.rmse = a.inlier_rmse;
    f.n_iterations = a.n_iterations;
    f.level_pose = a.level_pose;
    f.iter_pose = a.iter_pose;
    f.iter_ncorr = a.iter_ncorr;
    f.iter_rmse = a.iter_rmse;
    f.iter_corr = a.iter_corr;
    f.iter_x = a.iter_x;
    hipLaunchKernelGGL(cicp_voxel_kernel, dim3(2 * B * kLevels), dim3(1024), 0, s, f);
    hipLaunchKernelGGL(cicp_neighbors_kernel, dim3(std::min(N, 1024), B * kLevels), dim3(64), 0, s, f);
    hipLaunchKernelGGL(cicp_normals_kernel, dim3((N + 255) / 256, B * kLevels), dim3(256), 0, s, f);
    hipLaunchKernelGGL(cicp_init_kernel, dim3(B), dim3(64), 0, s, f);
    int slot = 0;
    for (int l = 0; l < kLevels; ++l)
        for (int k = 0; k < kMaxIter[l]; ++k, ++slot) {
            hipLaunchKernelGGL(cicp_nn_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, f, l, slot);
            hipLaunchKernelGGL(cicp_step_kernel, dim3(B), dim3(256), 0, s, f, l, k, slot);
        }
    RP_CHECK_LAUNCH();
    // the one synchronisation: the per-pair statuses tell whether a cloud had more voxels than max_points
    int h_over = 0;
    std::vector<int> hs(B);
    RP_HIP(hipMemcpyAsync(hs.data(), a.status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    RP_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) h_over |= hs[b] == RELPOSE_CICP_STATUS_OVERFLOW;
    return h_over ? RELPOSE_CICP_OVERFLOW : 0;
}

}  // extern "C"
