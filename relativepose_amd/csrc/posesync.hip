// Robust synchronisation of pose graphs: the relative poses of a scene's view pairs -> one absolute pose per view (the
// contract stands above relpose_pose_sync in include/relpose.h, tests/sync_model.py restates it in numpy).  Built with -ffp-contract=off:
// every f64 operation is rounded on its own.  No atomics, no eigen-solver, no stopping rule: every loop has a bound known at launch.
//
//   pose_sync_kernel      one workgroup of 256 threads per scene, one launch per call.  The scene's rotations, u = R^T t, the Laplacian
//                         (64 rows of 65 doubles: the odd stride keeps a column's rows on different LDS banks) and its factor stay in LDS for
//                         all iterations; the per-edge weights and residuals (8 + 24 bytes an edge) and the adjacency lists live in the
//                         workspace.
//     edge states         one thread per edge
//     adjacency           thread (view, quarter of the edge range) counts, rp_block_excl_scan orders the counts view-major, the same threads
//                         fill: a view's entries come out in ascending edge index without a sort or an atomic
//     Prim                M steps; each: a strided arg-max over the edges, the xor butterfly inside the wave, four partials through LDS
//     an iteration        residuals and weights, one thread per edge; the Laplacian's rows and the right-hand side, one lane per view along
//                         its adjacency list; right-looking Cholesky over the workgroup (two barriers a column); the substitutions inside
//                         wave 0 with one lane per row and the pivot row's value by a lane broadcast (no barrier); the translations reuse
//                         the factor
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "cloud_prims.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxViews = RELPOSE_SYNC_MAX_VIEWS;
constexpr int kMaxEdges = RELPOSE_SYNC_MAX_EDGES;
constexpr int kMaxIterations = RELPOSE_SYNC_MAX_ITERATIONS;
constexpr int kLd = kMaxViews + 1;               // the Laplacian's row stride in doubles
constexpr double kLogSmall = 1e-6;               // |v| below it: the fallbacks of so3 log
constexpr double kExpSmall = 1e-8;               // |d|^2 below it: the series of so3 exp

struct SyncBufs {
    int n_iter, robust;
    double sr2, st2, mu0, div;
    const int* view_begin;                       // [S + 1] device copy
    const int* edge_begin;                       // [S + 1] device copy
    const int* src;
    const int* dst;
    const double* T;
    const double* w0;
    double* pose;
    int* component;
    int* tree;
    int* edge_state;
    double* confidence;
    double* res_rot;
    double* res_trans;
    int* n_components;
    double* cost;
    double* last_step;
    double* w;                                   // [E] the iteration's weights, then the cost terms
    double* vec;                                 // [E, 3] omega, then R_j^T t
    int* adj;                                    // [2 E] (edge * 64 + the other view) * 2 + (the view is the edge's dst)
};

// (a0 b0 + a1 b1) + a2 b2 everywhere
__device__ __forceinline__ void mat_mm(const double* A, const double* B, double* C) {              // C = A B
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * a + c] = (A[3 * a] * B[c] + A[3 * a + 1] * B[3 + c]) + A[3 * a + 2] * B[6 + c];
}
__device__ __forceinline__ void mat_mtm(const double* A, const double* B, double* C) {             // C = A^T B
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * a + c] = (A[a] * B[c] + A[3 + a] * B[3 + c]) + A[6 + a] * B[6 + c];
}
__device__ __forceinline__ void mat_mtv(const double* A, const double* t, double* o) {             // o = A^T t
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (A[a] * t[0] + A[3 + a] * t[1]) + A[6 + a] * t[2];
}

__device__ __forceinline__ void so3_log(const double* E, double* om) {
    const double v[3] = {E[7] - E[5], E[2] - E[6], E[3] - E[1]};
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double c = (((E[0] + E[4]) + E[8]) - 1.0) * 0.5;
    const double th = atan2(n * 0.5, c);
    if (n < kLogSmall) {
        if (c > 0) {
            om[0] = v[0] * 0.5; om[1] = v[1] * 0.5; om[2] = v[2] * 0.5;
            return;
        }
        int k = 0;                                                   // near pi: the axis from the symmetric part
        if (E[4] > E[0]) k = 1;
        if (E[8] > E[4 * k]) k = 2;
        const double omc = 1.0 - c;
        const double q = (E[4 * k] - c) / omc;
        double a[3];
        a[k] = sqrt(q < 0.0 ? 0.0 : q);
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (m != k) a[m] = (E[3 * k + m] + E[3 * m + k]) / ((2.0 * omc) * a[k]);
        const double sg = ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]) < 0 ? -1.0 : 1.0;
        const double ths = th * sg;
        om[0] = ths * a[0]; om[1] = ths * a[1]; om[2] = ths * a[2];
        return;
    }
    const double f = th / n;
    om[0] = v[0] * f; om[1] = v[1] * f; om[2] = v[2] * f;
}

__device__ __forceinline__ void so3_exp(const double* d, double* X) {
    const double d0 = d[0], d1 = d[1], d2 = d[2];
    const double t2 = (d0 * d0 + d1 * d1) + d2 * d2;
    double A, B;
    if (t2 < kExpSmall) {
        A = 1.0 - t2 / 6.0;
        B = 0.5 - t2 / 24.0;
    } else {
        const double th = sqrt(t2), sh = sin(th * 0.5);
        A = sin(th) / th;
        B = (2.0 * (sh * sh)) / t2;
    }
    X[0] = 1.0 - B * (d1 * d1 + d2 * d2);
    X[1] = B * (d0 * d1) - A * d2;
    X[2] = B * (d0 * d2) + A * d1;
    X[3] = B * (d0 * d1) + A * d2;
    X[4] = 1.0 - B * (d0 * d0 + d2 * d2);
    X[5] = B * (d1 * d2) - A * d0;
    X[6] = B * (d0 * d2) - A * d1;
    X[7] = B * (d1 * d2) + A * d0;
    X[8] = 1.0 - B * (d0 * d0 + d1 * d1);
}

// omega and rho of edge e under the poses in LDS
__device__ __forceinline__ void edge_residual(const double* T, const double* Ri, const double* Rj, const double* ui, const double* uj,
                                              double* om, double* rho) {
    const double Rij[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const double t[3] = {T[3], T[7], T[11]};
    double P[9], Em[9], c[3];
    mat_mm(Rij, Ri, P);
    mat_mtm(Rj, P, Em);
    so3_log(Em, om);
    mat_mtv(Rj, t, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) rho[a] = c[a] - (uj[a] - ui[a]);
}

// a global load of an int: not a FLAT one, which would be ordered against the LDS updates around it (common.h)
__device__ __forceinline__ int ldg_i(const int* p) { return *(RP_GLOBAL const int*)p; }

__device__ __forceinline__ double norm2(const double* x) { return (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]; }

// L x = b and L^T x = b for the factor in LDS, inside wave 0: lane = row, the pivot row's value by a lane broadcast
__device__ __forceinline__ void wave_solve(const double* s_L, const double* s_dg, int M, double* y) {
    const int lane = rp_lane();
    for (int k = 0; k < M; ++k) {
        const double dk = s_dg[k];
        double xk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xk[c] = rp_shfl_d(y[c], k) / dk;
        if (lane == k) {
            y[0] = xk[0]; y[1] = xk[1]; y[2] = xk[2];
        } else if (lane > k && lane < M) {
            const double l = s_L[lane * kLd + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = y[c] - l * xk[c];
        }
    }
    for (int k = M - 1; k >= 0; --k) {
        const double dk = s_dg[k];
        double xk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xk[c] = rp_shfl_d(y[c], k) / dk;
        if (lane == k) {
            y[0] = xk[0]; y[1] = xk[1]; y[2] = xk[2];
        } else if (lane < k) {
            const double l = s_L[k * kLd + lane];
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = y[c] - l * xk[c];
        }
    }
}

__global__ __launch_bounds__(kThreads) void pose_sync_kernel(SyncBufs b) {
    __shared__ double s_L[kMaxViews * kLd];
    __shared__ double s_R[kMaxViews * 9], s_u[kMaxViews * 3], s_dg[kMaxViews], s_pv[kMaxViews], s_red[4];
    __shared__ int s_adjb[kMaxViews + 1], s_comp[kMaxViews], s_vis[kMaxViews], s_wsum[16], s_redi[4];
    const int tid = threadIdx.x, lane = rp_lane(), wave = tid >> 6;
    const int s = blockIdx.x;
    const int v0 = b.view_begin[s], M = b.view_begin[s + 1] - v0;
    const int e0 = b.edge_begin[s], E = b.edge_begin[s + 1] - e0;
    const int* src = b.src + e0;
    const int* dst = b.dst + e0;
    const double* T = b.T + (size_t)e0 * 16;
    const double* w0 = b.w0 + e0;
    int* state = b.edge_state + e0;
    double* ws_w = b.w + e0;
    double* ws_vec = b.vec + (size_t)e0 * 3;
    int* adj = b.adj + (size_t)e0 * 2;

    // ---- edge states
    for (int e = tid; e < E; e += kThreads) {
        const int i = src[e], j = dst[e];
        const double w = w0[e];
        int st = 0;
        if (i < 0 || i >= M || j < 0 || j >= M) st = RELPOSE_SYNC_BAD_INDEX;
        else if (i == j) st = RELPOSE_SYNC_SELF_EDGE;
        else if (!(isfinite(w) && w > 0)) st = RELPOSE_SYNC_BAD_WEIGHT;
        else {
            bool ok = true;
            for (int x = 0; x < 12; ++x) ok = ok && isfinite(T[(size_t)e * 16 + x]);
            if (!ok) st = RELPOSE_SYNC_BAD_POSE;
        }
        state[e] = st;
        b.tree[e0 + e] = 0;
        b.confidence[e0 + e] = st ? 0.0 : 1.0;
        if (st) {
            b.res_rot[e0 + e] = NAN;
            b.res_trans[e0 + e] = NAN;
        }
    }
    __syncthreads();

    // ---- adjacency lists: thread (view, quarter)
    {
        const int v = tid >> 2, q = tid & 3, chunk = (E + 3) >> 2;
        const int ea = min(E, q * chunk), eb = min(E, ea + chunk);
        int cnt = 0;
        if (v < M)
            for (int e = ea; e < eb; ++e) cnt += (state[e] == 0 && (src[e] == v || dst[e] == v)) ? 1 : 0;
        int total;
        int off = rp_block_excl_scan(cnt, s_wsum, total);
        if (q == 0) s_adjb[v] = off;
        if (tid == 0) s_adjb[kMaxViews] = total;
        if (v < M)
            for (int e = ea; e < eb; ++e)
                if (state[e] == 0 && (src[e] == v || dst[e] == v)) adj[off++] = (e * 64 + (dst[e] == v ? src[e] : dst[e])) * 2 + (dst[e] == v ? 1 : 0);
    }
    if (tid < kMaxViews) {
        s_vis[tid] = 0;
        s_comp[tid] = 0;
    }
    __syncthreads();

    // ---- Prim: components, the spanning forest and the poses chained along it
    int ncomp = 0;
    for (int step = 0; step < M; ++step) {
        double bw = -1.0;
        int be = INT_MAX;
        for (int e = tid; e < E; e += kThreads) {
            if (state[e] != 0) continue;
            if (s_vis[src[e]] == s_vis[dst[e]]) continue;
            const double w = w0[e];
            if (w > bw || (w == bw && e < be)) { bw = w; be = e; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ow = rp_shfl_xor_d(bw, m);
            const int oe = __shfl_xor(be, m, 64);
            if (ow > bw || (ow == bw && oe < be)) { bw = ow; be = oe; }
        }
        if (lane == 0) { s_red[wave] = bw; s_redi[wave] = be; }
        __syncthreads();
        bw = s_red[0]; be = s_redi[0];
#pragma unroll
        for (int k = 1; k < kThreads / 64; ++k) {
            const double ow = s_red[k];
            const int oe = s_redi[k];
            if (ow > bw || (ow == bw && oe < be)) { bw = ow; be = oe; }
        }
        if (be != INT_MAX) {
            if (tid == 0) {
                const int i = src[be], j = dst[be];
                const double* Te = T + (size_t)be * 16;
                const double Rij[9] = {Te[0], Te[1], Te[2], Te[4], Te[5], Te[6], Te[8], Te[9], Te[10]};
                const double t[3] = {Te[3], Te[7], Te[11]};
                double c[3];
                if (s_vis[i]) {                                      // X_j = T X_i
                    mat_mm(Rij, s_R + 9 * i, s_R + 9 * j);
                    mat_mtv(s_R + 9 * j, t, c);
                    for (int a = 0; a < 3; ++a) s_u[3 * j + a] = s_u[3 * i + a] + c[a];
                    s_comp[j] = s_comp[i];
                    s_vis[j] = 1;
                } else {                                             // X_i = inv(T) X_j
                    mat_mtm(Rij, s_R + 9 * j, s_R + 9 * i);
                    mat_mtv(s_R + 9 * j, t, c);
                    for (int a = 0; a < 3; ++a) s_u[3 * i + a] = s_u[3 * j + a] - c[a];
                    s_comp[i] = s_comp[j];
                    s_vis[i] = 1;
                }
                b.tree[e0 + be] = 1;
            }
        } else {
            int root = 0;
            while (root < M && s_vis[root]) ++root;                  // step < M: an unvisited view exists
            ++ncomp;
            if (tid == 0 && root < M) {
                for (int x = 0; x < 9; ++x) s_R[9 * root + x] = (x == 0 || x == 4 || x == 8) ? 1.0 : 0.0;
                for (int a = 0; a < 3; ++a) s_u[3 * root + a] = 0.0;
                s_comp[root] = root;
                s_vis[root] = 1;
            }
        }
        __syncthreads();
    }

    // ---- the iterations
    double mu = b.mu0, last_step = 0.0;
    const bool is_view = tid < M;
    const bool gauge = is_view && s_comp[tid] == tid;
    const int a0 = is_view ? s_adjb[tid] : 0, a1 = is_view ? s_adjb[tid + 1] : 0;
    for (int it = 0; it < b.n_iter; ++it) {
        for (int x = tid; x < M * kLd; x += kThreads) s_L[x] = 0.0;
        const double mu2 = mu * mu;
        for (int e = tid; e < E; e += kThreads) {
            if (state[e] != 0) continue;
            const int i = src[e], j = dst[e];
            double om[3], rho[3];
            edge_residual(T + (size_t)e * 16, s_R + 9 * i, s_R + 9 * j, s_u + 3 * i, s_u + 3 * j, om, rho);
            double conf = 1.0;
            if (b.robust) {
                const double q = 1.0 + (norm2(om) / b.sr2 + norm2(rho) / b.st2) / mu2;
                conf = 1.0 / (q * q);
            }
            ws_w[e] = w0[e] * conf;
            ws_vec[3 * e] = om[0]; ws_vec[3 * e + 1] = om[1]; ws_vec[3 * e + 2] = om[2];
            if (it == b.n_iter - 1) b.confidence[e0 + e] = conf;
        }
        __syncthreads();
        double y[3] = {0.0, 0.0, 0.0};
        if (is_view) {
            if (gauge) {
                s_L[tid * kLd + tid] = 1.0;
            } else {
                double dsum = 0.0;
#pragma unroll 4
                for (int k = a0; k < a1; ++k) {
                    const int ent = ldg_i(adj + k), e = ent >> 7, o = (ent >> 1) & 63, isdst = ent & 1;
                    const double w = rp_ldg(ws_w + e);
                    dsum = dsum + w;
                    if (s_comp[o] != o) s_L[tid * kLd + o] = s_L[tid * kLd + o] - w;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double p = w * rp_ldg(ws_vec + 3 * e + c);
                        y[c] = isdst ? y[c] + p : y[c] - p;
                    }
                }
                s_L[tid * kLd + tid] = dsum;
            }
        }
        __syncthreads();
        for (int k = 0; k < M; ++k) {                                // right-looking Cholesky, the lower triangle
            const double d = sqrt(s_L[k * kLd + k]);
            if (tid == k) s_dg[k] = d;
            if (tid > k && tid < M) s_L[tid * kLd + k] = s_L[tid * kLd + k] / d;
            __syncthreads();
            const int j = k + 1 + lane;
            for (int i = k + 1 + wave; i < M; i += kThreads / 64)
                if (j <= i) s_L[i * kLd + j] = s_L[i * kLd + j] - s_L[i * kLd + k] * s_L[j * kLd + k];
            __syncthreads();
        }
        if (wave == 0) {
            wave_solve(s_L, s_dg, M, y);
            double big = 0.0;
            if (is_view && !gauge) {
                double X[9], Rn[9];
                so3_exp(y, X);
                mat_mm(s_R + 9 * tid, X, Rn);
                for (int x = 0; x < 9; ++x) s_R[9 * tid + x] = Rn[x];
                for (int c = 0; c < 3; ++c) {
                    const double a = fabs(y[c]);
                    if (a > big || a != a) big = a;
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {                      // the largest |d|; a NaN stays
                const double o = rp_shfl_xor_d(big, m);
                big = (big != big || o != o) ? NAN : fmax(big, o);
            }
            last_step = big;
        }
        __syncthreads();
        for (int e = tid; e < E; e += kThreads) {                    // R_j^T t under the new rotations
            if (state[e] != 0) continue;
            const double* Te = T + (size_t)e * 16;
            const double t[3] = {Te[3], Te[7], Te[11]};
            double c[3];
            mat_mtv(s_R + 9 * dst[e], t, c);
            ws_vec[3 * e] = c[0]; ws_vec[3 * e + 1] = c[1]; ws_vec[3 * e + 2] = c[2];
        }
        __syncthreads();
        if (wave == 0) {
            y[0] = y[1] = y[2] = 0.0;
            if (is_view && !gauge) {
#pragma unroll 4
                for (int k = a0; k < a1; ++k) {
                    const int ent = ldg_i(adj + k), e = ent >> 7, isdst = ent & 1;
                    const double w = rp_ldg(ws_w + e);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double p = w * rp_ldg(ws_vec + 3 * e + c);
                        y[c] = isdst ? y[c] + p : y[c] - p;
                    }
                }
            }
            wave_solve(s_L, s_dg, M, y);
            if (is_view) {
                s_u[3 * tid] = gauge ? 0.0 : y[0];
                s_u[3 * tid + 1] = gauge ? 0.0 : y[1];
                s_u[3 * tid + 2] = gauge ? 0.0 : y[2];
            }
        }
        __syncthreads();
        mu = fmax(mu / b.div, 1.0);
    }

    // ---- outputs
    for (int e = tid; e < E; e += kThreads) {
        if (state[e] != 0) continue;
        const int i = src[e], j = dst[e];
        double om[3], rho[3];
        edge_residual(T + (size_t)e * 16, s_R + 9 * i, s_R + 9 * j, s_u + 3 * i, s_u + 3 * j, om, rho);
        const double n_om = norm2(om), n_rho = norm2(rho);
        b.res_rot[e0 + e] = sqrt(n_om);
        b.res_trans[e0 + e] = sqrt(n_rho);
        const double r2 = (n_om / b.sr2 + n_rho / b.st2) / 1.0;
        ws_w[e] = b.robust ? w0[e] * (r2 / (1.0 + r2)) : w0[e] * r2;
    }
    __syncthreads();
    if (is_view) {
        double pv = 0.0;
        for (int k = a0; k < a1; ++k) {
            const int ent = ldg_i(adj + k);
            if (ent & 1) pv = pv + rp_ldg(ws_w + (ent >> 7));
        }
        s_pv[tid] = pv;
        const double* R = s_R + 9 * tid;
        const double* u = s_u + 3 * tid;
        double* P = b.pose + (size_t)(v0 + tid) * 16;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[4 * a] = R[3 * a]; P[4 * a + 1] = R[3 * a + 1]; P[4 * a + 2] = R[3 * a + 2];
            P[4 * a + 3] = (R[3 * a] * u[0] + R[3 * a + 1] * u[1]) + R[3 * a + 2] * u[2];
        }
        P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
        b.component[v0 + tid] = s_comp[tid];
    }
    __syncthreads();
    if (tid == 0) {
        double cost = 0.0;
        for (int v = 0; v < M; ++v) cost = cost + s_pv[v];
        b.n_components[s] = ncomp;
        b.cost[s] = cost;
        b.last_step[s] = last_step;
    }
}

// ------------------------------------------------------------------------------------------------------- host
bool sizes_ok(long long S, long long V, long long E) {
    return S >= 1 && S < (1ll << 24) && V >= 0 && E >= 0 && V <= S * kMaxViews && E <= S * kMaxEdges;
}

// the number of iterations of the schedule, or -1 beyond RELPOSE_SYNC_MAX_ITERATIONS
int iterations_of(double mu0, double div, int n_final) {
    long long n = 0;
    for (double mu = mu0; mu > 1.0; mu = std::max(mu / div, 1.0))
        if (++n > kMaxIterations) return -1;
    n += n_final;
    return n > kMaxIterations ? -1 : (int)n;
}

size_t carve(long long S, long long E, char* base, SyncBufs& k) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += rp_align(bytes); return p; };
    k.view_begin = (const int*)take(((size_t)S + 1) * sizeof(int));
    k.edge_begin = (const int*)take(((size_t)S + 1) * sizeof(int));
    k.w = (double*)take((size_t)E * sizeof(double));
    k.vec = (double*)take((size_t)E * 3 * sizeof(double));
    k.adj = (int*)take((size_t)E * 2 * sizeof(int));
    return off;
}

bool offsets_ok(const int32_t* begin, int S, int total, int limit) {
    if (begin[0] != 0 || begin[S] != total) return false;
    for (int s = 0; s < S; ++s) {
        const long long n = (long long)begin[s + 1] - begin[s];
        if (n < 0 || n > limit) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t relpose_pose_sync_workspace(int32_t n_scenes, int32_t n_views, int32_t n_edges) {
    if (!sizes_ok(n_scenes, n_views, n_edges)) return 0;
    SyncBufs k{};
    return carve(n_scenes, n_edges, nullptr, k);
}

extern "C" int relpose_pose_sync(const RelposePoseSyncArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposePoseSyncArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposePoseSyncArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposePoseSyncArgs)));
    if (!a.view_begin_host || !a.edge_begin_host || !a.src || !a.dst || !a.T || !a.w0 || !a.workspace) return RELPOSE_EINVAL;
    if (!a.pose || !a.component || !a.tree || !a.edge_state || !a.confidence || !a.res_rot || !a.res_trans || !a.n_components || !a.cost ||
        !a.last_step)
        return RELPOSE_EINVAL;
    if ((a.robust != 0 && a.robust != 1) || a.reserved0 != 0 || a.reserved1 != 0 || a.n_final < 0) return RELPOSE_EINVAL;
    if (!(std::isfinite(a.sigma_r) && a.sigma_r > 0) || !(std::isfinite(a.sigma_t) && a.sigma_t > 0)) return RELPOSE_EINVAL;
    if (!(std::isfinite(a.div) && a.div > 1.0) || !(std::isfinite(a.mu0) && a.mu0 >= 1.0)) return RELPOSE_EINVAL;
    if (!sizes_ok(a.n_scenes, a.n_views, a.n_edges)) return RELPOSE_EINVAL;
    if (!offsets_ok(a.view_begin_host, a.n_scenes, a.n_views, kMaxViews) || !offsets_ok(a.edge_begin_host, a.n_scenes, a.n_edges, kMaxEdges))
        return RELPOSE_EINVAL;
    const int n_iter = iterations_of(a.mu0, a.div, a.n_final);
    if (n_iter < 0) return RELPOSE_EINVAL;
    SyncBufs k{};
    if (a.workspace_bytes < carve(a.n_scenes, a.n_edges, nullptr, k) || ((uintptr_t)a.workspace & 255)) return RELPOSE_EINVAL;
    carve(a.n_scenes, a.n_edges, (char*)a.workspace, k);
    k.n_iter = n_iter; k.robust = a.robust;
    k.sr2 = a.sigma_r * a.sigma_r; k.st2 = a.sigma_t * a.sigma_t; k.mu0 = a.mu0; k.div = a.div;
    k.src = a.src; k.dst = a.dst; k.T = a.T; k.w0 = a.w0;
    k.pose = a.pose; k.component = a.component; k.tree = a.tree; k.edge_state = a.edge_state;
    k.confidence = a.confidence; k.res_rot = a.res_rot; k.res_trans = a.res_trans;
    k.n_components = a.n_components; k.cost = a.cost; k.last_step = a.last_step;
    hipStream_t s = (hipStream_t)a.stream;
    const size_t nb = ((size_t)a.n_scenes + 1) * sizeof(int);
    RP_HIP(hipMemcpyAsync((void*)k.view_begin, a.view_begin_host, nb, hipMemcpyHostToDevice, s));
    RP_HIP(hipMemcpyAsync((void*)k.edge_begin, a.edge_begin_host, nb, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pose_sync_kernel, dim3((unsigned)a.n_scenes), dim3(kThreads), 0, s, k);
    RP_CHECK_LAUNCH();
    RP_HIP(hipStreamSynchronize(s));                                  // the two host arrays are the caller's again
    return 0;
}
