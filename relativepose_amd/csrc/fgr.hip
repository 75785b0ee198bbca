// FPFH features + fast global registration (Zhou, Park, Koltun, ECCV 2016) for a batch of point-cloud pairs: the reference's
// `--method fgs` baseline (baselines.py:36-50, 83-106).  The contract -- every constant, stage and order -- is DESIGN.md §4.6;
// tests/fgr_model.py restates it in numpy.  Built with -ffp-contract=off: the model and these kernels round alike.
//
// Clouds: c = 2b (source of pair b), 2b + 1 (target).  Kernels, each launched once per call whatever the batch size:
//   fgr_voxel_kernel      one block per cloud: min bound, voxel keys, compaction, stable LSD radix sort, segmented means (rp_voxel_downsample)
//   fgr_neighbors_kernel  one wave per query: the (d2, index)-ordered hybrid neighbour list (r 0.25, max 100) from the x-slab of the lattice
//   fgr_normals_kernel    one thread per point: covariance of the r 0.10 / 30 prefix, fixed-sweep Jacobi, turned toward the sensor
//   fgr_spfh_kernel       one thread per point, histograms in LDS
//   fgr_fpfh_kernel       one thread per point, the 33 bins in registers; also the fp32 copy the matcher reads
//   fgr_nn_kernel         one thread per query, the other cloud's features staged in LDS: exact fp32 nearest neighbour
//   fgr_match_kernel      one block per pair: mutual filter, then the tuple trials in order with a block scan
//   fgr_optimize_kernel   one block per pair: normalisation and the 64 Gauss-Newton steps, fixed-order 6x6 reduction
// The voxel downsample (scan, compaction, radix sort, segmented means), the normal of a neighbour list, the ordered block scan and the
// xor-tree reductions are cloud_prims.h's, shared with cicp.hip, ransac.hip and overlap.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cloud_prims.h"
#include "common.h"
#include "fgr_internal.h"

namespace {

constexpr double kVoxel = 0.05;
constexpr double kRFpfh = 0.25;
constexpr int kNnFpfh = 100;
constexpr double kRNormal = 0.10;
constexpr int kNnNormal = 30;
constexpr double kMaxCorr = 0.075;
constexpr double kDivision = 1.4;
constexpr int kIterations = 64;
constexpr double kTupleScale = 0.95;
constexpr int kMaxTuples = 1000;
constexpr int kMinCorr = 10;
constexpr int kSlab = 6;             // candidate voxel columns |dx| <= 6 >= r / voxel + 1
constexpr int kBuf = 256;            // per-wave candidate buffer of the neighbour search
constexpr int kFeat = 33;
constexpr int kNnStage = 64;         // targets per LDS stage of the matcher

// theta_k = -pi + 2 pi k / 11, k = 1..10, as directions; the same literals are in tests/fgr_model.py
__constant__ double kEdgeCos[10] = {-0.8412535328311811, -0.4154150130018863, 0.14231483827328512, 0.6548607339452851, 0.9594929736144975,
                                    0.9594929736144975,  0.6548607339452851,  0.14231483827328512, -0.41541501300188616, -0.8412535328311813};
__constant__ double kEdgeSin[10] = {-0.5406408174555978, -0.9096319953545184, -0.9898214418809327, -0.7557495743542583, -0.2817325568414295,
                                    0.2817325568414295,  0.7557495743542583,  0.9898214418809327,  0.9096319953545186,  0.5406408174555974};

__device__ __forceinline__ int cloud_n(const FgrBufs& f, int c) { return min(f.count[c], f.cap); }

// ------------------------------------------------------------------------------------------------------- 1. voxel downsample
// keeps every voxel's x cell: the neighbour search walks the x-slab of the lattice
struct FgrVoxelPolicy {
    static constexpr bool kExtra = false;
    int* ix;
    __device__ void lattice(const double*, long long, long long, long long) const {}
    __device__ void voxel(int o, long long key, long long ny, long long nz) const { ix[o] = (int)(key / (ny * nz)); }
};

__global__ __launch_bounds__(1024) void fgr_voxel_kernel(FgrBufs f) {
    const int c = blockIdx.x;
    const long long P = f.P;
    __shared__ RpVoxelScratch lds;
    const FgrVoxelPolicy pol{f.ix + (long long)c * f.cap};
    const int nvox = rp_voxel_downsample(f.pc + (long long)c * P * 3, f.valid + (long long)c * P, P, kVoxel, f.key[0] + (long long)c * P,
                                         f.idx[0] + (long long)c * P, f.key[1] + (long long)c * P, f.idx[1] + (long long)c * P,
                                         f.pts + (long long)c * f.cap * 3, f.cap, lds, pol);
    if (threadIdx.x == 0) f.count[c] = nvox;
}

// ------------------------------------------------------------------------------------------------------- 2. neighbours
// keep the kNnFpfh smallest (d2, index) of buf[0..m) in order at buf[0..min(m, K))
__device__ int select_k(double* bd, int* bi, double* td, int* ti, int m) {
    const int lane = threadIdx.x;
    for (int e = lane; e < m; e += 64) {
        const double de = bd[e];
        const int ie = bi[e];
        int rank = 0;
        for (int g = 0; g < m; ++g) rank += rp_lex_less(bd[g], bi[g], de, ie) ? 1 : 0;
        if (rank < kNnFpfh) { td[rank] = de; ti[rank] = ie; }
    }
    __syncthreads();
    const int k = min(m, kNnFpfh);
    for (int e = lane; e < k; e += 64) { bd[e] = td[e]; bi[e] = ti[e]; }
    __syncthreads();
    return k;
}

__global__ __launch_bounds__(64) void fgr_neighbors_kernel(FgrBufs f) {
    const int c = blockIdx.y, lane = threadIdx.x;
    __shared__ double bd[kBuf], td[kNnFpfh];
    __shared__ int bi[kBuf], ti[kNnFpfh];
    const int n = cloud_n(f, c);
    const double* pts = f.pts + (long long)c * f.cap * 3;
    const int* ix = f.ix + (long long)c * f.cap;
    const double r2 = kRFpfh * kRFpfh;
    for (int q = blockIdx.x; q < n; q += gridDim.x) {
        const double qx = pts[3 * q], qy = pts[3 * q + 1], qz = pts[3 * q + 2];
        const int lo = rp_lower_bound(ix, n, ix[q] - kSlab), hi = rp_lower_bound(ix, n, ix[q] + kSlab + 1);
        int m = 0;
        bool full = false;
        double bnd_d = 0.0;
        int bnd_i = 0;
        for (int b0 = lo; b0 < hi; b0 += 64) {
            const int cnd = b0 + lane;
            double d2 = 0.0;
            bool in = false;
            if (cnd < hi) {
                const double dx = pts[3 * cnd] - qx, dy = pts[3 * cnd + 1] - qy, dz = pts[3 * cnd + 2] - qz;
                d2 = (dx * dx + dy * dy) + dz * dz;
                in = d2 < r2 && (!full || rp_lex_less(d2, cnd, bnd_d, bnd_i));
            }
            unsigned long long msk = __ballot(in);
            if (m + __popcll(msk) > kBuf) {
                m = select_k(bd, bi, td, ti, m);
                full = true;
                bnd_d = bd[m - 1];
                bnd_i = bi[m - 1];
                in = in && rp_lex_less(d2, cnd, bnd_d, bnd_i);
                msk = __ballot(in);
            }
            if (in) {
                const int o = m + __popcll(msk & rp_lanes_below());
                bd[o] = d2;
                bi[o] = cnd;
            }
            m += __popcll(msk);
            __syncthreads();
        }
        m = select_k(bd, bi, td, ti, m);
        const long long row = (long long)c * f.cap + q;
        for (int e = lane; e < m; e += 64) {
            f.nbr[row * kNnFpfh + e] = bi[e];
            f.nd2[row * kNnFpfh + e] = bd[e];
        }
        if (lane == 0) f.ncnt[row] = m;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------- 3. normals
__global__ __launch_bounds__(256) void fgr_normals_kernel(FgrBufs f) {
    const int c = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = cloud_n(f, c);
    if (q >= n) return;
    const double* pts = f.pts + (long long)c * f.cap * 3;
    const long long row = (long long)c * f.cap + q;
    const int* nb = f.nbr + row * kNnFpfh;
    const double* nd = f.nd2 + row * kNnFpfh;
    const int cnt = f.ncnt[row];
    const double rn2 = kRNormal * kRNormal;
    int m = 0;
    while (m < cnt && m < kNnNormal && nd[m] < rn2) ++m;
    double nv[3];
    rp_normal_from_neighbors(pts, nb, m, pts + 3 * q, nv);
    for (int a = 0; a < 3; ++a) f.normal[row * 3 + a] = nv[a];
}

// ------------------------------------------------------------------------------------------------------- 4. SPFH / FPFH
__device__ __forceinline__ int lin_bin(double v) {
    const int h = (int)floor(11 * (v + 1.0) * 0.5);
    return h < 0 ? 0 : (h > 10 ? 10 : h);
}
__device__ __forceinline__ int angle_bin(double x, double y) {
    const bool upper = y >= 0;
    int b = 0;
    for (int k = 0; k < 10; ++k) {
        const bool eu = kEdgeSin[k] >= 0;
        const double cr = x * kEdgeSin[k] - y * kEdgeCos[k];
        const bool less = (!upper && eu) || (upper == eu && cr > 0);
        b += less ? 0 : 1;
    }
    return b;
}

// Open3D's ComputePairFeatures + the SPFH binning; the zero feature -> bins 5, 5, 5
__device__ void pair_bins(const double* p1, const double* n1, const double* p2, const double* n2, int* bins) {
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double L = sqrt(rp_dot3(dp, dp));
    bins[0] = bins[1] = bins[2] = 5;
    if (L == 0.0) return;
    const double a1 = rp_dot3(n1, dp) / L, a2 = rp_dot3(n2, dp) / L;
    const double* m1 = n1;
    const double* m2 = n2;
    double f2 = a1;
    if (fabs(a1) < fabs(a2)) {
        m1 = n2; m2 = n1;
        dp[0] = -dp[0]; dp[1] = -dp[1]; dp[2] = -dp[2];
        f2 = -a2;
    }
    double v[3], w[3];
    rp_cross3(dp, m1, v);
    const double vn = sqrt(rp_dot3(v, v));
    if (vn == 0.0) return;
    v[0] = v[0] / vn; v[1] = v[1] / vn; v[2] = v[2] / vn;
    rp_cross3(m1, v, w);
    bins[0] = angle_bin(rp_dot3(m1, m2), rp_dot3(w, m2));
    bins[1] = lin_bin(rp_dot3(v, m2));
    bins[2] = lin_bin(f2);
}

__global__ __launch_bounds__(64) void fgr_spfh_kernel(FgrBufs f) {
    const int c = blockIdx.y, tid = threadIdx.x;
    const int q = blockIdx.x * blockDim.x + tid;
    __shared__ double h[kFeat * 64];
    const int n = cloud_n(f, c);
    if (q >= n) return;
    for (int j = 0; j < kFeat; ++j) h[j * 64 + tid] = 0.0;
    const long long row = (long long)c * f.cap + q;
    const int cnt = f.ncnt[row];
    const double* pts = f.pts + (long long)c * f.cap * 3;
    const double* nrm = f.normal + (long long)c * f.cap * 3;
    if (cnt > 1) {
        const double incr = 100.0 / (double)(cnt - 1);
        const int* nb = f.nbr + row * kNnFpfh;
        for (int k = 1; k < cnt; ++k) {
            const int j = nb[k];
            int b[3];
            pair_bins(pts + 3 * q, nrm + 3 * q, pts + 3 * j, nrm + 3 * j, b);
            h[b[0] * 64 + tid] += incr;
            h[(11 + b[1]) * 64 + tid] += incr;
            h[(22 + b[2]) * 64 + tid] += incr;
        }
    }
    for (int j = 0; j < kFeat; ++j) f.spfh[row * kFeat + j] = h[j * 64 + tid];
}

__global__ __launch_bounds__(256) void fgr_fpfh_kernel(FgrBufs f) {
    const int c = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = cloud_n(f, c);
    if (q >= n) return;
    const long long row = (long long)c * f.cap + q;
    const int cnt = f.ncnt[row];
    double F[kFeat];
#pragma unroll
    for (int j = 0; j < kFeat; ++j) F[j] = 0.0;
    if (cnt > 1) {
        double sb[3] = {0.0, 0.0, 0.0};
        const int* nb = f.nbr + row * kNnFpfh;
        const double* nd = f.nd2 + row * kNnFpfh;
        const double* S = f.spfh + (long long)c * f.cap * kFeat;
        for (int k = 1; k < cnt; ++k) {
            const double dist = nd[k];
            if (dist == 0.0) continue;
            const double* Sk = S + (long long)nb[k] * kFeat;
#pragma unroll
            for (int j = 0; j < kFeat; ++j) {
                const double val = Sk[j] / dist;
                sb[j / 11] += val;
                F[j] += val;
            }
        }
        for (int b = 0; b < 3; ++b)
            if (sb[b] != 0.0) sb[b] = 100.0 / sb[b];
        const double* Si = S + (long long)q * kFeat;
#pragma unroll
        for (int j = 0; j < kFeat; ++j) {
            F[j] = F[j] * sb[j / 11];
            F[j] = F[j] + Si[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kFeat; ++j) {
        f.fpfh[row * kFeat + j] = F[j];
        f.f32[row * kFeat + j] = (float)F[j];
    }
}

// ------------------------------------------------------------------------------------------------------- 5. correspondences
__global__ __launch_bounds__(256) void fgr_nn_kernel(FgrBufs f) {
    const int c = blockIdx.y, tid = threadIdx.x;
    const int o = c ^ 1;                               // the other cloud of the pair
    const int nq = cloud_n(f, c), nt = cloud_n(f, o);
    const int q0 = blockIdx.x * blockDim.x;
    if (q0 >= nq) return;
    __shared__ float tf[kNnStage * kFeat];
    const int q = q0 + tid;
    float a[kFeat];
    const float* fq = f.f32 + ((long long)c * f.cap + min(q, nq - 1)) * kFeat;
#pragma unroll
    for (int k = 0; k < kFeat; ++k) a[k] = fq[k];
    const float* ft = f.f32 + (long long)o * f.cap * kFeat;
    float best = INFINITY;
    int bi = -1;
    for (int t0 = 0; t0 < nt; t0 += kNnStage) {
        const int m = min(kNnStage, nt - t0);
        for (int e = tid; e < m * kFeat; e += blockDim.x) tf[e] = ft[(long long)t0 * kFeat + e];
        __syncthreads();
        for (int t = 0; t < m; ++t) {
            float d = 0.0f;
#pragma unroll
            for (int k = 0; k < kFeat; ++k) {
                const float e = a[k] - tf[t * kFeat + k];
                d = d + e * e;
            }
            if (d < best) { best = d; bi = t0 + t; }
        }
        __syncthreads();
    }
    if (q < nq) f.nn[(long long)c * f.cap + q] = bi;
}

__global__ __launch_bounds__(1024) void fgr_match_kernel(FgrBufs f) {
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    __shared__ int wsum[16];
    const int ns = cloud_n(f, 2 * b), nt = cloud_n(f, 2 * b + 1);
    const int* nns = f.nn + (long long)(2 * b) * f.cap;
    const int* nnt = f.nn + (long long)(2 * b + 1) * f.cap;
    int* corr = f.corr + (long long)b * f.cap * 2;
    int nc = 0;
    const bool live = f.count[2 * b] <= f.cap && f.count[2 * b + 1] <= f.cap && ns >= 3 && nt >= 3;
    if (live) {
        for (int t0 = 0; t0 < ns; t0 += nth) {
            const int i = t0 + tid;
            const int j = i < ns ? nns[i] : -1;
            const bool mu = j >= 0 && nnt[j] == i;
            int tot;
            const int r = rp_block_rank(mu, wsum, tot);
            if (mu) { corr[2 * (nc + r)] = i; corr[2 * (nc + r) + 1] = j; }
            nc += tot;
        }
    }
    __syncthreads();
    int ntup = 0;
    if (nc >= 3) {
        const double* ps = f.pts + (long long)(2 * b) * f.cap * 3;
        const double* pt = f.pts + (long long)(2 * b + 1) * f.cap * 3;
        const unsigned long long base = f.seed * 0x9E3779B97F4A7C15ull;
        const long long trials = 100LL * nc;
        int* tc = f.tcorr + (long long)b * kMaxTuples * 6;
        for (long long t0 = 0; t0 < trials && ntup < kMaxTuples; t0 += nth) {
            const long long t = t0 + tid;
            bool ok = false;
            int r[3] = {0, 0, 0};
            if (t < trials) {
                for (int k = 0; k < 3; ++k) r[k] = (int)(fgr_splitmix(base + (unsigned long long)t * 3ull + (unsigned long long)k) % (unsigned long long)nc);
                const double* a0 = ps + 3 * corr[2 * r[0]];
                const double* a1 = ps + 3 * corr[2 * r[1]];
                const double* a2 = ps + 3 * corr[2 * r[2]];
                const double* c0 = pt + 3 * corr[2 * r[0] + 1];
                const double* c1 = pt + 3 * corr[2 * r[1] + 1];
                const double* c2 = pt + 3 * corr[2 * r[2] + 1];
                const double li[3] = {rp_dist3(a0, a1), rp_dist3(a1, a2), rp_dist3(a2, a0)};
                const double lj[3] = {rp_dist3(c0, c1), rp_dist3(c1, c2), rp_dist3(c2, c0)};
                ok = true;
                for (int k = 0; k < 3; ++k) ok = ok && (li[k] * kTupleScale < lj[k]) && (lj[k] < li[k] / kTupleScale);
            }
            int tot;
            const int rk = rp_block_rank(ok, wsum, tot) + ntup;
            if (ok && rk < kMaxTuples)
                for (int k = 0; k < 3; ++k) {
                    tc[2 * (3 * rk + k)] = corr[2 * r[k]];
                    tc[2 * (3 * rk + k) + 1] = corr[2 * r[k] + 1];
                }
            ntup += tot;
        }
    }
    if (tid == 0) {
        f.ncorr[b] = nc;
        f.ntup[b] = min(ntup, kMaxTuples);
    }
}

// ------------------------------------------------------------------------------------------------------- 6. optimisation
__global__ __launch_bounds__(256) void fgr_optimize_kernel(FgrBufs f) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ double red[4];
    __shared__ double sol[12];
    double* T = f.pose + (long long)b * 16;
    const int ns = cloud_n(f, 2 * b), nt = cloud_n(f, 2 * b + 1);
    int status = 0;
    if (f.count[2 * b] > f.cap || f.count[2 * b + 1] > f.cap) status = 3;
    else if (ns < 3 || nt < 3) status = 1;
    else if (f.ncorr[b] < 3 || 3 * f.ntup[b] < kMinCorr) status = 2;
    if (status != 0) {
        if (tid < 16) T[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid == 0) f.status[b] = status;
        return;
    }
    const double* ps = f.pts + (long long)(2 * b) * f.cap * 3;
    const double* pt = f.pts + (long long)(2 * b + 1) * f.cap * 3;
    double ms[3], mt[3];
    for (int a = 0; a < 3; ++a) {
        double s = 0.0, u = 0.0;
        for (int i = tid; i < ns; i += 256) s += ps[3 * i + a];
        for (int i = tid; i < nt; i += 256) u += pt[3 * i + a];
        ms[a] = rp_block_xor_sum<4>(s, red) / (double)ns;
        mt[a] = rp_block_xor_sum<4>(u, red) / (double)nt;
    }
    double mx = 0.0;
    for (int i = tid; i < ns; i += 256) {
        const double d[3] = {ps[3 * i] - ms[0], ps[3 * i + 1] - ms[1], ps[3 * i + 2] - ms[2]};
        mx = fmax(mx, sqrt(rp_dot3(d, d)));
    }
    for (int i = tid; i < nt; i += 256) {
        const double d[3] = {pt[3 * i] - mt[0], pt[3 * i + 1] - mt[1], pt[3 * i + 2] - mt[2]};
        mx = fmax(mx, sqrt(rp_dot3(d, d)));
    }
    const double scale = rp_block_max<4>(mx, red);
    const int m = 3 * f.ntup[b];
    const int* tc = f.tcorr + (long long)b * kMaxTuples * 6;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    double par = 1.0;
    for (int itr = 0; itr < kIterations; ++itr) {
        if (itr % 4 == 0 && par > kMaxCorr) par /= kDivision;
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int cc = tid; cc < m; cc += 256) {
            const int i = tc[2 * cc], j = tc[2 * cc + 1];
            const double p[3] = {(ps[3 * i] - ms[0]) / scale, (ps[3 * i + 1] - ms[1]) / scale, (ps[3 * i + 2] - ms[2]) / scale};
            const double q0[3] = {(pt[3 * j] - mt[0]) / scale, (pt[3 * j + 1] - mt[1]) / scale, (pt[3 * j + 2] - mt[2]) / scale};
            double q[3];
            for (int a = 0; a < 3; ++a) q[a] = ((R[3 * a] * q0[0] + R[3 * a + 1] * q0[1]) + R[3 * a + 2] * q0[2]) + t[a];
            const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
            const double w = par / (rp_dot3(r, r) + par);
            const double s = w * w;
            const double J[3][6] = {{0, -q[2], q[1], -1, 0, 0}, {q[2], 0, -q[0], 0, -1, 0}, {-q[1], q[0], 0, 0, 0, -1}};
            int k = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u)
#pragma unroll
                for (int v = u; v < 6; ++v, ++k)
                    acc[k] += s * ((J[0][u] * J[0][v] + J[1][u] * J[1][v]) + J[2][u] * J[2][v]);
#pragma unroll
            for (int u = 0; u < 6; ++u) acc[21 + u] += s * ((J[0][u] * r[0] + J[1][u] * r[1]) + J[2][u] * r[2]);
        }
        double tot[27];
        for (int k = 0; k < 27; ++k) tot[k] = rp_block_xor_sum<4>(acc[k], red);
        if (tid == 0) {
            double A[6][6], L[6][6] = {}, y[6], x[6] = {0, 0, 0, 0, 0, 0};
            int k = 0;
            for (int u = 0; u < 6; ++u)
                for (int v = u; v < 6; ++v, ++k) A[u][v] = A[v][u] = tot[k];
            bool ok = true;
            // Every product is subtracted from the running value; cicp.hip's chol_solve sums the products from 0 and subtracts once.  The two
            // round differently and each is pinned by its own numpy model: do not unify them.
            for (int j = 0; j < 6 && ok; ++j) {
                double s = A[j][j];
                for (int kk = 0; kk < j; ++kk) s -= L[j][kk] * L[j][kk];
                if (!(s > 0)) { ok = false; break; }
                L[j][j] = sqrt(s);
                for (int i = j + 1; i < 6; ++i) {
                    double v = A[i][j];
                    for (int kk = 0; kk < j; ++kk) v -= L[i][kk] * L[j][kk];
                    L[i][j] = v / L[j][j];
                }
            }
            if (ok) {
                for (int i = 0; i < 6; ++i) {
                    double v = tot[21 + i];
                    for (int kk = 0; kk < i; ++kk) v -= L[i][kk] * y[kk];
                    y[i] = v / L[i][i];
                }
                for (int i = 5; i >= 0; --i) {
                    double v = y[i];
                    for (int kk = i + 1; kk < 6; ++kk) v -= L[kk][i] * x[kk];
                    x[i] = v / L[i][i];
                }
            }
            for (int i = 0; i < 6; ++i) sol[i] = -x[i];
        }
        __syncthreads();
        const double ca = cos(sol[0]), sa = sin(sol[0]), cb = cos(sol[1]), sb = sin(sol[1]), cg = cos(sol[2]), sg = sin(sol[2]);
        // Rz(g) Ry(b) Rx(a)
        const double D[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                             sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                             -sb, cb * sa, cb * ca};
        double R2[9], t2[3];
        for (int a = 0; a < 3; ++a) {
            for (int e = 0; e < 3; ++e) R2[3 * a + e] = (D[3 * a] * R[e] + D[3 * a + 1] * R[3 + e]) + D[3 * a + 2] * R[6 + e];
            t2[a] = ((D[3 * a] * t[0] + D[3 * a + 1] * t[1]) + D[3 * a + 2] * t[2]) + sol[3 + a];
        }
        for (int e = 0; e < 9; ++e) R[e] = R2[e];
        for (int a = 0; a < 3; ++a) t[a] = t2[a];
        __syncthreads();
    }
    if (tid == 0) {
        double tt[3];
        for (int a = 0; a < 3; ++a) tt[a] = -((R[3 * a] * mt[0] + R[3 * a + 1] * mt[1]) + R[3 * a + 2] * mt[2]) + t[a] * scale + ms[a];
        for (int a = 0; a < 3; ++a) {
            for (int e = 0; e < 3; ++e) T[4 * a + e] = R[3 * e + a];
            T[4 * a + 3] = -((R[a] * tt[0] + R[3 + a] * tt[1]) + R[6 + a] * tt[2]);
        }
        T[12] = T[13] = T[14] = 0.0;
        T[15] = 1.0;
        f.status[b] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct FgrPlan {
    size_t off_key0, off_key1, off_idx0, off_idx1, off_pts, off_ix, off_count, off_nbr, off_nd2, off_ncnt, off_normal, off_spfh, off_fpfh,
        off_f32, off_nn, off_corr, off_ncorr, off_tcorr, off_ntup, off_pose, total;
};

bool fgr_plan(int B, int P, int cap, FgrPlan& p) {
    if (B <= 0 || P <= 0 || cap <= 0 || cap > RELPOSE_FGR_MAX_POINTS_LIMIT || (long long)P > (1LL << 30)) return false;
    const size_t C = 2 * (size_t)B, N = (size_t)cap;
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
    p.off_corr = take((size_t)B * N * 2 * 4);
    p.off_ncorr = take((size_t)B * 4);
    p.off_tcorr = take((size_t)B * kMaxTuples * 6 * 4);
    p.off_ntup = take((size_t)B * 4);
    p.off_pose = take((size_t)B * 16 * 8);
    p.total = off;
    return true;
}

}  // namespace

void fgr_front_end(const FgrBufs& f, hipStream_t s) {
    const int C = f.n_clouds, N = f.cap;
    const dim3 per_point((N + 255) / 256, C), per_point64((N + 63) / 64, C);
    hipLaunchKernelGGL(fgr_voxel_kernel, dim3(C), dim3(1024), 0, s, f);
    hipLaunchKernelGGL(fgr_neighbors_kernel, dim3(std::min(N, 1024), C), dim3(64), 0, s, f);
    hipLaunchKernelGGL(fgr_normals_kernel, per_point, dim3(256), 0, s, f);
    hipLaunchKernelGGL(fgr_spfh_kernel, per_point64, dim3(64), 0, s, f);
    hipLaunchKernelGGL(fgr_fpfh_kernel, per_point, dim3(256), 0, s, f);
    hipLaunchKernelGGL(fgr_nn_kernel, per_point, dim3(256), 0, s, f);
}

extern "C" {

size_t relpose_fgr_workspace_bytes(int32_t n_pairs, int32_t n_points, int32_t max_points) {
    FgrPlan p;
    return fgr_plan(n_pairs, n_points, max_points, p) ? p.total : 0;
}

int relpose_fgr(const RelposeFgrArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeFgrArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeFgrArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeFgrArgs)));
    FgrPlan p;
    if (!a.pc || !a.valid || !a.pose || !a.status || !a.workspace || !fgr_plan(a.n_pairs, a.n_points, a.max_points, p)) return RELPOSE_EINVAL;
    if (a.workspace_bytes < p.total) return RELPOSE_ENOMEM;
    hipStream_t s = (hipStream_t)a.stream;
    char* ws = (char*)a.workspace;
    const int B = a.n_pairs, C = 2 * B, N = a.max_points;
    FgrBufs f{};
    f.n_clouds = C;
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
    f.nbr = a.nbr_index ? a.nbr_index : (int*)(ws + p.off_nbr);
    f.nd2 = (double*)(ws + p.off_nd2);
    f.ncnt = a.nbr_count ? a.nbr_count : (int*)(ws + p.off_ncnt);
    f.normal = a.normals ? a.normals : (double*)(ws + p.off_normal);
    f.spfh = (double*)(ws + p.off_spfh);
    f.fpfh = a.fpfh ? a.fpfh : (double*)(ws + p.off_fpfh);
    f.f32 = (float*)(ws + p.off_f32);
    f.nn = (int*)(ws + p.off_nn);
    f.corr = a.corr ? a.corr : (int*)(ws + p.off_corr);
    f.ncorr = a.n_corr ? a.n_corr : (int*)(ws + p.off_ncorr);
    f.tcorr = a.tuple_corr ? a.tuple_corr : (int*)(ws + p.off_tcorr);
    f.ntup = a.n_tuples ? a.n_tuples : (int*)(ws + p.off_ntup);
    f.pose = a.pose;
    f.status = a.status;
    f.seed = a.seed;
    fgr_front_end(f, s);
    hipLaunchKernelGGL(fgr_match_kernel, dim3(B), dim3(1024), 0, s, f);
    hipLaunchKernelGGL(fgr_optimize_kernel, dim3(B), dim3(256), 0, s, f);
    RP_CHECK_LAUNCH();
    // the one synchronisation: the per-pair statuses tell whether a cloud had more voxels than max_points
    int h_over = 0;
    std::vector<int> hs(B);
    RP_HIP(hipMemcpyAsync(hs.data(), a.status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    RP_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) h_over |= hs[b] == RELPOSE_FGR_STATUS_OVERFLOW;
    return h_over ? RELPOSE_FGR_OVERFLOW : 0;
}

}  // extern "C"
