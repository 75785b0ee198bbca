// The arithmetic of relpose_tsdf_align (the contract stands above the declaration in include/relpose.h, tests/align_model.py
// restates it in numpy): the rigid inverse, a point's class and quantised row, and a view's step -- the exact int64 -> f64 conversion, a cyclic
// Jacobi eigen-solve with a fixed sweep count, the eigenvalue floor and the Cayley update.  Only + - * / sqrt floor llrint, one statement per
// rounding: the including file is built with -ffp-contract=off.  The functions are __host__ __device__ and depend on <cmath> alone, so a host
// program can run this very text against the model.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#define RP_ALIGN_FN __host__ __device__ __forceinline__

constexpr int kAlignSums = 32;                   // 21 JtJ (upper triangle, row-major) + 6 Jtr + r^2 + outside, unknown, saturated, used
constexpr int kAlignOutside = 28, kAlignUnknown = 29, kAlignSaturated = 30, kAlignUsed = 31;
constexpr int kAlignSweeps = 8;
constexpr double kAlignFix = 32768.0;            // relpose_tsdf_fuse's: tsdf_sum counts t in 1 / 32768
constexpr double kAlignScaleRot = 256.0;         // l x g in 1 / 2^8
constexpr double kAlignScaleTrans = 65536.0;     // g in 1 / 2^16
constexpr double kAlignScaleRes = 65536.0;       // r in 1 / 2^16

struct AlignVolume {
    int nx, ny, nz, min_weight;
    double voxel;
    double origin[3];
    double centre[3];                            // origin_a + (n_a * 0.5) * voxel
    const int* tsdf;                             // the scene's [nz, ny, nx]
    const int* weight;
};

// world -> camera T (row-major 4 x 4, the last row is not read) -> camera -> world W [3][4]
RP_ALIGN_FN void align_inverse(const double* T, double* W) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) W[4 * a + b] = T[4 * b + a];
        W[4 * a + 3] = -((T[a] * T[3] + T[4 + a] * T[7]) + T[8 + a] * T[11]);
    }
}

// The class of the camera-frame point (x, y, z) under W (kAlignOutside .. kAlignUsed) and, for a used point, its quantised row and residual.
RP_ALIGN_FN int align_row(const AlignVolume& g, const double* W, double x, double y, double z, long long Jq[6], long long& rq) {
    double q[3], fl[3], f[3];
    int i0[3];
    const int n[3] = {g.nx, g.ny, g.nz};
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        q[a] = ((W[4 * a] * x + W[4 * a + 1] * y) + W[4 * a + 2] * z) + W[4 * a + 3];
        in = in && std::isfinite(q[a]);
    }
    if (!in) return kAlignOutside;
    for (int a = 0; a < 3; ++a) {
        const double u = (q[a] - g.origin[a]) / g.voxel - 0.5;
        fl[a] = floor(u);
        in = in && fl[a] >= 0.0 && fl[a] <= (double)(n[a] - 2);
        f[a] = u - fl[a];
    }
    if (!in) return kAlignOutside;                                   // nothing is read for such a point
    for (int a = 0; a < 3; ++a) i0[a] = (int)fl[a];
    double t[8];
    bool known = true, sat = false;
    for (int c = 0; c < 8; ++c) {
        const size_t lin = ((size_t)(i0[2] + (c >> 2 & 1)) * (size_t)g.ny + (size_t)(i0[1] + (c >> 1 & 1))) * (size_t)g.nx + (size_t)(i0[0] + (c & 1));
        const int w = g.weight[lin];
        const int s = g.tsdf[lin];
        if (w < g.min_weight) {
            known = false;
            t[c] = 0.0;
        } else {
            t[c] = (double)s / (kAlignFix * (double)w);
            sat = sat || fabs(t[c]) >= 1.0;
        }
    }
    if (!known) return kAlignUnknown;
    if (sat) return kAlignSaturated;
    const double d00 = t[1] - t[0], d10 = t[3] - t[2], d01 = t[5] - t[4], d11 = t[7] - t[6];
    const double a00 = t[0] + f[0] * d00, a10 = t[2] + f[0] * d10, a01 = t[4] + f[0] * d01, a11 = t[6] + f[0] * d11;
    const double c0 = a10 - a00, c1 = a11 - a01;
    const double b0 = a00 + f[1] * c0, b1 = a01 + f[1] * c1;
    const double gz = b1 - b0;
    const double r = b0 + f[2] * gz;
    const double gy = c0 + f[2] * (c1 - c0);
    const double e0 = d00 + f[1] * (d10 - d00), e1 = d01 + f[1] * (d11 - d01);
    const double gx = e0 + f[2] * (e1 - e0);
    const double l0 = (q[0] - g.centre[0]) / g.voxel, l1 = (q[1] - g.centre[1]) / g.voxel, l2 = (q[2] - g.centre[2]) / g.voxel;
    Jq[0] = llrint((l1 * gz - l2 * gy) * kAlignScaleRot);
    Jq[1] = llrint((l2 * gx - l0 * gz) * kAlignScaleRot);
    Jq[2] = llrint((l0 * gy - l1 * gx) * kAlignScaleRot);
    Jq[3] = llrint(gx * kAlignScaleTrans);
    Jq[4] = llrint(gy * kAlignScaleTrans);
    Jq[5] = llrint(gz * kAlignScaleTrans);
    rq = llrint(r * kAlignScaleRes);
    return kAlignUsed;
}

// sums += the row's 28 products (the class count is the caller's).  |Jq| <= 2^20 and |rq| <= 2^16 fit an int: 32 x 32 -> 64 bit products
RP_ALIGN_FN void align_add_row(long long* sums, const long long Jq[6], long long rq) {
    int J[6];
    for (int i = 0; i < 6; ++i) J[i] = (int)Jq[i];
    const int r = (int)rq;
    int n = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) sums[n++] += (long long)J[i] * (long long)J[j];
    for (int i = 0; i < 6; ++i) sums[21 + i] += (long long)J[i] * (long long)r;
    sums[27] += (long long)r * (long long)r;
}

RP_ALIGN_FN double align_rms(const long long* sums) {
    const long long n = sums[kAlignUsed];
    return n > 0 ? sqrt((double)sums[27] / (double)n) / kAlignScaleRes : 0.0;
}

// One view's step from its integer sums: eig [6] ascending (lambda / n_used; 0 without a used point), the number of held directions, and
// Tout = T D^-1 (T itself, bit for bit, when fewer than 6 points were used or move is false).  T and Tout may be the same 16 doubles.
RP_ALIGN_FN void align_step(const long long* sums, const double* Tin, const AlignVolume& g, double eig_min, bool move, double* Tout, double* eig,
                            int& held) {
    const double scale[6] = {kAlignScaleRot, kAlignScaleRot, kAlignScaleRot, kAlignScaleTrans, kAlignScaleTrans, kAlignScaleTrans};
    double A[6][6], V[6][6], b[6], T[16];
    for (int e = 0; e < 16; ++e) T[e] = Tin[e];
    int m = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            A[i][j] = (double)sums[m++] / (scale[i] * scale[j]);
            A[j][i] = A[i][j];
        }
    for (int i = 0; i < 6; ++i) {
        b[i] = (double)sums[21 + i] / (scale[i] * kAlignScaleRes);
        for (int j = 0; j < 6; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    }
    // p, q and k are unrolled so that every index is a constant and A, V stay in registers; the sweeps are a loop
#pragma unroll 1
    for (int sweep = 0; sweep < kAlignSweeps; ++sweep)
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double tt = theta * theta;
                const double den = fabs(theta) + sqrt(tt + 1.0);
                const double t = theta >= 0.0 ? 1.0 / den : -(1.0 / den);
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = c * akp - s * akq;
                        A[p][k] = A[k][p];
                        A[k][q] = s * akp + c * akq;
                        A[q][k] = A[k][q];
                    }
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    const long long n = sums[kAlignUsed];
    const double nn = (double)n;
    for (int k = 0; k < 6; ++k) eig[k] = n > 0 ? A[k][k] / nn : 0.0;
    for (int i = 1; i < 6; ++i) {                                    // ascending
        const double v = eig[i];
        int j = i - 1;
        while (j >= 0 && eig[j] > v) {
            eig[j + 1] = eig[j];
            --j;
        }
        eig[j + 1] = v;
    }
    const double floor_ = eig_min * nn;
    double coef[6], delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    held = 0;
    for (int k = 0; k < 6; ++k) {
        coef[k] = 0.0;
        if (n >= 6 && A[k][k] > floor_) {
            double vb = 0.0;
            for (int i = 0; i < 6; ++i) vb = vb + V[i][k] * b[i];
            coef[k] = -(vb / A[k][k]);
        } else {
            ++held;
        }
    }
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < 6; ++i) delta[i] = delta[i] + V[i][k] * coef[k];
    for (int e = 0; e < 16; ++e) Tout[e] = T[e];
    if (!move || n < 6) return;
    // the world-frame motion x -> c + Rd (x - c) + voxel tau, Rd the Cayley rotation of the vector delta[0..2]
    const double a0 = delta[0] * 0.5, a1 = delta[1] * 0.5, a2 = delta[2] * 0.5;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1.0 + aa, om = 1.0 - aa;
    double Rd[3][3];
    Rd[0][0] = (om + 2.0 * (a0 * a0)) / den;
    Rd[1][1] = (om + 2.0 * (a1 * a1)) / den;
    Rd[2][2] = (om + 2.0 * (a2 * a2)) / den;
    Rd[0][1] = (2.0 * (a0 * a1 - a2)) / den;
    Rd[1][0] = (2.0 * (a0 * a1 + a2)) / den;
    Rd[0][2] = (2.0 * (a0 * a2 + a1)) / den;
    Rd[2][0] = (2.0 * (a0 * a2 - a1)) / den;
    Rd[1][2] = (2.0 * (a1 * a2 - a0)) / den;
    Rd[2][1] = (2.0 * (a1 * a2 + a0)) / den;
    double d[3];
    for (int i = 0; i < 3; ++i)
        d[i] = (g.centre[i] - ((Rd[i][0] * g.centre[0] + Rd[i][1] * g.centre[1]) + Rd[i][2] * g.centre[2])) + g.voxel * delta[3 + i];
    for (int i = 0; i < 3; ++i) {
        double nr[3];
        for (int j = 0; j < 3; ++j) nr[j] = (T[4 * i] * Rd[j][0] + T[4 * i + 1] * Rd[j][1]) + T[4 * i + 2] * Rd[j][2];      // (R_T Rd^T)_ij
        Tout[4 * i] = nr[0];
        Tout[4 * i + 1] = nr[1];
        Tout[4 * i + 2] = nr[2];
        Tout[4 * i + 3] = T[4 * i + 3] - ((nr[0] * d[0] + nr[1] * d[1]) + nr[2] * d[2]);
    }
}
