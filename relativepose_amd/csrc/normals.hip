// Normal maps from depth panoramas: one normal per pixel of the four-face skybox grid, from the covariance of the unprojected points in a
// (2r+1)^2 window that wraps around the ring of faces.  The contract -- the fp32 expressions, the visiting order, the gate, the validity
// rule -- is DESIGN.md §4.12 and the comment above relpose_depth_normals in include/relpose.h; tests/normals_model.py restates it in
// numpy.  Built with -ffp-contract=off: count and the nine moments agree with the model bit for bit.
//
//   depth_normals_kernel<R>   one launch.  A workgroup of 256 threads owns a tile of 64 columns x 4 rows (a wave = 64 consecutive floats of
//                             one row: the depth loads and every store are coalesced).  It unprojects tile + halo once into LDS as three
//                             float arrays; the ring wrap-around and the face of every halo column are resolved there.  A pixel without data
//                             (depth 0, or a row outside the map) is staged with x = NaN: its squared distance to anything is NaN, which
//                             fails the gate, so the window loop has no test of its own for it.  Each thread then walks its window (dy
//                             ascending outer, dx ascending inner; lane l reads LDS word base + l: no bank conflicts), keeps ten scalar
//                             accumulators, solves the 3x3 covariance with a fixed number of Jacobi sweeps on named scalars (nothing is
//                             indexed at run time, nothing spills) and stores its pixel.  Tiles at the right and bottom edges are masked.
// No atomics, no workspace: a pixel's result depends on its view alone, whatever the batch around it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"

namespace {

constexpr int kTileW = 64, kTileH = 4, kThreads = kTileW * kTileH;
constexpr int kMaxR = 4;
constexpr int kSweeps = 6;       // cyclic Jacobi on a symmetric 3x3 converges quadratically: fp32 is reached in 4, two more are margin

struct NormalsBufs {
    int n, h, dataset, min_neighbors;
    float gate;                  // gate_scale * (float)r * (2.0f / (float)h), rounded after every operation
    const float* depth;          // [n, h, 4h]
    float* normal;               // [n, 3, h, 4h]
    uint8_t* valid;              // [n, h, 4h] or NULL
    int* count;                  // [n, h, 4h] or NULL
    float* moments;              // [n, 9, h, 4h] or NULL
};

// One Jacobi rotation in the (P, Q) plane of the symmetric 3x3 {a00, a01, a02, a11, a12, a22} (K = the third index; APK / AQK its couplings
// to P and Q), accumulated into the eigenvector columns P and Q.  theta * theta may overflow to +inf: t is then 0 and the rotation the
// identity.
#define RP_NJROT(APP, AQQ, APQ, APK, AQK, V0P, V1P, V2P, V0Q, V1Q, V2Q)                                 \
    if (APQ != 0.0f) {                                                                                  \
        const float theta = (AQQ - APP) / (2.0f * APQ);                                                 \
        const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));  \
        const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;                                          \
        APP = APP - t * APQ; AQQ = AQQ + t * APQ; APQ = 0.0f;                                           \
        const float pk = APK, qk = AQK;                                                                 \
        APK = c * pk - s * qk; AQK = s * pk + c * qk;                                                   \
        const float p0 = V0P, q0 = V0Q, p1 = V1P, q1 = V1Q, p2 = V2P, q2 = V2Q;                         \
        V0P = c * p0 - s * q0; V0Q = s * p0 + c * q0;                                                   \
        V1P = c * p1 - s * q1; V1Q = s * p1 + c * q1;                                                   \
        V2P = c * p2 - s * q2; V2Q = s * p2 + c * q2;                                                   \
    }

template <int R>
__global__ __launch_bounds__(kThreads) void depth_normals_kernel(NormalsBufs a) {
    constexpr int SW = kTileW + 2 * R, SH = kTileH + 2 * R;
    __shared__ float sx[SH * SW], sy[SH * SW], sz[SH * SW];
    const int h = a.h, W = 4 * h;
    const int tid = threadIdx.x, tx = tid & (kTileW - 1), ty = tid >> 6;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const size_t HW = (size_t)h * W;
    const float* dep = a.depth + (size_t)blockIdx.z * HW;
    const float fh = (float)h;

    for (int i = tid; i < SH * SW; i += kThreads) {
        const int ly = i / SW, lx = i - ly * SW;
        const int gy = y0 + ly - R;
        int gx = (x0 + lx - R) % W;                      // the ring: column 4h - 1 is next to column 0
        gx = gx < 0 ? gx + W : gx;
        const bool in = gy >= 0 && gy < h;
        const float z = in ? rp_ldg(dep + (size_t)gy * W + gx) : 0.0f;
        const int slot = gx / h, xf = gx - slot * h;
        const float xn = ((float)xf / fh - 0.5f) * 2.0f;
        const float yn = (0.5f - (float)gy / fh) * 2.0f;
        const float fx = xn * z, fy = yn * z, fz = -z;
        const int k = a.dataset == RELPOSE_SUNCG ? slot : (slot + 3) & 3;       // the face rotation: a signed permutation, exact
        float px, pz;
        if (k == 0) { px = fx; pz = fz; }
        else if (k == 1) { px = -fz; pz = fx; }
        else if (k == 2) { px = -fx; pz = -fz; }
        else { px = fz; pz = -fx; }
        sx[i] = z != 0.0f ? px : __builtin_nanf("");
        sy[i] = fy;
        sz[i] = pz;
    }
    __syncthreads();

    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= h) return;
    const size_t pix = (size_t)y * W + x;
    const float zp = rp_ldg(dep + pix);
    const int ci = (ty + R) * SW + tx + R;
    const float cx = sx[ci], cy = sy[ci], cz = sz[ci];
    const float g = a.gate * zp, g2 = g * g;             // zp == 0: cx is NaN and nothing passes

    int cnt = 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, m00 = 0.0f, m01 = 0.0f, m02 = 0.0f, m11 = 0.0f, m12 = 0.0f, m22 = 0.0f;
#pragma unroll 1
    for (int dy = 0; dy < 2 * R + 1; ++dy) {             // (one row of the window per trip: unrolled whole, r = 2 took 182 VGPRs)
        const int row = (ty + dy) * SW + tx;
#pragma unroll
        for (int dx = 0; dx < 2 * R + 1; ++dx) {
            if (dy == R && dx == R) continue;            // the centre
            const float qx = sx[row + dx] - cx, qy = sy[row + dx] - cy, qz = sz[row + dx] - cz;
            const float d2 = qx * qx + qy * qy + qz * qz;
            const bool ok = d2 <= g2;
            cnt += ok ? 1 : 0;
            // a rejected neighbour adds +0 to every sum, which leaves it as it is bit for bit: the sums start at +0, and no rounded
            // sum of two floats is -0 unless both are (three selects per neighbour instead of nine)
            const float ex = ok ? qx : 0.0f, ey = ok ? qy : 0.0f, ez = ok ? qz : 0.0f;
            s0 += ex; s1 += ey; s2 += ez;
            m00 += ex * ex; m01 += ex * ey; m02 += ex * ez;
            m11 += ey * ey; m12 += ey * ez; m22 += ez * ez;
        }
    }

    const size_t vp = (size_t)blockIdx.z * HW + pix;
    if (a.count) a.count[vp] = cnt;
    if (a.moments) {
        float* mo = a.moments + (size_t)blockIdx.z * 9 * HW + pix;
        rp_stg(mo, s0); rp_stg(mo + HW, s1); rp_stg(mo + 2 * HW, s2);
        rp_stg(mo + 3 * HW, m00); rp_stg(mo + 4 * HW, m01); rp_stg(mo + 5 * HW, m02);
        rp_stg(mo + 6 * HW, m11); rp_stg(mo + 7 * HW, m12); rp_stg(mo + 8 * HW, m22);
    }

    // covariance about the mean of the accepted points and the centre (whose difference is 0)
    const float m = (float)(cnt + 1);
    float a00 = m00 - s0 * s0 / m, a01 = m01 - s0 * s1 / m, a02 = m02 - s0 * s2 / m;
    float a11 = m11 - s1 * s1 / m, a12 = m12 - s1 * s2 / m, a22 = m22 - s2 * s2 / m;
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        RP_NJROT(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21)
        RP_NJROT(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22)
        RP_NJROT(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22)
    }
    // l0 <= l1 <= l2 of the diagonal and the column of l0
    float l0 = a00, n0 = v00, n1 = v10, n2 = v20;
    if (a11 < l0) { l0 = a11; n0 = v01; n1 = v11; n2 = v21; }
    if (a22 < l0) { l0 = a22; n0 = v02; n1 = v12; n2 = v22; }
    const float l2 = fmaxf(fmaxf(a00, a11), a22);
    const float l1 = ((a00 + a11) + a22) - l0 - l2;      // only for the collinearity test: its rounding is far inside the test's slack
    const float nrm = sqrtf(n0 * n0 + n1 * n1 + n2 * n2);
    n0 = n0 / nrm; n1 = n1 / nrm; n2 = n2 / nrm;
    if (n0 * cx + n1 * cy + n2 * cz > 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
    const bool ok = zp != 0.0f && cnt >= a.min_neighbors && l1 > 1e-6f * l2;
    float* no = a.normal + (size_t)blockIdx.z * 3 * HW + pix;
    rp_stg(no, ok ? n0 : 0.0f); rp_stg(no + HW, ok ? n1 : 0.0f); rp_stg(no + 2 * HW, ok ? n2 : 0.0f);
    if (a.valid) a.valid[vp] = ok ? 1 : 0;
}

template <int R>
void launch(const NormalsBufs& k, hipStream_t s) {
    const dim3 grid((4 * k.h + kTileW - 1) / kTileW, (k.h + kTileH - 1) / kTileH, k.n);
    hipLaunchKernelGGL(depth_normals_kernel<R>, grid, dim3(kThreads), 0, s, k);
}

}  // namespace

extern "C" int relpose_depth_normals(const RelposeDepthNormalsArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeDepthNormalsArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeDepthNormalsArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeDepthNormalsArgs)));
    if (!a.depth || !a.normal) return RELPOSE_EINVAL;
    const int r = a.radius, win = (2 * r + 1) * (2 * r + 1);
    if (r < 1 || r > kMaxR || a.n_views < 1 || a.n_views > 65535 || a.h < 2 * r + 1 || a.h > 8192) return RELPOSE_EINVAL;
    if (a.min_neighbors < 3 || a.min_neighbors > win - 1) return RELPOSE_EINVAL;
    if (!std::isfinite(a.gate_scale) || !(a.gate_scale > 0.0f)) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    NormalsBufs k{};
    k.n = a.n_views; k.h = a.h; k.dataset = a.dataset; k.min_neighbors = a.min_neighbors;
    k.gate = a.gate_scale * (float)r * (2.0f / (float)a.h);
    k.depth = a.depth; k.normal = a.normal; k.valid = a.valid; k.count = a.count; k.moments = a.moments;
    hipStream_t s = (hipStream_t)a.stream;
    if (r == 1) launch<1>(k, s);
    else if (r == 2) launch<2>(k, s);
    else if (r == 3) launch<3>(k, s);
    else launch<4>(k, s);
    RP_CHECK_LAUNCH();
    return 0;
}
