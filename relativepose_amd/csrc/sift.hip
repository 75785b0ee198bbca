// SIFT keypoint detector (positions only), batched over views: the detector behind rputil.getKeypoint / getKeypoint_kinect
// (cv2.xfeatures2d.SIFT_create(contrastThreshold=0.02).detectAndCompute, rputil.py:152-172, :253-265).  Lowe's scale space
// (IJCV 60(2), 2004) with 3 layers per octave, sigma 1.6, contrast 0.02, edge ratio 10 and the image doubled first.  The detection
// contract -- what every step computes, in which order the floating-point sums run -- is DESIGN.md's "SIFT detector" section;
// tests/sift_model.py implements the same contract in numpy.  Compiled with -ffp-contract=off: no FMA contraction, so the blur,
// the differences of Gaussians and the refinement round exactly like the float32 model.  The source image, its gray value and the border
// rule are sift_common.h's, shared with siftdesc.hip.
//
// Launches (none of them depends on the number of views; views are the z / y grid dimension of each):
//   per octave   layer 0 (octave 0: gray + x2 upsample + base blur, fused; later octaves: every second pixel of layer 3 before),
//                5 blurs (LDS tile, rows then columns, the DoG of the previous layer as epilogue), extremum detection (wave-aggregated append)
//   then         refinement (one lane per candidate), orientation histograms (one wave per keypoint), per-view bitonic sort + dedup
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>

#include "cloud_prims.h"
#include "common.h"
#include "sift_common.h"

namespace {

constexpr int SIFT_NG = 6;          // Gaussian layers per octave (3 + 3)
constexpr int SIFT_ND = 5;          // DoG layers per octave
constexpr int SIFT_BORDER = 5;
constexpr int SIFT_MAX_OCT = 10;    // RELPOSE_SIFT_MAX_SIDE 2048: round(log2 2048 - 2) + 1 = 10 octaves (4 bits of kp_code)
constexpr int SIFT_RMAX = 13;       // radius of the widest tap table (sigma_5 = 3.09: 27 taps)
constexpr int SIFT_MAX_STEPS = 5;
constexpr int SIFT_HIST = 36;
constexpr int SIFT_SORT_LDS = 4096; // keypoints per view sorted in LDS (5 floats each: 80 KB); larger views sort in their global stage lists
constexpr int BT_W = 64, BT_H = 16; // blur output tile

struct SiftTaps {
    float t[2 * SIFT_RMAX + 1];
    int r;
};

// candidate / keypoint location: c 12 bits, r 12 bits, layer 2 bits, octave 4 bits
__device__ inline int kp_code(int o, int l, int r, int c) { return (o << 26) | (l << 24) | (r << 12) | c; }
__device__ inline void kp_decode(int code, int& o, int& l, int& r, int& c) {
    c = code & 4095; r = (code >> 12) & 4095; l = (code >> 24) & 3; o = (code >> 26) & 15;
}

struct SiftGeom {
    int n_oct, V;
    int H[SIFT_MAX_OCT], W[SIFT_MAX_OCT];
    long long g_off[SIFT_MAX_OCT], d_off[SIFT_MAX_OCT];   // floats: octave o's [V][6][H][W] Gaussians / [V][5][H][W] DoGs
};

// Wave-aggregated append: every active lane with `want` gets a slot in the list behind `counter` (one atomic per wave).
__device__ inline int wave_append(bool want, int* counter) {
    const unsigned long long m = __ballot(want);
    if (!m) return -1;
    const int lane = rp_lane();
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader, 64);
    return want ? base + __popcll(m & rp_lanes_below()) : -1;
}

// ------------------------------------------------------------------------------------------------------------------ gray + blur
// x2 bilinear upsample with half-pixel centres: taps 3/4 (nearer source pixel), 1/4 (the other neighbour, edge clamped)
__device__ inline float up_at(const SiftImage& s, const uint8_t* im, int gy, int gx) {
    const int ny = gy >> 1, fy = (gy & 1) ? min(ny + 1, s.h - 1) : max(ny - 1, 0);
    const int nx = gx >> 1, fx = (gx & 1) ? min(nx + 1, s.w - 1) : max(nx - 1, 0);
    const float a = (float)sift_gray_at(s, im, ny, nx), b = (float)sift_gray_at(s, im, ny, fx);
    const float c = (float)sift_gray_at(s, im, fy, nx), d = (float)sift_gray_at(s, im, fy, fx);
    return 0.75f * (0.75f * a + 0.25f * b) + 0.25f * (0.75f * c + 0.25f * d);
}

__global__ __launch_bounds__(256) void sift_gray_kernel(SiftImage s, uint8_t* __restrict__ gray) {
    const int v = blockIdx.y;
    const int n = s.w * s.h;
    const uint8_t* im = s.img + v * s.vstride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        gray[(long long)v * n + i] = (uint8_t)sift_gray_at(s, im, i / s.w, i % s.w);
}

// One Gaussian layer: dst = blur(src) (rows first, then columns, float32 intermediate, reflect-101 border), taps summed in index order.
// UP: the source is the gray crop of the uint8 images, upsampled x2 on the fly (octave 0 layer 0).  dog != NULL: also dog = dst - src.
template <bool UP>
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ src, long long src_vstride, SiftImage s, float* __restrict__ dst,
                                                        long long dst_vstride, float* __restrict__ dog, long long dog_vstride, int H, int W, SiftTaps tp) {
    __shared__ float tin[BT_H + 2 * SIFT_RMAX][BT_W + 2 * SIFT_RMAX];
    __shared__ float tmid[BT_H + 2 * SIFT_RMAX][BT_W];
    const int R = tp.r, v = blockIdx.z;
    const int x0 = blockIdx.x * BT_W, y0 = blockIdx.y * BT_H;
    const int rows = BT_H + 2 * R, cols = BT_W + 2 * R;
    const float* sv = src + v * src_vstride;
    const uint8_t* im = UP ? s.img + v * s.vstride : nullptr;
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const int gy = sift_refl101(y0 + ly - R, H), gx = sift_refl101(x0 + lx - R, W);
        tin[ly][lx] = UP ? up_at(s, im, gy, gx) : sv[(long long)gy * W + gx];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * BT_W; i += 256) {
        const int ly = i / BT_W, lx = i - ly * BT_W;
        float acc = tp.t[0] * tin[ly][lx];
        for (int j = 1; j <= 2 * R; ++j) acc = acc + tp.t[j] * tin[ly][lx + j];
        tmid[ly][lx] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BT_H * BT_W; i += 256) {
        const int ly = i / BT_W, lx = i - ly * BT_W;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float acc = tp.t[0] * tmid[ly][lx];
        for (int j = 1; j <= 2 * R; ++j) acc = acc + tp.t[j] * tmid[ly + j][lx];
        const long long o = (long long)gy * W + gx;
        dst[v * dst_vstride + o] = acc;
        if (dog) dog[v * dog_vstride + o] = acc - tin[ly + R][lx + R];
    }
}

// layer 0 of octave o > 0: every second pixel (from 0) of layer 3 of octave o-1
__global__ __launch_bounds__(256) void sift_down_kernel(const float* __restrict__ src, long long src_vstride, int Ws, float* __restrict__ dst,
                                                        long long dst_vstride, int H, int W) {
    const int v = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        dst[v * dst_vstride + i] = src[v * src_vstride + (long long)(2 * y) * Ws + 2 * x];
    }
}

// ------------------------------------------------------------------------------------------------------------------ extrema
// DoG layers 1..3 of one octave, 5-pixel border: a positive value >= its 26 neighbours or a negative one <= them (|D| > 0: the threshold
// floor(0.5 * 0.02 / 3 * 255) is 0).  Appended to the view's candidate list.
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ dog, int H, int W, int oct, int* __restrict__ cand,
                                                           long long cand_cap, int* __restrict__ cand_count) {
    const int v = blockIdx.z, l = 1 + blockIdx.y;
    const int iw = W - 2 * SIFT_BORDER, n = iw * (H - 2 * SIFT_BORDER);
    const long long P = (long long)H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    int r = 0, c = 0;
    if (i < n) {
        r = SIFT_BORDER + i / iw;
        c = SIFT_BORDER + i % iw;
        const float* d = dog + ((long long)v * SIFT_ND + l) * P + (long long)r * W + c;
        const float v0 = d[0];
        const int sgn = v0 > 0.f ? 1 : (v0 < 0.f ? -1 : 0);
        hit = sgn != 0;
        for (int k = 0; k < 27 && hit; ++k) {
            if (k == 13) continue;
            const int dl = k / 9 - 1, dy = (k / 3) % 3 - 1, dx = k % 3 - 1;
            const float u = d[dl * P + dy * W + dx];
            hit = sgn > 0 ? v0 >= u : v0 <= u;
        }
    }
    const int slot = wave_append(hit, cand_count + v);
    if (hit && slot < cand_cap) cand[v * cand_cap + slot] = kp_code(oct, l, r, c);
}

// ------------------------------------------------------------------------------------------------------------------ refinement
struct RefKp {
    int code;            // octave, layer, row, column after refinement
    float x, y, size, response, scale;   // output position / diameter (crop frame), |contrast|, sigma in octave units
};

// Up to 5 Newton steps on (x, y, layer); contrast and edge tests (SIFT detector, step 6).  One lane per candidate.
__global__ __launch_bounds__(256) void sift_refine_kernel(const float* __restrict__ dogs, SiftGeom g, const int* __restrict__ cand, long long cand_cap,
                                                          const int* __restrict__ cand_count, RefKp* __restrict__ ref, int ref_cap, int* __restrict__ ref_count) {
    const int v = blockIdx.y;
    const long long ncand = min((long long)cand_count[v], cand_cap);
    const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    const int wave = threadIdx.x >> 6, stride = gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256 + wave * 64; base < ncand; base += stride) {
        const long long i = base + rp_lane();
        bool keep = false;
        RefKp kp{};
        if (i < ncand) {
            int o, l, r, c;
            kp_decode(cand[v * cand_cap + i], o, l, r, c);
            const int H = g.H[o], W = g.W[o];
            const long long P = (long long)H * W;
            const float* Db = dogs + g.d_off[o] + (long long)v * SIFT_ND * P;
            float gx = 0.f, gy = 0.f, gs = 0.f, dxx = 0.f, dyy = 0.f, dxy = 0.f, xc = 0.f, xr = 0.f, xs = 0.f, val = 0.f;
            int state = 0;       // 0 running, 1 converged, 2 rejected
            for (int it = 0; it < SIFT_MAX_STEPS && state == 0; ++it) {
                const float* im = Db + l * P + (long long)r * W + c;
                const float* pv = im - P;
                const float* nx = im + P;
                val = im[0];
                gx = (im[1] - im[-1]) * deriv_scale;
                gy = (im[W] - im[-W]) * deriv_scale;
                gs = (nx[0] - pv[0]) * deriv_scale;
                const float v2 = val * 2.f;
                dxx = (im[1] + im[-1] - v2) * second_scale;
                dyy = (im[W] + im[-W] - v2) * second_scale;
                const float dss = (nx[0] + pv[0] - v2) * second_scale;
                dxy = (im[W + 1] - im[W - 1] - im[-W + 1] + im[-W - 1]) * cross_scale;
                const float dxs = (nx[1] - nx[-1] - pv[1] + pv[-1]) * cross_scale;
                const float dys = (nx[W] - nx[-W] - pv[W] + pv[-W]) * cross_scale;
                // x_hat = -H^-1 g by Cramer's rule, H = [[dxx dxy dxs] [dxy dyy dys] [dxs dys dss]]
                const float a = dxx, b = dxy, cc = dxs, d = dyy, e = dys, f = dss;
                const float m0 = d * f - e * e, m1 = b * f - e * cc, m2 = b * e - d * cc;
                const float det = a * m0 - b * m1 + cc * m2;
                if (det == 0.f) { state = 2; break; }
                const float n0 = gx * m0 - b * (gy * f - e * gs) + cc * (gy * e - d * gs);
                const float n1 = a * (gy * f - e * gs) - gx * m1 + cc * (b * gs - gy * cc);
                const float n2 = a * (d * gs - gy * e) - b * (b * gs - gy * cc) + gx * m2;
                xc = -(n0 / det);
                xr = -(n1 / det);
                xs = -(n2 / det);
                if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xs) < 0.5f) { state = 1; break; }
                if (!(fabsf(xc) < 1e6f) || !(fabsf(xr) < 1e6f) || !(fabsf(xs) < 1e6f)) { state = 2; break; }
                c += (int)rintf(xc);
                r += (int)rintf(xr);
                l += (int)rintf(xs);
                if (l < 1 || l > 3 || c < SIFT_BORDER || c >= W - SIFT_BORDER || r < SIFT_BORDER || r >= H - SIFT_BORDER) state = 2;
            }
            if (state == 1) {
                const float t = gx * xc + gy * xr + gs * xs;
                const float contr = val * img_scale + t * 0.5f;
                const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
                if (!(fabsf(contr) * 3.f < 0.02f) && det2 > 0.f && !(tr * tr * 10.f >= 121.f * det2)) {
                    keep = true;
                    const float so = (float)(1 << o);
                    kp.code = kp_code(o, l, r, c);
                    kp.x = ((float)c + xc) * so * 0.5f;
                    kp.y = ((float)r + xr) * so * 0.5f;
                    const double sc = 1.6 * exp2(((double)l + (double)xs) / 3.0);
                    kp.size = (float)(sc * (double)(1 << o) * 2.0 * 0.5);
                    kp.scale = (float)sc;
                    kp.response = fabsf(contr);
                }
            }
        }
        const int slot = wave_append(keep, ref_count + v);
        if (keep && slot < ref_cap) ref[(long long)v * ref_cap + slot] = kp;
    }
}

// ------------------------------------------------------------------------------------------------------------------ orientations
// One 64-thread block (one wave) per keypoint: 36-bin gradient histogram on Gaussian layer `layer` of the keypoint's octave, radius
// round(4.5 s), Gaussian weight sigma 1.5 s.  Each lane accumulates its pixels into a private histogram row in LDS, the rows are summed
// in lane order: the histogram does not depend on scheduling.  Every smoothed local peak >= 0.8 max yields a keypoint in the stage list.
struct Stage {
    float* x; float* y; float* size; float* angle; float* resp;   // [V][cap] each
    int cap;
};

__global__ __launch_bounds__(64) void sift_orient_kernel(const float* __restrict__ gauss, SiftGeom g, const RefKp* __restrict__ ref, int ref_cap,
                                                         const int* __restrict__ ref_count, Stage st, int* __restrict__ stage_count) {
    __shared__ float hl[64][SIFT_HIST + 1];
    __shared__ float hraw[SIFT_HIST + 4];
    __shared__ float hs[SIFT_HIST];
    const int v = blockIdx.y, lane = threadIdx.x;
    const int nref = min(ref_count[v], ref_cap);
    for (int k = blockIdx.x; k < nref; k += gridDim.x) {
        const RefKp kp = ref[(long long)v * ref_cap + k];
        int o, l, r, c;
        kp_decode(kp.code, o, l, r, c);
        const int H = g.H[o], W = g.W[o];
        const float* im = gauss + g.g_off[o] + ((long long)v * SIFT_NG + l) * H * W;
        const int R = (int)rintf(4.5f * kp.scale);
        const float sw = 1.5f * kp.scale;
        const float escale = -1.f / (2.f * sw * sw);
        for (int b = 0; b < SIFT_HIST; ++b) hl[lane][b] = 0.f;
        const int side = 2 * R + 1, npx = side * side;
        for (int p = lane; p < npx; p += 64) {
            const int di = p / side - R, dj = p % side - R;
            const int y = r + di, x = c + dj;
            if (y <= 0 || y >= H - 1 || x <= 0 || x >= W - 1) continue;
            const float* q = im + (long long)y * W + x;
            const float dx = q[1] - q[-1], dy = q[-W] - q[W];
            const float w = expf((float)(di * di + dj * dj) * escale);
            const float mag = sqrtf(dx * dx + dy * dy);
            const float ori = atan2f(dy, dx) * (float)(180.0 / M_PI);
            int bin = (int)rintf(ori * ((float)SIFT_HIST / 360.f));
            if (bin >= SIFT_HIST) bin -= SIFT_HIST;
            if (bin < 0) bin += SIFT_HIST;
            hl[lane][bin] += w * mag;
        }
        __syncthreads();
        if (lane < SIFT_HIST) {
            float s = hl[0][lane];
            for (int q = 1; q < 64; ++q) s = s + hl[q][lane];
            hraw[lane] = s;
        }
        __syncthreads();
        if (lane < SIFT_HIST) {
            const float tm2 = hraw[(lane + SIFT_HIST - 2) % SIFT_HIST], tm1 = hraw[(lane + SIFT_HIST - 1) % SIFT_HIST];
            const float tp1 = hraw[(lane + 1) % SIFT_HIST], tp2 = hraw[(lane + 2) % SIFT_HIST];
            hs[lane] = (tm2 + tp2) * (1.f / 16.f) + (tm1 + tp1) * (4.f / 16.f) + hraw[lane] * (6.f / 16.f);
        }
        __syncthreads();
        bool peak = false;
        float angle = 0.f;
        if (lane < SIFT_HIST) {
            float mx = hs[0];
            for (int b = 1; b < SIFT_HIST; ++b) mx = fmaxf(mx, hs[b]);
            const float thr = mx * 0.8f;
            const float hl_ = hs[(lane + SIFT_HIST - 1) % SIFT_HIST], hr_ = hs[(lane + 1) % SIFT_HIST], h0 = hs[lane];
            if (h0 > hl_ && h0 > hr_ && h0 >= thr) {
                peak = true;
                float bin = (float)lane + 0.5f * (hl_ - hr_) / (hl_ - 2.f * h0 + hr_);
                bin = bin < 0.f ? (float)SIFT_HIST + bin : (bin >= (float)SIFT_HIST ? bin - (float)SIFT_HIST : bin);
                angle = 360.f - (360.f / SIFT_HIST) * bin;
                if (fabsf(angle - 360.f) < FLT_EPSILON) angle = 0.f;
            }
        }
        const int slot = wave_append(peak, stage_count + v);
        if (peak && slot < st.cap) {
            const long long j = (long long)v * st.cap + slot;
            st.x[j] = kp.x; st.y[j] = kp.y; st.size[j] = kp.size; st.angle[j] = angle; st.resp[j] = kp.response;
        }
        __syncthreads();       // hl / hraw / hs are reused by the next keypoint
    }
}

// ------------------------------------------------------------------------------------------------------------------ sort + dedup
__device__ inline bool kp_less(float* const* k, int a, int b) {
    if (k[0][a] != k[0][b]) return k[0][a] < k[0][b];      // x ascending
    if (k[1][a] != k[1][b]) return k[1][a] < k[1][b];      // y ascending
    if (k[2][a] != k[2][b]) return k[2][a] > k[2][b];      // size descending
    if (k[3][a] != k[3][b]) return k[3][a] < k[3][b];      // angle ascending
    return k[4][a] > k[4][b];                              // response descending
}

// One workgroup per view: bitonic sort of the stage list (in LDS up to SIFT_SORT_LDS entries, else in place in the global stage arrays
// through the same generic pointers), removal of exact (x, y, size, angle) duplicates, compaction into the caller's outputs.
__global__ __launch_bounds__(1024) void sift_sort_kernel(Stage st, const int* __restrict__ stage_count, const int* __restrict__ ref_count, int ref_cap,
                                                         const int* __restrict__ cand_count, long long cand_cap, int max_kp, float* __restrict__ xy,
                                                         float* __restrict__ size_out, float* __restrict__ angle_out, int* __restrict__ count,
                                                         int* __restrict__ flag) {
    extern __shared__ float lds[];
    __shared__ int scan[1024];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int n_st = stage_count[v];
    const int n = min(n_st, st.cap);
    int P = 1;
    while (P < n) P <<= 1;
    const long long gbase = (long long)v * st.cap;
    float* gk[5] = {st.x + gbase, st.y + gbase, st.size + gbase, st.angle + gbase, st.resp + gbase};
    const bool in_lds = P <= SIFT_SORT_LDS;
    float* k[5];
    for (int j = 0; j < 5; ++j) k[j] = in_lds ? lds + j * SIFT_SORT_LDS : gk[j];
    for (int i = tid; i < P; i += 1024) {
        if (i < n) {
            if (in_lds)
                for (int j = 0; j < 5; ++j) k[j][i] = gk[j][i];
        } else {
            k[0][i] = INFINITY;
            for (int j = 1; j < 5; ++j) k[j][i] = 0.f;
        }
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 1024) {
                const int ij = i ^ j;
                if (ij > i) {
                    const bool asc = (i & kk) == 0;
                    if (asc ? kp_less(k, ij, i) : kp_less(k, i, ij)) {
                        for (int q = 0; q < 5; ++q) { const float t = k[q][i]; k[q][i] = k[q][ij]; k[q][ij] = t; }
                    }
                }
            }
            __syncthreads();
        }
    }
    // dedup: thread t owns the contiguous chunk [t*chunk, (t+1)*chunk); exclusive scan of the kept counts
    const int chunk = (n + 1023) / 1024;
    const int b0 = min(n, tid * chunk), b1 = min(n, b0 + chunk);
    int kept = 0;
    for (int i = b0; i < b1; ++i)
        kept += (i == 0 || k[0][i] != k[0][i - 1] || k[1][i] != k[1][i - 1] || k[2][i] != k[2][i - 1] || k[3][i] != k[3][i - 1]) ? 1 : 0;
    scan[tid] = kept;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int out = scan[tid] - kept;
    const int total = scan[1023];
    for (int i = b0; i < b1; ++i) {
        if (i == 0 || k[0][i] != k[0][i - 1] || k[1][i] != k[1][i - 1] || k[2][i] != k[2][i - 1] || k[3][i] != k[3][i - 1]) {
            if (out < max_kp) {
                const long long o = (long long)v * max_kp + out;
                xy[2 * o] = k[0][i];
                xy[2 * o + 1] = k[1][i];
                if (size_out) size_out[o] = k[2][i];
                if (angle_out) angle_out[o] = k[3][i];
            }
            ++out;
        }
    }
    if (tid == 0) {
        count[v] = total;
        if (total > max_kp || n_st > st.cap || ref_count[v] > ref_cap || (long long)cand_count[v] > cand_cap) atomicOr(flag, 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct SiftPlan {
    SiftGeom g;
    long long cand_cap;      // per view
    int stage_cap;           // per view, power of two
    size_t off_g, off_d, off_cand, off_ref, off_stage, off_cnt, total;
};


int sift_octaves(int h, int w) {
    return (int)std::floor(std::log2((double)std::min(h, w)) - 2.0 + 0.5) + 1;
}

bool sift_plan(int V, int h, int w, int max_kp, SiftPlan& p) {
    if (V <= 0 || h < 16 || w < 16 || h > RELPOSE_SIFT_MAX_SIDE || w > RELPOSE_SIFT_MAX_SIDE || max_kp <= 0 || max_kp > (1 << 20)) return false;
    p = SiftPlan{};
    p.g.V = V;
    p.g.n_oct = sift_octaves(h, w);
    if (p.g.n_oct < 1 || p.g.n_oct > SIFT_MAX_OCT) return false;
    long long gsum = 0, dsum = 0, csum = 0;
    int H = 2 * h, W = 2 * w;
    for (int o = 0; o < p.g.n_oct; ++o) {
        p.g.H[o] = H; p.g.W[o] = W;
        p.g.g_off[o] = gsum; p.g.d_off[o] = dsum;
        gsum += (long long)V * SIFT_NG * H * W;
        dsum += (long long)V * SIFT_ND * H * W;
        csum += 3LL * std::max(H - 2 * SIFT_BORDER, 0) * std::max(W - 2 * SIFT_BORDER, 0);
        H /= 2; W /= 2;
    }
    p.cand_cap = std::max(csum, 1LL);
    int sc = 1;
    while (sc < std::max(4 * max_kp, 8192)) sc <<= 1;
    p.stage_cap = sc;
    size_t off = 0;
    p.off_g = off; off += rp_align(gsum * sizeof(float));
    p.off_d = off; off += rp_align(dsum * sizeof(float));
    p.off_cand = off; off += rp_align((size_t)V * p.cand_cap * sizeof(int));
    p.off_ref = off; off += rp_align((size_t)V * sc * sizeof(RefKp));
    p.off_stage = off; off += rp_align((size_t)5 * V * sc * sizeof(float));
    p.off_cnt = off; off += rp_align((size_t)(3 * V + 1) * sizeof(int));
    p.total = off;
    return true;
}

SiftTaps make_taps(double sigma) {
    SiftTaps t{};
    int ks = (int)std::floor(sigma * 8.0 + 1.0 + 0.5) | 1;
    t.r = ks / 2;
    double w[2 * SIFT_RMAX + 1], sum = 0.0;
    for (int i = 0; i < ks; ++i) { const double x = i - t.r; w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma)); sum += w[i]; }
    for (int i = 0; i < ks; ++i) t.t[i] = (float)(w[i] / sum);
    return t;
}

// taps[0] = the base blur sqrt(1.6^2 - (2 * 0.5)^2); taps[i] = sigma_i = 1.6 k^(i-1) sqrt(k^2 - 1), k = 2^(1/3), i = 1..5
SiftTaps g_taps[SIFT_NG];
std::once_flag g_taps_once, g_attr_once;
hipError_t g_attr_err = hipSuccess;

void init_taps() {
    const double sigma = 1.6, k = std::pow(2.0, 1.0 / 3.0);
    g_taps[0] = make_taps(std::sqrt(std::max(sigma * sigma - 1.0, 0.01)));
    for (int i = 1; i < SIFT_NG; ++i) g_taps[i] = make_taps(sigma * std::pow(k, i - 1) * std::sqrt(k * k - 1.0));
}

}  // namespace

extern "C" {

size_t relpose_sift_workspace_bytes(int32_t n_views, int32_t h, int32_t w, int32_t max_kp) {
    SiftPlan p;
    return sift_plan(n_views, h, w, max_kp, p) ? p.total : 0;
}

int32_t relpose_sift_stage_capacity(int32_t max_kp) {
    SiftPlan p;
    return sift_plan(1, 16, 16, max_kp, p) ? p.stage_cap : RELPOSE_EINVAL;
}

int relpose_sift_detect(const RelposeSiftArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeSiftArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeSiftArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeSiftArgs)));
    SiftPlan p;
    if (!a.images || !a.xy || !a.count || !a.workspace || (a.channels != 1 && a.channels != 3) || a.img_h <= 0 || a.img_w <= 0 ||
        !sift_plan(a.n_views, a.crop_h, a.crop_w, a.max_kp, p) || a.crop_x < 0 || a.crop_y < 0 || a.crop_x + a.crop_w > a.img_w ||
        a.crop_y + a.crop_h > a.img_h)
        return RELPOSE_EINVAL;
    if (a.workspace_bytes < p.total) return RELPOSE_ENOMEM;
    std::call_once(g_taps_once, init_taps);
    // the sort kernel's 80 KB of dynamic LDS is beyond the 64 KB default: set the attribute once per process, not per call
    std::call_once(g_attr_once, [] {
        g_attr_err = hipFuncSetAttribute((const void*)sift_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 5 * SIFT_SORT_LDS * (int)sizeof(float));
    });
    RP_HIP(g_attr_err);
    hipStream_t s = (hipStream_t)a.stream;
    const int V = a.n_views;
    char* ws = (char*)a.workspace;
    float* G = (float*)(ws + p.off_g);
    float* D = (float*)(ws + p.off_d);
    int* cand = (int*)(ws + p.off_cand);
    RefKp* ref = (RefKp*)(ws + p.off_ref);
    float* stg = (float*)(ws + p.off_stage);
    int* cnt = (int*)(ws + p.off_cnt);
    int *cand_count = cnt, *ref_count = cnt + V, *stage_count = cnt + 2 * V, *flag = cnt + 3 * V;
    const long long sc = p.stage_cap;
    Stage st{stg, stg + V * sc, stg + 2 * V * sc, stg + 3 * V * sc, stg + 4 * V * sc, p.stage_cap};
    RP_HIP(hipMemsetAsync(cnt, 0, (size_t)(3 * V + 1) * sizeof(int), s));

    SiftImage src{a.images, (long long)a.img_h * a.img_w * a.channels, a.img_w, a.channels, a.crop_x, a.crop_y, a.crop_w, a.crop_h};
    if (a.gray) {
        const int n = a.crop_w * a.crop_h;
        hipLaunchKernelGGL(sift_gray_kernel, dim3(std::min((n + 255) / 256, 1024), V), dim3(256), 0, s, src, a.gray);
    }
    for (int o = 0; o < p.g.n_oct; ++o) {
        const int H = p.g.H[o], W = p.g.W[o];
        const long long P = (long long)H * W, gv = SIFT_NG * P, dv = SIFT_ND * P;
        float* Go = G + p.g.g_off[o];
        float* Do = D + p.g.d_off[o];
        const dim3 tiles((W + BT_W - 1) / BT_W, (H + BT_H - 1) / BT_H, V);
        if (o == 0) {
            hipLaunchKernelGGL(sift_blur_kernel<true>, tiles, dim3(256), 0, s, (const float*)nullptr, 0LL, src, Go, gv, (float*)nullptr, 0LL, H, W,
                               g_taps[0]);
        } else {
            const int Wp = p.g.W[o - 1];
            const long long Pp = (long long)p.g.H[o - 1] * Wp;
            hipLaunchKernelGGL(sift_down_kernel, dim3(std::min((int)((P + 255) / 256), 4096), V), dim3(256), 0, s,
                               (const float*)(G + p.g.g_off[o - 1] + 3 * Pp), SIFT_NG * Pp, Wp, Go, gv, H, W);
        }
        for (int i = 1; i < SIFT_NG; ++i)
            hipLaunchKernelGGL(sift_blur_kernel<false>, tiles, dim3(256), 0, s, (const float*)(Go + (i - 1) * P), gv, src, Go + i * P, gv,
                               Do + (i - 1) * P, dv, H, W, g_taps[i]);
        const int n_in = std::max(H - 2 * SIFT_BORDER, 0) * std::max(W - 2 * SIFT_BORDER, 0);
        if (n_in > 0)
            hipLaunchKernelGGL(sift_extrema_kernel, dim3((n_in + 255) / 256, 3, V), dim3(256), 0, s, (const float*)Do, H, W, o, cand, p.cand_cap,
                               cand_count);
    }
    hipLaunchKernelGGL(sift_refine_kernel, dim3(32, V), dim3(256), 0, s, (const float*)D, p.g, (const int*)cand, p.cand_cap,
                       (const int*)cand_count, ref, p.stage_cap, ref_count);
    hipLaunchKernelGGL(sift_orient_kernel, dim3(256, V), dim3(64), 0, s, (const float*)G, p.g, (const RefKp*)ref, p.stage_cap,
                       (const int*)ref_count, st, stage_count);
    hipLaunchKernelGGL(sift_sort_kernel, dim3(V), dim3(1024), (size_t)5 * SIFT_SORT_LDS * sizeof(float), s, st, (const int*)stage_count,
                       (const int*)ref_count, p.stage_cap, (const int*)cand_count, p.cand_cap, a.max_kp, a.xy, a.size, a.angle, a.count, flag);
    RP_CHECK_LAUNCH();
    int h_flag = 0;
    RP_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    RP_HIP(hipStreamSynchronize(s));
    return h_flag ? RELPOSE_SIFT_OVERFLOW : 0;
}

}  // extern "C"
