// Descriptor evaluation for a batch of panorama pairs: the dense ground-truth correspondences of the reference's loaders
// (datasets/SUNCG.py:315-341) and the rank counts behind its feature-quality metric (evalDLDescriptor,
// mainPanoCompletion2view.py:383-414, with the observed / unobserved classes of :535-542).  The contract -- transform order,
// tie rule, the fixed fp32 expression -- is DESIGN.md §4.9; tests/descriptor_model.py restates it in numpy.  Built with
// -ffp-contract=off: the model and these kernels round alike.
//
// Clouds / images: 2b = the source of pair b, 2b + 1 its target.
//   dense_nn_kernel     one block per 256 queries of a pair, one query per thread: the target cloud streams through LDS in tiles of 1024
//                       points, transformed on load, and is scanned in ascending index with a strict `<` (lowest index wins a tie; no
//                       cross-block reduction, so the result cannot depend on scheduling)
//   rank_prep_kernel    one thread per slot: the threshold in the fixed expression, the class, and the counter's start value (0 or -1)
//   rank_count_kernel   one block per tile of target pixels and pair: threads keep their pixels' features in registers (two pixels per
//                       packed fp32 lane pair), the slots' source features sit in LDS and are read as same-address broadcasts; per slot a
//                       wave ballot + popcount, then one integer atomic add per slot and block (integer adds: the sum is order-free)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "desc_dist.h"

namespace {

constexpr double kDefaultMaxDist = 0.08;        // datasets/SUNCG.py:328
constexpr int kNnThreads = 256;
constexpr int kNnTile = 1024;

struct NnBufs {
    int B, P, nq, h;
    double max_dist;
    const double* pc;        // [2B, 3, P]
    const uint8_t* valid;    // [2B, P]
    const double* to_world;  // [2B, 4, 4]
    const int* query;        // [B, nq]
    int* nn_index;
    double* nn_dist;
    uint8_t* hit;
    int* idx_src;            // [B, nq, 2]
    int* idx_tgt;
};

// w_a = ((M_a0 x + M_a1 y) + M_a2 z) + M_a3
__device__ __forceinline__ void to_world3(const double* M, double x, double y, double z, double w[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = ((M[4 * a] * x + M[4 * a + 1] * y) + M[4 * a + 2] * z) + M[4 * a + 3];
}

// the reference's PanoIdx (datasets/SUNCG.py:164-174): face-major point index -> (x, y) panorama pixel
__device__ __forceinline__ void pano_idx(int i, int h, int& x, int& y) {
    const int face = i / (h * h), r = i - face * h * h;
    y = r / h;
    x = (r - y * h) + face * h;
}

__global__ __launch_bounds__(kNnThreads) void dense_nn_kernel(NnBufs a) {
    __shared__ double tx[kNnTile], ty[kNnTile], tz[kNnTile];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int q = blockIdx.x * kNnThreads + tid;
    const size_t P = (size_t)a.P;
    const double* ps = a.pc + (size_t)(2 * b) * 3 * P;
    const double* pt = a.pc + (size_t)(2 * b + 1) * 3 * P;
    const uint8_t* vt = a.valid + (size_t)(2 * b + 1) * P;
    double Mt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Mt[k] = a.to_world[(size_t)(2 * b + 1) * 16 + k];
    int qi = -1;
    if (q < a.nq) {
        qi = a.query[(size_t)b * a.nq + q];
        if (qi < 0 || qi >= a.P || !a.valid[(size_t)(2 * b) * P + qi]) qi = -1;
    }
    double w[3] = {0.0, 0.0, 0.0};
    if (qi >= 0) {
        double Ms[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Ms[k] = a.to_world[(size_t)(2 * b) * 16 + k];
        to_world3(Ms, ps[qi], ps[P + qi], ps[2 * P + qi], w);
    }
    double best = INFINITY;
    int bi = -1;
    for (int t0 = 0; t0 < a.P; t0 += kNnTile) {
        const int nt = min(kNnTile, a.P - t0);
        __syncthreads();                            // the previous tile has been read by every thread
        for (int e = tid; e < nt; e += kNnThreads) {
            const int i = t0 + e;
            double p[3];
            to_world3(Mt, pt[i], pt[P + i], pt[2 * P + i], p);
            // an invalid point can never win: NaN compares false under `<`
            tx[e] = vt[i] ? p[0] : NAN;
            ty[e] = p[1];
            tz[e] = p[2];
        }
        __syncthreads();
        for (int e = 0; e < nt; ++e) {
            const double dx = tx[e] - w[0], dy = ty[e] - w[1], dz = tz[e] - w[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) { best = d2; bi = t0 + e; }
        }
    }
    if (q >= a.nq) return;
    const size_t o = (size_t)b * a.nq + q;
    const bool found = qi >= 0 && bi >= 0;
    const double dist = found ? sqrt(best) : -1.0;
    a.nn_index[o] = found ? bi : -1;
    a.nn_dist[o] = dist;
    a.hit[o] = (found && dist < a.max_dist) ? 1 : 0;
    int xs = 0, ys = 0, xt = 0, yt = 0;
    if (found) {
        pano_idx(qi, a.h, xs, ys);
        pano_idx(bi, a.h, xt, yt);
    }
    a.idx_src[2 * o] = xs; a.idx_src[2 * o + 1] = ys;
    a.idx_tgt[2 * o] = xt; a.idx_tgt[2 * o + 1] = yt;
}

// ------------------------------------------------------------------------------------------------------------- rank counts
struct RankBufs {
    int B, Ct, off, C, h, K, E;
    const float* f;          // [2B, Ct, h, 4h]
    const int* idx_src;      // [B, K, 2] (x, y)
    const int* idx_tgt;
    const int* sel;          // [B, E] or NULL (slot e = correspondence e)
    const uint8_t* pair_valid;   // [B] or NULL (all valid)
    const float* mask;       // [2B, h, 4h] or NULL
    int* count;              // [B, E]
    float* thr;              // [B, E]
    int* type;               // [B, E]
};

// The source / target pixel offsets (y * 4h + x) of slot (b, e), or false for an unused slot, an invalid pair or pixels outside the map.
__device__ __forceinline__ bool rank_slot(const RankBufs& r, int b, int e, int& ps, int& pt) {
    if (r.pair_valid && !r.pair_valid[b]) return false;
    const int k = r.sel ? r.sel[(size_t)b * r.E + e] : e;
    if (k < 0 || k >= r.K) return false;
    const int* s = r.idx_src + ((size_t)b * r.K + k) * 2;
    const int* t = r.idx_tgt + ((size_t)b * r.K + k) * 2;
    const int w = 4 * r.h;
    if (s[0] < 0 || s[0] >= w || s[1] < 0 || s[1] >= r.h || t[0] < 0 || t[0] >= w || t[1] < 0 || t[1] >= r.h) return false;
    ps = s[1] * w + s[0];
    pt = t[1] * w + t[0];
    return true;
}

__global__ __launch_bounds__(256) void rank_prep_kernel(RankBufs r) {
    const int b = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= r.E) return;
    const size_t o = (size_t)b * r.E + e;
    int ps, pt;
    if (!rank_slot(r, b, e, ps, pt)) {
        r.count[o] = -1;
        r.thr[o] = 0.0f;
        r.type[o] = -1;
        return;
    }
    const size_t HW = (size_t)r.h * 4 * r.h;
    const float* fs = r.f + ((size_t)(2 * b) * r.Ct + r.off) * HW + ps;
    const float* ft = r.f + ((size_t)(2 * b + 1) * r.Ct + r.off) * HW + pt;
    r.count[o] = 0;
    r.thr[o] = rp_desc_dist2(fs, HW, ft, HW, r.C);
    r.type[o] = r.mask ? (int)(r.mask[(size_t)(2 * b) * HW + ps] != 0.0f) + (int)(r.mask[(size_t)(2 * b + 1) * HW + pt] != 0.0f) : -1;
}

constexpr int kRankThreads = 256;
constexpr int kRankChunk = 128;          // slots whose source features sit in LDS at a time

// CT: channels kept per pixel (C rounded up; the padding channels are 0 on both sides and add +0 to the sum: bitwise neutral).
// NP: packed pixel pairs per thread.  A block covers kRankThreads * 2 * NP consecutive pixels of one target map.
template <int CT, int NP>
__global__ __launch_bounds__(kRankThreads) void rank_count_kernel(RankBufs r) {
    __shared__ __attribute__((aligned(16))) float qf[kRankChunk * CT];
    __shared__ float qthr[kRankChunk];
    __shared__ int qpix[kRankChunk];
    __shared__ int wcnt[kRankThreads / 64][kRankChunk];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (r.pair_valid && !r.pair_valid[b]) return;          // uniform over the block: before any barrier
    const int HW = r.h * 4 * r.h;
    const float* fs = r.f + ((size_t)(2 * b) * r.Ct + r.off) * HW;
    const float* ft = r.f + ((size_t)(2 * b + 1) * r.Ct + r.off) * HW;
    rp_v2f tf[NP][CT];
    bool live[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = (blockIdx.x * NP + j) * (kRankThreads * 2) + 2 * tid;       // HW and p are even: a pair is inside or outside the map as one
        live[j] = p < HW;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            rp_v2f v = {0.0f, 0.0f};
            if (live[j] && c < r.C) v = *(RP_GLOBAL const rp_v2f*)(ft + (size_t)c * HW + p);
            tf[j][c] = v;
        }
    }
    for (int e0 = 0; e0 < r.E; e0 += kRankChunk) {
        const int ne = min(kRankChunk, r.E - e0);
        __syncthreads();                                    // the previous chunk's features and counters have been consumed
        if (tid < kRankChunk) {
            int ps = -1, pt;
            if (tid < ne && !rank_slot(r, b, e0 + tid, ps, pt)) ps = -1;
            qpix[tid] = ps;
            // an unused slot counts nothing: no distance is below -inf
            qthr[tid] = ps >= 0 ? r.thr[(size_t)b * r.E + e0 + tid] : -INFINITY;
        }
        __syncthreads();
        for (int i = tid; i < kRankChunk * CT; i += kRankThreads) {
            const int q = i / CT, c = i - q * CT;
            const int ps = qpix[q];
            qf[i] = (ps >= 0 && c < r.C) ? fs[(size_t)c * HW + ps] : 0.0f;
        }
        __syncthreads();
        for (int q = 0; q < ne; ++q) {
            const float t = qthr[q];
            const rp_v4f* row = (const rp_v4f*)(qf + q * CT);
            rp_v2f acc[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) acc[j] = rp_v2f{0.0f, 0.0f};
#pragma unroll
            for (int c4 = 0; c4 < CT / 4; ++c4) {
                const rp_v4f s = row[c4];                   // same address in every lane: an LDS broadcast
                const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const rp_v2f s2 = {sv[k], sv[k]};
#pragma unroll
                    for (int j = 0; j < NP; ++j) {
                        const rp_v2f d = s2 - tf[j][4 * c4 + k];
                        acc[j] = acc[j] + d * d;
                    }
                }
            }
            int n = 0;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                n += __popcll(__ballot(live[j] && acc[j].x < t));
                n += __popcll(__ballot(live[j] && acc[j].y < t));
            }
            if (lane == 0) wcnt[wave][q] = n;
        }
        __syncthreads();
        if (tid < ne && qpix[tid] >= 0) {
            int n = 0;
#pragma unroll
            for (int w = 0; w < kRankThreads / 64; ++w) n += wcnt[w][tid];
            if (n) atomicAdd(r.count + (size_t)b * r.E + e0 + tid, n);
        }
    }
}

template <int CT, int NP>
void launch_rank(const RankBufs& r, hipStream_t s) {
    const int HW = r.h * 4 * r.h, per = kRankThreads * 2 * NP;
    hipLaunchKernelGGL((rank_count_kernel<CT, NP>), dim3((HW + per - 1) / per, r.B), dim3(kRankThreads), 0, s, r);
}

}  // namespace

extern "C" {

int relpose_dense_nn(const RelposeDenseNnArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeDenseNnArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeDenseNnArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeDenseNnArgs)));
    if (!a.pc || !a.valid || !a.to_world || !a.query || !a.nn_index || !a.nn_dist || !a.hit || !a.idx_src || !a.idx_tgt) return RELPOSE_EINVAL;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.n_points < 1 || a.n_query < 1 || a.h < 1 || a.h > 8192) return RELPOSE_EINVAL;
    if ((long long)4 * a.h * a.h != (long long)a.n_points || !(a.max_dist >= 0.0)) return RELPOSE_EINVAL;
    NnBufs n{};
    n.B = a.n_pairs; n.P = a.n_points; n.nq = a.n_query; n.h = a.h;
    n.max_dist = a.max_dist == 0.0 ? kDefaultMaxDist : a.max_dist;
    n.pc = a.pc; n.valid = a.valid; n.to_world = a.to_world; n.query = a.query;
    n.nn_index = a.nn_index; n.nn_dist = a.nn_dist; n.hit = a.hit; n.idx_src = a.idx_src; n.idx_tgt = a.idx_tgt;
    hipLaunchKernelGGL(dense_nn_kernel, dim3((a.n_query + kNnThreads - 1) / kNnThreads, a.n_pairs), dim3(kNnThreads), 0, (hipStream_t)a.stream, n);
    RP_CHECK_LAUNCH();
    return 0;
}

int relpose_descriptor_rank(const RelposeDescRankArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeDescRankArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeDescRankArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeDescRankArgs)));
    if (!a.f || ((uintptr_t)a.f & 7) || !a.idx_src || !a.idx_tgt || !a.count || !a.thr || !a.type) return RELPOSE_EINVAL;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.h < 1 || a.h > 8192 || a.n_channels < 1 || a.n_channels > RELPOSE_DESC_MAX_CHANNELS) return RELPOSE_EINVAL;
    if (a.feat_off < 0 || a.total_channels < a.feat_off + a.n_channels || a.n_corres < 1) return RELPOSE_EINVAL;
    const int E = a.sel ? a.n_slots : a.n_corres;
    if (E < 1) return RELPOSE_EINVAL;
    RankBufs r{};
    r.B = a.n_pairs; r.Ct = a.total_channels; r.off = a.feat_off; r.C = a.n_channels; r.h = a.h; r.K = a.n_corres; r.E = E;
    r.f = a.f; r.idx_src = a.idx_src; r.idx_tgt = a.idx_tgt; r.sel = a.sel; r.pair_valid = a.pair_valid; r.mask = a.mask;
    r.count = a.count; r.thr = a.thr; r.type = a.type;
    hipStream_t s = (hipStream_t)a.stream;
    hipLaunchKernelGGL(rank_prep_kernel, dim3((E + 255) / 256, r.B), dim3(256), 0, s, r);
    RP_CHECK_LAUNCH();
    if (r.C <= 8) launch_rank<8, 2>(r, s);
    else if (r.C <= 16) launch_rank<16, 2>(r, s);
    else if (r.C <= 32) launch_rank<32, 2>(r, s);
    else launch_rank<64, 1>(r, s);
    RP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
