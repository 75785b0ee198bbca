// Skybox panoramas from posed perspective RGB-D frames: every frame pixel with data is unprojected (util.depth2pc's 480x640 branch), moved
// by its frame's pose, projected into the four-face panorama by reproj_helper's rule (skybox.h's rp_skybox_project, shared with visibility.hip), and the
// points that fall on one panorama pixel are fused by a foreground-gated mean.  The contract -- the float64 geometry, the gate, the integer
// accumulators, the resolve -- is DESIGN.md §4.13 and the comment above relpose_frames_to_pano in include/relpose.h;
// tests/panorama_model.py restates it in numpy.  Built with -ffp-contract=off.  Every accumulator is an integer, so the result does not
// depend on the order in which points arrive, nor on which of the two paths below a point took.
//
//   pano_splat_kernel<1>   zmin: per panorama pixel the smallest face depth d over all frames of the view.  d > 0, and positive floats
//                          order like their bit patterns: an unsigned atomic min.
//   pano_splat_kernel<2>   accumulate: a point with d <= zmin + zmin * gate adds 1 to count, llrint(d 65536) to sum_z and its three
//                          colour bytes to sum_rgb.
//   pano_resolve_kernel    one thread per panorama pixel: depth, rgb, valid from the sums; copies the stage buffers out.
//
// A 480x640 frame puts ~50 points on each panorama pixel: one global atomic per point would queue every adder on a few rows.  So a
// 256-thread workgroup owns a 16x16 tile of one frame (four tile rows per wave: depth is read in 64-byte row segments) and aggregates in
// LDS first: a table of kSlots entries keyed by panorama pixel, open addressing with at most kProbes probes, LDS integer atomics on the
// entry's accumulators.  A point that finds no entry within kProbes probes goes to the global atomics directly.  After the barrier every
// occupied entry does one global atomic per accumulator: a dozen or so per workgroup instead of 256 or more.  The rgb bytes of a tile that
// lies inside the frame's columns are fetched as 12 dwords per row into LDS when the rows start on dword boundaries, else byte by byte.
// The frame's scale and pose are read at wave-uniform addresses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "skybox.h"

namespace {

constexpr int kTile = 16, kThreads = kTile * kTile;
constexpr int kSlots = 64;            // LDS table entries: an aligned 480x640 tile touches ~3x3 panorama pixels, a seam or a steep pose a few more
constexpr int kProbes = 8;            // bounded probing: beyond it the point takes the global path
constexpr int kRowDwords = kTile * 3 / 4;
constexpr unsigned kEmptyZ = 0xffffffffu;
constexpr float kMaxDepth = 32768.0f; // llrint(d 65536) < 2^31

struct PanoBufs {
    int n, F, Hf, Wf, h, dataset;
    int by0, by1, bx0, bx1;           // the box; the whole map when there is none
    float gate;
    int rgb_dwords;                   // every frame row of rgb starts on a dword boundary
    const float* depth;               // [n, F, Hf, Wf]
    const uint8_t* rgb;               // [n, F, Hf, Wf, 3]
    const double* scale;              // [n, F, 2]
    const double* pose;               // [n, F, 4, 4] or NULL
    unsigned* zmin;                   // [n, h, 4h]   workspace
    unsigned* count;                  // [n, h, 4h]
    unsigned long long* sum_z;        // [n, h, 4h]
    unsigned* sum_rgb;                // [n, 3, h, 4h]
};

// Frame pixel (r, c) with depth zf -> panorama pixel (row * 4h + column) and face depth d, or -1 when the point is dropped.
// sc = (sx, sy), T = the frame's 4x4 pose or NULL.
__device__ __forceinline__ int pano_point(const PanoBufs& a, const double* sc, const double* T, int r, int c, float zf, float& d) {
    if (!(zf > 0.0f) || !(zf <= FLT_MAX)) return -1;             // 0, negative, NaN, inf: no data
    const double z = (double)zf;
    const double xs = ((double)c / a.Wf - 0.5) * 2, ys = (0.5 - (double)r / a.Hf) * 2;
    const double X = (xs * z) / sc[0], Y = (ys * z) / sc[1], Z = -z;
    double q0 = X, q1 = Y, q2 = Z;
    if (T) {                                                     // np.matmul(R44, [p; 1])[:3], left to right like warp_point
        q0 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3] * 1.0;
        q1 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7] * 1.0;
        q2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11] * 1.0;
    }
    // the first slot whose test passes (skybox.h); the box, the depth cap and the -2 code are this kernel's own
    int slot, cx, cy;
    double zz;
    if (!rp_skybox_project(a.dataset, a.h, q0, q1, q2, slot, cx, cy, zz)) return -1;
    const int px = slot * a.h + cx, py = cy;
    d = (float)(-zz);
    const bool keep = py >= a.by0 && py < a.by1 && px >= a.bx0 && px < a.bx1 && d < kMaxDepth;
    return keep ? py * 4 * a.h + px : -2;                        // -2: found its face and is dropped
}

// Claims the table entry of `key`: its index, or -1 when kProbes probes found only other keys.
__device__ __forceinline__ int pano_claim(int* skey, int key) {
    const unsigned h0 = ((unsigned)key * 0x9E3779B1u) >> 26;     // kSlots = 2^6
    int slot = -1;
    for (int i = 0; i < kProbes && slot < 0; ++i) {
        const int s = (int)((h0 + (unsigned)i) & (kSlots - 1));
        const int prev = atomicCAS(&skey[s], -1, key);
        if (prev == -1 || prev == key) slot = s;
    }
    return slot;
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void pano_splat_kernel(PanoBufs a) {
    __shared__ int skey[kSlots];
    __shared__ unsigned sval[kSlots];                            // pass 1: min of the depth bits; pass 2: count
    __shared__ unsigned long long ssum[PASS == 2 ? kSlots : 1];
    __shared__ unsigned scol[PASS == 2 ? 3 * kSlots : 1];
    __shared__ unsigned srgb[PASS == 2 ? kTile * kRowDwords : 1];

    const int tid = threadIdx.x, tx = tid & (kTile - 1), ty = tid >> 4;
    const int vf = blockIdx.z, v = vf / a.F;
    const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
    const int c = c0 + tx, r = r0 + ty;
    const bool in = c < a.Wf && r < a.Hf;
    const size_t fpix = ((size_t)vf * a.Hf + (in ? r : 0)) * a.Wf + (in ? c : 0);
    const size_t hw = (size_t)a.h * 4 * a.h;

    if (tid < kSlots) {
        skey[tid] = -1;
        sval[tid] = PASS == 1 ? kEmptyZ : 0u;
        if (PASS == 2) { ssum[tid] = 0ull; scol[tid] = 0u; scol[kSlots + tid] = 0u; scol[2 * kSlots + tid] = 0u; }
    }
    const bool tile_dwords = PASS == 2 && a.rgb_dwords && c0 + kTile <= a.Wf;
    if (PASS == 2 && tile_dwords && tid < kTile * kRowDwords) {
        const int ry = tid / kRowDwords, j = tid - ry * kRowDwords;
        if (r0 + ry < a.Hf) {
            const size_t b = (((size_t)vf * a.Hf + r0 + ry) * a.Wf + c0) * 3;   // a multiple of 4: rows are dword-aligned, c0 * 3 = 48 k
            srgb[tid] = *(RP_GLOBAL const unsigned*)(a.rgb + b + 4 * (size_t)j);
        }
    }
    const float zf = in ? rp_ldg(a.depth + fpix) : 0.0f;
    float d = 0.0f;
    int pix = pano_point(a, a.scale + (size_t)vf * 2, a.pose ? a.pose + (size_t)vf * 16 : nullptr, r, c, zf, d);
    unsigned cr = 0, cg = 0, cb = 0;
    if (PASS == 2 && pix >= 0) {
        const float zm = __uint_as_float(a.zmin[(size_t)v * hw + pix]);
        if (!(d <= zm + zm * a.gate)) pix = -2;                  // behind the foreground
    }
    __syncthreads();

    if (pix >= 0) {
        if (PASS == 2) {
            if (tile_dwords) {
                const uint8_t* sb = (const uint8_t*)srgb + ty * (kRowDwords * 4) + tx * 3;
                cr = sb[0]; cg = sb[1]; cb = sb[2];
            } else {
                const uint8_t* gb = a.rgb + fpix * 3;
                cr = gb[0]; cg = gb[1]; cb = gb[2];
            }
        }
        const int slot = pano_claim(skey, pix);
        const size_t gp = (size_t)v * hw + pix;
        if (PASS == 1) {
            const unsigned bits = __float_as_uint(d);
            if (slot >= 0) atomicMin(&sval[slot], bits);
            else atomicMin(&a.zmin[gp], bits);
        } else {
            const unsigned long long q = (unsigned long long)llrint((double)d * 65536.0);
            unsigned* gc = a.sum_rgb + (size_t)v * 3 * hw + pix;
            if (slot >= 0) {
                atomicAdd(&sval[slot], 1u);
                atomicAdd(&ssum[slot], q);
                atomicAdd(&scol[slot], cr); atomicAdd(&scol[kSlots + slot], cg); atomicAdd(&scol[2 * kSlots + slot], cb);
            } else {
                atomicAdd(&a.count[gp], 1u);
                atomicAdd(&a.sum_z[gp], q);
                atomicAdd(gc, cr); atomicAdd(gc + hw, cg); atomicAdd(gc + 2 * hw, cb);
            }
        }
    }
    __syncthreads();

    if (tid < kSlots && skey[tid] >= 0) {
        const int key = skey[tid];
        const size_t gp = (size_t)v * hw + key;
        if (PASS == 1) {
            if (sval[tid] != kEmptyZ) atomicMin(&a.zmin[gp], sval[tid]);
        } else {
            unsigned* gc = a.sum_rgb + (size_t)v * 3 * hw + key;
            atomicAdd(&a.count[gp], sval[tid]);
            atomicAdd(&a.sum_z[gp], ssum[tid]);
            atomicAdd(gc, scol[tid]); atomicAdd(gc + hw, scol[kSlots + tid]); atomicAdd(gc + 2 * hw, scol[2 * kSlots + tid]);
        }
    }
}

struct PanoOut {
    float* depth;                     // [n, h, 4h]
    float* rgb;                       // [n, 3, h, 4h]
    uint8_t* valid;                   // [n, h, 4h]
    unsigned* zmin; unsigned* count; unsigned long long* sum_z; unsigned* sum_rgb;   // stage copies or NULL
};

__global__ __launch_bounds__(256) void pano_resolve_kernel(PanoBufs a, PanoOut o) {
    const size_t hw = (size_t)a.h * 4 * a.h, total = (size_t)a.n * hw;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t v = i / hw, p = i - v * hw;
    const unsigned cnt = a.count[i];
    const unsigned long long sz = a.sum_z[i];
    const unsigned* sc = a.sum_rgb + v * 3 * hw + p;
    const unsigned s0 = sc[0], s1 = sc[hw], s2 = sc[2 * hw];
    float dep = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (cnt > 0) {
        dep = (float)((double)sz / (double)cnt / 65536.0);
        const unsigned long long k = cnt, k2 = 2ull * cnt;
        c0 = (float)(unsigned)((2ull * s0 + k) / k2) / 255.0f;
        c1 = (float)(unsigned)((2ull * s1 + k) / k2) / 255.0f;
        c2 = (float)(unsigned)((2ull * s2 + k) / k2) / 255.0f;
    }
    rp_stg(o.depth + i, dep);
    float* oc = o.rgb + v * 3 * hw + p;
    rp_stg(oc, c0); rp_stg(oc + hw, c1); rp_stg(oc + 2 * hw, c2);
    o.valid[i] = cnt > 0 ? 1 : 0;
    if (o.zmin) o.zmin[i] = cnt > 0 ? a.zmin[i] : 0u;
    if (o.count) o.count[i] = cnt;
    if (o.sum_z) o.sum_z[i] = sz;
    if (o.sum_rgb) { unsigned* os = o.sum_rgb + v * 3 * hw + p; os[0] = s0; os[hw] = s1; os[2 * hw] = s2; }
}

// workspace: sum_z [n hw] u64 | zmin [n hw] u32 | count [n hw] u32 | sum_rgb [n 3 hw] u32
constexpr size_t kBytesPerPixel = 8 + 4 + 4 + 12;

bool pano_dims_ok(int64_t n, int64_t h) { return n >= 1 && n <= 65535 && h >= 2 && h <= 8192 && (h & 1) == 0; }

}  // namespace

extern "C" size_t relpose_frames_to_pano_workspace_bytes(int32_t n, int32_t h) {
    if (!pano_dims_ok(n, h)) return 0;
    return rp_align((size_t)n * h * 4 * h * kBytesPerPixel);
}

extern "C" int relpose_frames_to_pano(const RelposeFramesToPanoArgs* args_in) {
    if (!args_in || args_in->struct_size < offsetof(RelposeFramesToPanoArgs, stream) + sizeof(void*)) return RELPOSE_EINVAL;
    RelposeFramesToPanoArgs a{};
    memcpy(&a, args_in, std::min((size_t)args_in->struct_size, sizeof(RelposeFramesToPanoArgs)));
    if (!pano_dims_ok(a.n_views, a.h) || a.n_frames < 1 || a.frame_h < 0 || a.frame_w < 0) return RELPOSE_EINVAL;
    const uint64_t per_view = (uint64_t)a.n_frames * (uint64_t)a.frame_h * (uint64_t)a.frame_w;
    // sum_rgb is u32: 255 * count must fit; the frames of a view ride on blockIdx.z
    if (per_view > (1ull << 24) || (uint64_t)a.n_views * a.n_frames > 65535 || a.frame_h > 16 * 65535) return RELPOSE_EINVAL;
    const bool empty = per_view == 0;
    // a launch holds fewer than 2^32 threads: the splat passes one per frame pixel of whole 16x16 tiles, the resolve one per panorama pixel
    const uint64_t tiles = (uint64_t)((a.frame_w + kTile - 1) / kTile) * (uint64_t)((a.frame_h + kTile - 1) / kTile);
    if (tiles * kThreads * (uint64_t)a.n_views * (uint64_t)a.n_frames >= (1ull << 32)) return RELPOSE_EINVAL;
    if ((uint64_t)a.n_views * a.h * 4 * a.h + 255 >= (1ull << 32)) return RELPOSE_EINVAL;
    if (!a.out_depth || !a.out_rgb || !a.out_valid || !a.workspace || (uintptr_t)a.workspace % 8 != 0) return RELPOSE_EINVAL;
    if (!empty && (!a.depth || !a.rgb || !a.scale)) return RELPOSE_EINVAL;
    if (!(a.gate >= 0.0f) || !std::isfinite(a.gate)) return RELPOSE_EINVAL;
    if (a.dataset != RELPOSE_SUNCG && a.dataset != RELPOSE_MATTERPORT && a.dataset != RELPOSE_SCANNET) return RELPOSE_EINVAL;
    if (a.workspace_bytes < relpose_frames_to_pano_workspace_bytes(a.n_views, a.h)) return RELPOSE_EINVAL;
    PanoBufs k{};
    k.n = a.n_views; k.F = a.n_frames; k.Hf = a.frame_h; k.Wf = a.frame_w; k.h = a.h; k.dataset = a.dataset; k.gate = a.gate;
    if (a.box[0] == -1 && a.box[1] == -1 && a.box[2] == -1 && a.box[3] == -1) { k.by0 = 0; k.by1 = a.h; k.bx0 = 0; k.bx1 = 4 * a.h; }
    else {
        k.by0 = a.box[0]; k.by1 = a.box[1]; k.bx0 = a.box[2]; k.bx1 = a.box[3];
        if (k.by0 < 0 || k.by1 > a.h || k.by0 > k.by1 || k.bx0 < 0 || k.bx1 > 4 * a.h || k.bx0 > k.bx1) return RELPOSE_EINVAL;
    }
    k.depth = a.depth; k.rgb = a.rgb; k.scale = a.scale; k.pose = a.pose;
    k.rgb_dwords = ((uintptr_t)a.rgb % 4 == 0 && ((size_t)a.frame_w * 3) % 4 == 0) ? 1 : 0;
    const size_t npix = (size_t)a.n_views * a.h * 4 * a.h;
    uint8_t* ws = (uint8_t*)a.workspace;
    k.sum_z = (unsigned long long*)ws;
    k.zmin = (unsigned*)(ws + npix * 8);
    k.count = k.zmin + npix;
    k.sum_rgb = k.count + npix;
    PanoOut o{a.out_depth, a.out_rgb, a.out_valid, a.zmin, a.count, (unsigned long long*)a.sum_z, a.sum_rgb};
    hipStream_t s = (hipStream_t)a.stream;
    RP_HIP(hipMemsetAsync(ws, 0, npix * kBytesPerPixel, s));
    RP_HIP(hipMemsetAsync(k.zmin, 0xff, npix * 4, s));
    if (!empty) {
        const dim3 grid((a.frame_w + kTile - 1) / kTile, (a.frame_h + kTile - 1) / kTile, a.n_views * a.n_frames);
        hipLaunchKernelGGL(pano_splat_kernel<1>, grid, dim3(kThreads), 0, s, k);
        hipLaunchKernelGGL(pano_splat_kernel<2>, grid, dim3(kThreads), 0, s, k);
    }
    hipLaunchKernelGGL(pano_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, k, o);
    RP_CHECK_LAUNCH();
    return 0;
}
