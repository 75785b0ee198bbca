// The descriptor distance of DESIGN.md §4.9, shared by descriptor.hip (the rank threshold) and completion.hip (the contrastive loss):
// fp32, accumulated from 0 with c ascending as acc = acc + d * d.  Both sources are built with -ffp-contract=off, so it is never fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// a[c * sa], b[c * sb]: channel c of the two descriptors (feature maps keep their channels one map apart)
__device__ __forceinline__ float rp_desc_dist2(const float* a, size_t sa, const float* b, size_t sb, int C) {
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float d = a[c * sa] - b[c * sb];
        acc = acc + d * d;
    }
    return acc;
}
