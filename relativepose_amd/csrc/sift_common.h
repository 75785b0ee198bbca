// The uint8 source image of the SIFT detector (sift.hip) and of the SIFT descriptors (siftdesc.hip): the crop, its gray value and the
// blurs' border rule.  The two blur kernels stay in their files: the detector's has a run-time radius, the descriptors' a compile-time one.
#pragma once
#include "common.h"

struct SiftImage {
    const uint8_t* img;
    long long vstride;   // bytes per view
    int img_w, channels, cx, cy, w, h;   // the crop: w x h pixels from (cx, cy)
};

// cv2.BORDER_REFLECT_101: index i of an axis of n pixels
__device__ inline int sift_refl101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// cv2.COLOR_BGR2GRAY on uint8: 14-bit fixed-point weights B 1868, G 9617, R 4899 (rputil.bgr2gray)
__device__ inline int sift_gray_at(const SiftImage& s, const uint8_t* im, int y, int x) {
    const uint8_t* p = im + ((long long)(s.cy + y) * s.img_w + (s.cx + x)) * s.channels;
    if (s.channels == 1) return p[0];
    return ((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + (1 << 13)) >> 14;
}
