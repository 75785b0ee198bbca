// The four-face skybox panorama shared by geometry.hip, panorama.hip, visibility.hip and tsdf.hip: the face rotations and reproj_helper's rule for
// the panorama pixel of a point.  Device-only and force-inlined; the including files are built with -ffp-contract=off.
#pragma once
#include "common.h"

// Face rotations Rs[k] of the skybox (util.py:757-761).  Entries are 0 / +-1, so applying them is an exact permutation / sign flip.
// rp_face_rot = Rs[k] v, rp_face_rot_t = Rs[k]^T v.
__device__ __forceinline__ void rp_face_rot(int k, double x, double y, double z, double& ox, double& oy, double& oz) {
    switch (k & 3) {
        case 0: ox = x; oy = y; oz = z; break;
        case 1: ox = -z; oy = y; oz = x; break;
        case 2: ox = -x; oy = y; oz = -z; break;
        default: ox = z; oy = y; oz = -x; break;
    }
}
__device__ __forceinline__ void rp_face_rot_t(int k, double x, double y, double z, double& ox, double& oy, double& oz) {
    switch (k & 3) {
        case 0: ox = x; oy = y; oz = z; break;
        case 1: ox = z; oy = y; oz = -x; break;
        case 2: ox = -x; oy = y; oz = -z; break;
        default: ox = -z; oy = y; oz = x; break;
    }
}
// the rotation of panorama slot `slot` (the h columns from slot h)
__device__ __forceinline__ int rp_face_index(int dataset, int slot) { return dataset == RELPOSE_SUNCG ? slot : (slot + 3) & 3; }

// The panorama pixel of the point q: the first slot whose face takes it (the strict tests make the faces disjoint), the pixel (cx, cy) inside
// that face -- round half to even, clamped to [0, h - 1] -- and zz < 0, the point's coordinate along the face's axis (face depth = -zz).
// False when no face takes the point; the outputs are then unset.  |x| >= az implies |x / az| >= 1 after rounding too, so the divisions
// are only made where the test can still pass.
__device__ __forceinline__ bool rp_skybox_project(int dataset, int h, double q0, double q1, double q2, int& slot, int& cx, int& cy, double& zz) {
    bool found = false;
#pragma unroll 1
    for (int s = 0; s < 4 && !found; ++s) {
        double x, y, z;
        rp_face_rot_t(rp_face_index(dataset, s), q0, q1, q2, x, y, z);
        const double az = fabs(z) + 1e-32;
        if (z < 0 && fabs(x) < az && fabs(y) < az) {
            const double xn = x / az, yn = y / az;
            if (fabs(xn) < 1 && fabs(yn) < 1) {
                double fx = rint((xn + 1) * 0.5 * h), fy = rint((1 - yn) * 0.5 * h);      // round half to even
                fx = fx < 0 ? 0 : (fx > h - 1 ? h - 1 : fx);
                fy = fy < 0 ? 0 : (fy > h - 1 ? h - 1 : fy);
                slot = s; cx = (int)fx; cy = (int)fy; zz = z;
                found = true;
            }
        }
    }
    return found;
}
