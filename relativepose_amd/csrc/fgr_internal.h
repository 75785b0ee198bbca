// The front end shared by relpose_fgr (fgr.hip) and relpose_ransac (ransac.hip): stages 1-4 of DESIGN.md §4.6 (voxels, neighbour
// lists, normals, FPFH) and the exact fp32 feature nearest neighbour, and the draw generator both contracts name.  (The device helpers the
// two share with the other point-cloud kernels -- dot, distance, scans, sort, reductions -- are in cloud_prims.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct FgrBufs {
    int n_clouds, P, cap;
    const double* pc;
    const uint8_t* valid;
    long long* key[2];       // [2B, P] ping-pong
    int* idx[2];
    double* pts;             // [2B, cap, 3]
    int* ix;                 // [2B, cap]
    int* count;              // [2B] true voxel count
    int* nbr;                // [2B, cap, 100]
    double* nd2;             // [2B, cap, 100]
    int* ncnt;               // [2B, cap]
    double* normal;          // [2B, cap, 3]
    double* spfh;            // [2B, cap, 33]
    double* fpfh;            // [2B, cap, 33]
    float* f32;              // [2B, cap, 33]
    int* nn;                 // [2B, cap]
    int* corr;               // [B, cap, 2]
    int* ncorr;              // [B]
    int* tcorr;              // [B, 3000, 2]
    int* ntup;               // [B]
    double* pose;            // [B, 4, 4]
    int* status;             // [B]
    unsigned long long seed;
};

// Enqueue the six front-end launches on s: voxel downsample, neighbours, normals, SPFH, FPFH, and the fp32 feature nearest neighbour of
// every voxel of cloud c among the voxels of cloud c ^ 1 (ties to the lower index) into f.nn.  Reads pc / valid, writes key .. nn.
__attribute__((visibility("hidden"))) void fgr_front_end(const FgrBufs& f, hipStream_t s);

__device__ __forceinline__ unsigned long long fgr_splitmix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
