// The naive form of relpose_mesh_components' triangle statistics, for tools/components_time.py only (not part of the library): one integer
// atomicAdd per triangle and sum, straight into comp_triangles / comp_area, where csrc/meshcc.hip first sums the runs of equal labels in the
// wave and the workgroup's own component in LDS.  Same terms, same results; built with -ffp-contract=off like the library.
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void naive_stats_kernel(const int* tri, const int* tri_label, const double* points, int cap, int cap_tri, int cap_comp,
                                                          double scale, int* comp_triangles, unsigned long long* comp_area) {
    const unsigned nblk = (cap_tri + 255) / 256, s = blockIdx.x / nblk, t = (blockIdx.x - s * nblk) * 256 + threadIdx.x;
    if (t >= (unsigned)cap_tri) return;
    const int c = tri_label[(size_t)s * cap_tri + t];
    if (c < 0 || c >= cap_comp) return;                                          // a labelled row is a good row: its indices are inside [0, cap)
    const int* r = tri + ((size_t)s * cap_tri + t) * 3;
    const double* p = points + (size_t)s * cap * 3;
    const double* p0 = p + (size_t)r[0] * 3;
    const double* p1 = p + (size_t)r[1] * 3;
    const double* p2 = p + (size_t)r[2] * 3;
    const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, w[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double cx = u[1] * w[2] - u[2] * w[1], cy = u[2] * w[0] - u[0] * w[2], cz = u[0] * w[1] - u[1] * w[0];
    const double q = sqrt((cx * cx + cy * cy) + cz * cz) * 0.5 * scale;
    const long long a = isfinite(q) ? llrint(fmin(q, 2147483648.0)) : 0;
    atomicAdd(comp_triangles + (size_t)s * cap_comp + c, 1);
    atomicAdd(comp_area + (size_t)s * cap_comp + c, (unsigned long long)a);
}

extern "C" int components_naive_stats(const int* tri, const int* tri_label, const double* points, int n_scenes, int cap, int cap_tri, int cap_comp,
                                      double scale, int* comp_triangles, int64_t* comp_area, void* stream) {
    if (n_scenes < 1 || cap < 1 || cap_tri < 1 || cap_comp < 1) return -1;
    const unsigned nblk = (cap_tri + 255) / 256;
    hipLaunchKernelGGL(naive_stats_kernel, dim3((unsigned)n_scenes * nblk), dim3(256), 0, (hipStream_t)stream, tri, tri_label, points, cap, cap_tri,
                       cap_comp, scale, comp_triangles, (unsigned long long*)comp_area);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
