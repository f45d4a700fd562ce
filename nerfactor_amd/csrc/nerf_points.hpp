// nerf_points.hpp — the points of one density launch (nerf_geom.hip, nerf_geom_x3.hip, nerf_sigma_x3_pipe.hip), for the host
// that fills it in (capi_geom.cpp) and the kernels that walk it: which flat sample of z[n_rays, n_samples] is point m of
// the launch, where is it in space, and where does its density go.  Three forms:
//   EVERY SAMPLE  (list null, last_sample 0): point m is flat sample m, n_pts = n_rays n_samples; density to out[m].
//   LIST          (list, count in device memory): the points are the flat samples list[0 .. *count) — the number of selected
//                 samples never visits the host; n_pts is the list's capacity and only sizes the grid, a workgroup without a
//                 tile leaves before it touches the weight stream.  The density of sample s goes to out[list_stride (s + 1) - 1]:
//                 list_stride = 4 is the sigma channel of rgbs[N, S, 4] (the selective coarse refinement of the bf16 render,
//                 nfx_nerf_sigma_refine), 1 a flat [N, S] (nfx_nerf_sigma_fwd_list, the occupancy-grid march).  The gradient
//                 kernels (nfx_nerf_sigma_grad_rows: the samples with a positive density) write (normal, sigma) of sample s to
//                 row s of out[N S][4].
//   LAST SAMPLE   (last_sample 1, density only): n_pts = n_rays, point m is the last sample of ray m, flat (m + 1) S - 1, and
//                 is stored like a listed one (nfx_nerf_sigma_refine_last).
#pragma once
#include <hip/hip_runtime.h>

namespace nfx {
namespace geo {

struct Points {
    const float* rayo;    // [n_rays, 3]
    const float* rayd;    // [n_rays, 3]
    const float* z;       // [n_rays, n_samples]
    long long n_pts;
    int n_samples;
    const int* list;
    const int* count;
    int list_stride;
    int last_sample;

    // n: the points of the launch, as the device counts them; false: this workgroup of tile_rows points per tile has none
    __device__ __forceinline__ bool counted(int tile_rows, long long& n) const {
        n = n_pts;
        if (list != nullptr) {
            n = *count;
            if ((long long)blockIdx.x * tile_rows >= n) return false;
        }
        return true;
    }
    // position m of a launch of n_pts points -> flat sample (a lane past the end repeats the last point)
    __device__ __forceinline__ long long sample(long long m, long long n_pts) const {
        long long mm = m < n_pts ? m : n_pts - 1;
        if (list != nullptr) mm = list[mm];
        else if (last_sample) mm = (mm + 1) * n_samples - 1;
        return mm;
    }
    __device__ __forceinline__ void position(long long mm, float (&x)[3]) const {
        const long long ray = mm / n_samples;
        const float zz = z[mm];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = rayo[ray * 3 + k] + rayd[ray * 3 + k] * zz;
    }
    // the density of point m = flat sample mm to its place
    __device__ __forceinline__ void store_sigma(float* out, long long m, long long mm, float sigma) const {
        if (list != nullptr || last_sample) out[list_stride * (mm + 1) - 1] = sigma;
        else out[m] = sigma;
    }
    // ... and its (normal, sigma) row
    __device__ __forceinline__ long long grad_row(long long m, long long mm) const { return list != nullptr ? mm : m; }
};

}  // namespace geo
}  // namespace nfx
