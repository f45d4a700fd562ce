// occgrid.hip — the occupancy grid of the density marches: which samples of a march the density
// kernel has to evaluate, and the bake of the grid from a trained network's densities.
//
// The grid: R^3 cells over the box (x_min, x_max, y_min, y_max, z_min, z_max), one bit per cell, cell (i, j, k) (i along x)
// at bit c & 31 of word c >> 5, c = (i R + j) R + k.  A point p inside the box (box_lo <= p <= box_hi on every axis) lies in
// cell floor((p - lo) / (hi - lo) * R) per axis, R - 1 on the upper face; every other point (NaN included) is outside it.
//
// Selection (nfx_occgrid_select): sample s of ray r is the point rayo[r] + rayd[r] z[r, s] (fp32, multiply then add: the
// density kernels' and torch's arithmetic).  It is listed when it lies outside the grid's box or in a cell whose bit is
// set — unless a scene bbox is given and the point is outside it (p < lo or p > hi on an axis; models/nerf.py multiplies
// the density there by 0).  The list is rowsel's (three launches, ascending, no host sync); the writing pass stores 0.0f
// at every unlisted sample's output, the density kernel's list form fills in the rest.
//
// Bake (nfx_occgrid_bake): the raw densities of a lattice of M = R P points per axis, point (a, b, c) at
// lo + (idx + 0.5) / M (hi - lo) per axis, stored at sigma[(a M + b) M + c]; cell (i, j, k) holds the P^3 lattice points
// [i P, i P + P) x ... .  A cell is occupied when one of its probes has sigma_raw > -margin (or is NaN), and its bit is set
// when an occupied cell lies within `dilate` cells of it on every axis (a (2 dilate + 1)^3 max filter).  The filter is
// separable: one pass for the occupancy of every cell (P^3 reads per cell), then one 1-D pass per axis (2 dilate + 1 bit
// reads per cell) — O(R^3 (P^3 + 6 dilate)) in all, ping-ponging between the output and a workspace of the same size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rowsel.hpp"
#include "launchers.hpp"

namespace nfx {
namespace occ {

struct Select {
    const float* rayo;
    const float* rayd;
    const float* z;
    const uint32_t* bits;
    float* out;
    int n_samples, res, has_bbox;
    float box[6], bbox[6];

    __device__ bool operator()(long long i) const {
        const long long ray = i / n_samples;
        const float zz = z[i];
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = rayo[ray * 3 + k] + rayd[ray * 3 + k] * zz;
        if (has_bbox) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (p[k] < bbox[2 * k] || p[k] > bbox[2 * k + 1]) return false;
        }
        int cell[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = box[2 * k], hi = box[2 * k + 1];
            if (!(p[k] >= lo && p[k] <= hi)) return true;
            const int c = (int)((p[k] - lo) / (hi - lo) * (float)res);
            cell[k] = c < res - 1 ? c : res - 1;
        }
        const long long c = ((long long)cell[0] * res + cell[1]) * res + cell[2];
        return (bits[c >> 5] >> (c & 31)) & 1u;
    }
    __device__ void visit(long long i, bool on) const {
        if (!on) out[i] = 0.f;
    }
};

__device__ __forceinline__ bool occupied(const float* __restrict__ sigma, int res, int probes, float margin, int i, int j,
                                         int k) {
    const long long m = (long long)res * probes;
    for (int a = 0; a < probes; ++a)
        for (int b = 0; b < probes; ++b) {
            const float* row = sigma + ((long long)(i * probes + a) * m + (j * probes + b)) * m + (long long)k * probes;
            for (int c = 0; c < probes; ++c)
                if (!(row[c] <= -margin)) return true;
        }
    return false;
}

__device__ __forceinline__ bool bit(const uint32_t* __restrict__ bits, long long c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

// one thread per 32-bit word of the grid: the occupancy of its 32 cells
__global__ __launch_bounds__(256) void occupancy_kernel(const float* __restrict__ sigma, int res, int probes, float margin,
                                                        uint32_t* __restrict__ bits) {
    const long long n_cells = (long long)res * res * res;
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w * 32 >= n_cells) return;
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const long long c = w * 32 + b;
        if (c >= n_cells) break;
        const int i = (int)(c / ((long long)res * res)), j = (int)(c / res % res), k = (int)(c % res);
        word |= (uint32_t)occupied(sigma, res, probes, margin, i, j, k) << b;
    }
    bits[w] = word;
}

// one thread per 32-bit word: dst bit c = OR of src over the cells within `dilate` of c along one axis (stride = that
// axis' step in the cell index: R^2 for x, R for y, 1 for z)
__global__ __launch_bounds__(256) void dilate_kernel(const uint32_t* __restrict__ src, int res, int dilate, long long stride,
                                                     uint32_t* __restrict__ dst) {
    const long long n_cells = (long long)res * res * res;
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w * 32 >= n_cells) return;
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const long long c = w * 32 + b;
        if (c >= n_cells) break;
        const int pos = (int)(c / stride % res);
        const int lo = pos - dilate > 0 ? pos - dilate : 0, hi = pos + dilate < res - 1 ? pos + dilate : res - 1;
        bool on = false;
        for (int q = lo; q <= hi && !on; ++q) on = bit(src, c + (long long)(q - pos) * stride);
        word |= (uint32_t)on << b;
    }
    dst[w] = word;
}

}  // namespace occ
}  // namespace nfx

extern "C" size_t nfx_occgrid_list_bytes(long long n_pts) { return nfx::rowsel::workspace_bytes(n_pts); }

extern "C" int nfx_launch_occgrid_select(const float* rayo, const float* rayd, const float* z, long long n_rays,
                                         int n_samples, const uint32_t* bits, int res, const float* box, const float* bbox,
                                         float* out, void* ws, hipStream_t st) {
    nfx::occ::Select s{rayo, rayd, z, bits, out, n_samples, res, bbox != nullptr, {}, {}};
    for (int k = 0; k < 6; ++k) {
        s.box[k] = box[k];
        s.bbox[k] = bbox ? bbox[k] : 0.f;
    }
    return nfx::rowsel::build(s, n_rays * n_samples, ws, st);
}

// occupancy -> bits (dilate = 0), or occupancy -> ws, x: ws -> bits, y: bits -> ws, z: ws -> bits
extern "C" int nfx_launch_occgrid_bake(const float* sigma, int res, int probes, float margin, int dilate, uint32_t* bits,
                                       uint32_t* ws, hipStream_t st) {
    using namespace nfx::occ;
    const long long n_words = ((long long)res * res * res + 31) / 32;
    const dim3 grid((unsigned)((n_words + 255) / 256));
    hipLaunchKernelGGL(occupancy_kernel, grid, dim3(256), 0, st, sigma, res, probes, margin, dilate ? ws : bits);
    if (dilate) {
        const long long r = res;
        hipLaunchKernelGGL(dilate_kernel, grid, dim3(256), 0, st, (const uint32_t*)ws, res, dilate, r * r, bits);
        hipLaunchKernelGGL(dilate_kernel, grid, dim3(256), 0, st, (const uint32_t*)bits, res, dilate, r, ws);
        hipLaunchKernelGGL(dilate_kernel, grid, dim3(256), 0, st, (const uint32_t*)ws, res, dilate, 1ll, bits);
    }
    return (int)hipGetLastError();
}
