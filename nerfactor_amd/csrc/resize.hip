// resize.hip — antialiased bilinear resize of channels-last images (include/nfx.h: nfx_resize_antialias).
//
// One workgroup owns a tile of ty x tx output pixels and a chunk of cc channels.  The taps of its rows and columns span a
// rectangle of the input, its footprint: the workgroup copies it to LDS in the input's own type (16-byte global loads
// where a run of the contiguous (x, channel) axis is aligned, single elements at its ends), runs the horizontal pass from
// there into a float32 LDS image of footprint rows x tx columns, and the vertical pass from that image to the output
// (four consecutive values of the (x, channel) axis per thread: one 16-byte store for float32, one 4-byte store for uint8,
// single elements where the run or the alignment ends).  The value between the passes never leaves LDS.  One thread
// computes one output value in ascending tap order, so the tile shape has no part in the result.
//
// The tables are device arrays that the host cannot read: a tile clamps every index it takes from them to its footprint,
// so that tables that are not the ones of nfx_resize_axis_table give wrong pictures, not accesses out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"
#include "resize.hpp"

namespace nfx {
namespace rsz {

struct Params {
    const void* in;
    void* out;
    const int *first_y, *count_y, *first_x, *count_x;
    const float *wy, *wx;
    int h, w, c, oh, ow, taps_y, taps_x;
    float in_scale;
    int tiles_x;
    Plan plan;
};

__device__ __forceinline__ float to_float(unsigned char v, float s) { return (float)v * s; }
__device__ __forceinline__ float to_float(unsigned short v, float s) { return (float)v * s; }
__device__ __forceinline__ float to_float(float v, float) { return v; }

__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(unsigned char* p, float v) { *p = (unsigned char)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

__device__ __forceinline__ void put4(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void put4(unsigned char* p, const float* v) {
    uchar4 q;
    put(&q.x, v[0]);
    put(&q.y, v[1]);
    put(&q.z, v[2]);
    put(&q.w, v[3]);
    *(uchar4*)p = q;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One axis of a tile: outputs o0 .. o0 + n - 1.  Returns the footprint [*lo, *lo + *len) inside [0, n_in), at most cap
// long; meta[3 i ..] = first tap of output i relative to *lo, and the range [k0, k1) of its taps that lie in the footprint
// (all of them for the tables of nfx_resize_axis_table); ws[i taps + k] = its weights.
__device__ void stage_axis(const int* first, const int* count, const float* weights, int taps, int o0, int n, int n_in, int cap,
                           int* meta, float* ws, int* lo, int* len) {
    const int f0 = clampi(first[o0], 0, n_in - 1);
    const int last = o0 + n - 1;
    const int end = clampi(clampi(first[last], 0, n_in - 1) + clampi(count[last], 0, taps), f0 + 1, n_in);
    const int span = end - f0 < cap ? end - f0 : cap;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int f = clampi(first[o0 + i], 0, n_in - 1), cnt = clampi(count[o0 + i], 0, taps);
        const int rel = f - f0;
        meta[3 * i] = rel;
        meta[3 * i + 1] = rel < 0 ? (-rel < cnt ? -rel : cnt) : 0;
        meta[3 * i + 2] = rel + cnt > span ? (span - rel > 0 ? span - rel : 0) : cnt;
    }
    for (int i = threadIdx.x; i < n * taps; i += kThreads) ws[i] = weights[(long long)o0 * taps + i];
    *lo = f0;
    *len = span;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kThreads) void resize_kernel(const Params P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Plan& pl = P.plan;
    float* mid = (float*)lds;
    float* wys = (float*)(lds + pl.off_wy);
    float* wxs = (float*)(lds + pl.off_wx);
    int* meta_y = (int*)(lds + pl.off_meta);
    int* meta_x = meta_y + 3 * pl.ty;
    Tin* ins = (Tin*)(lds + pl.off_in);

    const int tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x % P.tiles_x;
    const int oy0 = tile_y * pl.ty, ox0 = tile_x * pl.tx;
    const int tyn = P.oh - oy0 < pl.ty ? P.oh - oy0 : pl.ty, txn = P.ow - ox0 < pl.tx ? P.ow - ox0 : pl.tx;
    const int c0 = blockIdx.y * pl.cc;
    const int ccn = P.c - c0 < pl.cc ? P.c - c0 : pl.cc;
    const long long b = blockIdx.z;
    const int tid = threadIdx.x;

    int r0, nr, q0, nq;
    stage_axis(P.first_y, P.count_y, P.wy, P.taps_y, oy0, tyn, P.h, pl.fr_cap, meta_y, wys, &r0, &nr);
    stage_axis(P.first_x, P.count_x, P.wx, P.taps_x, ox0, txn, P.w, pl.fc_cap, meta_x, wxs, &q0, &nq);

    // ---- the footprint: nr rows of nq pixels of ccn channels.  A run is what is contiguous in memory: a whole row of the
    // footprint when the chunk is every channel, one pixel's ccn channels otherwise.
    {
        constexpr int V = 16 / (int)sizeof(Tin);
        const Tin* in = (const Tin*)P.in;
        const bool whole = ccn == P.c;
        const int runs_per_row = whole ? 1 : nq, run_len = whole ? nq * ccn : ccn;
        const int units = run_len / V + 2;                       // 16-byte pieces of a run, a partial one at either end
        const int items = nr * runs_per_row * units;
        for (int it = tid; it < items; it += kThreads) {
            const int u = it % units, run = it / units;
            const int px = run % runs_per_row, r = run / runs_per_row;
            const Tin* g = in + ((b * P.h + (r0 + r)) * P.w + (q0 + px)) * P.c + c0;
            Tin* s = ins + r * pl.in_pitch + px * ccn;
            const int mis = (int)(((uintptr_t)g / sizeof(Tin)) % V);
            const int e0 = u * V - mis;
            if (e0 >= 0 && e0 + V <= run_len) {
                const uint4 q = *(const uint4*)(g + e0);
                const Tin* qe = (const Tin*)&q;
#pragma unroll
                for (int e = 0; e < V; ++e) s[e0 + e] = qe[e];
            } else {
                const int lo = e0 > 0 ? e0 : 0, hi = e0 + V < run_len ? e0 + V : run_len;
                for (int e = lo; e < hi; ++e) s[e] = g[e];
            }
        }
    }
    __syncthreads();

    // ---- horizontal pass: mid[r, i, ch] for every footprint row
    {
        const int items = nr * txn * ccn;
        for (int it = tid; it < items; it += kThreads) {
            const int ch = it % ccn, t2 = it / ccn;
            const int i = t2 % txn, r = t2 / txn;
            const int rel = meta_x[3 * i], k0 = meta_x[3 * i + 1], k1 = meta_x[3 * i + 2];
            const Tin* s = ins + r * pl.in_pitch + rel * ccn + ch;
            const float* wk = wxs + i * P.taps_x;
            float t = 0.f;
            for (int k = k0; k < k1; ++k) t = t + wk[k] * to_float(s[k * ccn], P.in_scale);
            mid[r * pl.mid_pitch + i * ccn + ch] = t;
        }
    }
    __syncthreads();

    // ---- vertical pass: four consecutive values of the tile row's (x, channel) axis per thread
    {
        Tout* out = (Tout*)P.out;
        const int len = txn * ccn, groups = (len + 3) / 4;
        const bool whole = ccn == P.c;
        const int items = tyn * groups;
        for (int it = tid; it < items; it += kThreads) {
            const int j0 = (it % groups) * 4, j = it / groups;
            const int rel = meta_y[3 * j], k0 = meta_y[3 * j + 1], k1 = meta_y[3 * j + 2];
            const float* wk = wys + j * P.taps_y;
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = k0; k < k1; ++k) {
                const float wgt = wk[k];
                const float4 m = *(const float4*)(mid + (rel + k) * pl.mid_pitch + j0);     // the pitch is a multiple of 4
                t[0] = t[0] + wgt * m.x;
                t[1] = t[1] + wgt * m.y;
                t[2] = t[2] + wgt * m.z;
                t[3] = t[3] + wgt * m.w;
            }
            Tout* row = out + ((b * P.oh + (oy0 + j)) * P.ow + ox0) * P.c + c0;
            // element jj of the tile row: pixel jj / ccn, channel jj % ccn
            const int px0 = whole ? 0 : j0 / ccn, ch0 = whole ? j0 : j0 % ccn;
            Tout* p = row + (long long)px0 * P.c + ch0;
            const bool together = j0 + 4 <= len && (whole || ch0 + 4 <= ccn);
            if (together && ((uintptr_t)p & (4 * sizeof(Tout) - 1)) == 0) {
                put4(p, t);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e < len) {
                        const int jj = j0 + e;
                        put(whole ? row + jj : row + (long long)(jj / ccn) * P.c + jj % ccn, t[e]);
                    }
            }
        }
    }
}

template <typename Tin>
static void launch_out(const Params& P, int out_uint8, dim3 grid, hipStream_t st) {
    if (out_uint8)
        hipLaunchKernelGGL((resize_kernel<Tin, unsigned char>), grid, dim3(kThreads), P.plan.lds_bytes, st, P);
    else
        hipLaunchKernelGGL((resize_kernel<Tin, float>), grid, dim3(kThreads), P.plan.lds_bytes, st, P);
}

}  // namespace rsz
}  // namespace nfx

extern "C" int nfx_launch_resize_antialias(const void* in, int in_type, int batch, int h, int w, int c, float in_scale, const int* first_y,
                                           const int* count_y, const float* weights_y, int taps_y, const int* first_x,
                                           const int* count_x, const float* weights_x, int taps_x, void* out, int out_uint8, int oh,
                                           int ow, hipStream_t st) {
    using namespace nfx::rsz;
    Params P;
    P.in = in;
    P.out = out;
    P.first_y = first_y;
    P.count_y = count_y;
    P.first_x = first_x;
    P.count_x = count_x;
    P.wy = weights_y;
    P.wx = weights_x;
    P.h = h;
    P.w = w;
    P.c = c;
    P.oh = oh;
    P.ow = ow;
    P.taps_y = taps_y;
    P.taps_x = taps_x;
    P.in_scale = in_scale;
    P.plan = plan(in_type, h, w, c, oh, ow, taps_y, taps_x);
    P.tiles_x = (int)P.plan.tiles_x;
    const dim3 grid((unsigned)(P.plan.tiles_y * P.plan.tiles_x), (unsigned)P.plan.chunks, (unsigned)batch);
    if (in_type == NFX_RESIZE_U8)
        launch_out<unsigned char>(P, out_uint8, grid, st);
    else if (in_type == NFX_RESIZE_U16)
        launch_out<unsigned short>(P, out_uint8, grid, st);
    else
        launch_out<float>(P, out_uint8, grid, st);
    return (int)hipGetLastError();
}
