// image_metrics.hip — PSNR and SSIM of a batch of image pairs (the rules are include/nfx.h's).
//
// FIXED OPERATION ORDER (fp64 throughout, the build has -ffp-contract=off: no fused multiply-add anywhere in this file).
//   value    a uint8 or float32 sample converted to double (exact); with `luma` and three channels the pixel's one value is
//            L = (0.2126 r + 0.7152 g) + 0.0722 b.
//   fields   per pixel, from the two values x and y: x, y, x * y, (x * x) + (y * y).
//   filter   horizontal pass h[x] = sum_k g[k] f[x + k], accumulated in ascending k starting from g[0] f[x] (acc = g[0] f[x];
//            acc = acc + g[k] f[x + k], k = 1 .. 10); vertical pass the same over the horizontally filtered rows.  This gives
//            mx, my, sxy, sxx_yy at every window position (VALID: [H - 10, W - 10]).
//   formula  m = (mx * mx) + (my * my);  p = (2 * mx) * my
//            lum = (p + c1) / (m + c1)
//            cs  = (((2 * sxy) - p) + c2) / ((sxx_yy - m) + c2)
//            v   = lum * cs
//   error    d = (x - y) / max_val;  e = d * d
//
// SUMS are integers, so they have no order: every v is added as llrint(v * 2^40) and every selected e as llrint(e * 2^40),
// first per thread, then per block into the block's own four words of the workspace (plain stores, every word written),
// then per image and channel by a second kernel that walks the blocks' words.  Nothing is zeroed beforehand and no atomic
// is used: the workspace and the totals may hold anything on entry, and the totals do not depend on the launch shape.
// A value that is not finite (an input NaN / Inf, or a product of huge floats) adds nothing and raises the image's flag;
// so does a squared error above 1, |x - y| > max_val: the images are not in the range the caller declared.
//
// One block = one TY x TX tile of window positions of one image and one channel: it loads the (TY + 10) x (TX + 10) values
// it needs into LDS as doubles, filters them horizontally into LDS, vertically out of it.  The squared error of a pixel is
// added by the block whose tile has the pixel's coordinates as a window position; the tiles of the last row / column also
// own the 10 trailing rows / columns, which they hold as halo.  LDS only, no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "image_metrics.hpp"
#include "launchers.hpp"

namespace nfx {
namespace imet {

constexpr int kThreads = 256;
constexpr int IY = kTileY + kHalo, IX = kTileX + kHalo;    // the values a tile reads
constexpr double kScale = 1099511627776.0;                 // 2^40
// What one addend may reach: a squared error 1 (|x - y| = max_val), a map value 2 (|v| <= 1 up to rounding).  With at most
// 2^22 addends per image and channel (the C-ABI refuses more) a total stays below 2^63.
constexpr double kErrLimit = kScale, kMapLimit = 2. * kScale;

struct Params {
    const void* a;
    const void* b;
    const unsigned char* mask;   // [B, H, W] or null
    double* ssim_map;            // [B, H - 10, W - 10, C'] or null
    long long* partial;          // [blocks, 4]: squared error, map, pixels counted, flag
    int H, W, C, Cp;             // Cp: channels scored (1 with luma)
    int tiles_x, tiles_y;
    double max_val, c1, c2;
    double g[kWin];
};

template <typename T>
__device__ __forceinline__ double value_at(const T* __restrict__ im, long long px, int C, int ch, bool luma) {
    if (luma) {
        const double r = (double)im[px * 3 + 0], g = (double)im[px * 3 + 1], b = (double)im[px * 3 + 2];
        return (0.2126 * r + 0.7152 * g) + 0.0722 * b;
    }
    return (double)im[px * C + ch];
}

__device__ __forceinline__ bool finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }   // false for NaN

// v * 2^40 as an integer; a value that cannot be one raises the flag and adds nothing
__device__ __forceinline__ long long fixed_point(double v, double limit, long long& flag) {
    const double s = v * kScale;
    if (!(__builtin_fabs(s) <= limit)) {
        flag = 1;
        return 0;
    }
    return __builtin_llrint(s);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tile_kernel(const Params P) {
    __shared__ double sx[IY][IX], sy[IY][IX];
    __shared__ double hf[4][IY][kTileX];
    __shared__ long long red[kThreads / 64][4];

    const int tid = threadIdx.x;
    const int img = blockIdx.z / P.Cp, ch = blockIdx.z % P.Cp;
    const int y0 = blockIdx.y * kTileY, x0 = blockIdx.x * kTileX;
    const int oh = P.H - kHalo, ow = P.W - kHalo;
    const bool luma = P.C == 3 && P.Cp == 1;
    const bool last_y = blockIdx.y == (unsigned)P.tiles_y - 1, last_x = blockIdx.x == (unsigned)P.tiles_x - 1;
    const T* __restrict__ a = (const T*)P.a;
    const T* __restrict__ b = (const T*)P.b;
    const long long img_px = (long long)img * P.H * P.W;

    long long se = 0, sm = 0, cnt = 0, flag = 0;

    // values into LDS (zero outside the image: such an entry feeds no window position of the image); the squared error
    // of the pixels this tile owns
    for (int i = tid; i < IY * IX; i += kThreads) {
        const int ly = i / IX, lx = i % IX;
        const int y = y0 + ly, x = x0 + lx;
        double vx = 0., vy = 0.;
        if (y < P.H && x < P.W) {
            const long long px = img_px + (long long)y * P.W + x;
            vx = value_at(a, px, P.C, ch, luma);
            vy = value_at(b, px, P.C, ch, luma);
            if (!finite(vx) || !finite(vy)) flag = 1;
            const bool own = (ly < kTileY || last_y) && (lx < kTileX || last_x);
            if (own && (!P.mask || P.mask[px])) {
                const double d = (vx - vy) / P.max_val;
                se += fixed_point(d * d, kErrLimit, flag);
                cnt += 1;
            }
        }
        sx[ly][lx] = vx;
        sy[ly][lx] = vy;
    }
    __syncthreads();

    // horizontal pass
    for (int i = tid; i < IY * kTileX; i += kThreads) {
        const int ly = i / kTileX, lx = i % kTileX;
        double vx = sx[ly][lx], vy = sy[ly][lx];
        double ax = P.g[0] * vx, ay = P.g[0] * vy, axy = P.g[0] * (vx * vy), aq = P.g[0] * ((vx * vx) + (vy * vy));
#pragma unroll
        for (int k = 1; k < kWin; ++k) {
            vx = sx[ly][lx + k];
            vy = sy[ly][lx + k];
            ax = ax + P.g[k] * vx;
            ay = ay + P.g[k] * vy;
            axy = axy + P.g[k] * (vx * vy);
            aq = aq + P.g[k] * ((vx * vx) + (vy * vy));
        }
        hf[0][ly][lx] = ax;
        hf[1][ly][lx] = ay;
        hf[2][ly][lx] = axy;
        hf[3][ly][lx] = aq;
    }
    __syncthreads();

    // vertical pass and the formula
    for (int i = tid; i < kTileY * kTileX; i += kThreads) {
        const int ly = i / kTileX, lx = i % kTileX;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= oh || x >= ow) continue;
        double mx = P.g[0] * hf[0][ly][lx], my = P.g[0] * hf[1][ly][lx], sxy = P.g[0] * hf[2][ly][lx], sq = P.g[0] * hf[3][ly][lx];
#pragma unroll
        for (int k = 1; k < kWin; ++k) {
            mx = mx + P.g[k] * hf[0][ly + k][lx];
            my = my + P.g[k] * hf[1][ly + k][lx];
            sxy = sxy + P.g[k] * hf[2][ly + k][lx];
            sq = sq + P.g[k] * hf[3][ly + k][lx];
        }
        const double m = (mx * mx) + (my * my);
        const double p = (2. * mx) * my;
        const double lum = (p + P.c1) / (m + P.c1);
        const double cs = (((2. * sxy) - p) + P.c2) / ((sq - m) + P.c2);
        const double v = lum * cs;
        sm += fixed_point(v, kMapLimit, flag);
        if (P.ssim_map) P.ssim_map[(((long long)img * oh + y) * ow + x) * P.Cp + ch] = v;
    }

    // the block's four integers: across the wave, then across the four waves
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        se += __shfl_down(se, off, 64);
        sm += __shfl_down(sm, off, 64);
        cnt += __shfl_down(cnt, off, 64);
        flag |= __shfl_down(flag, off, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = se;
        red[tid >> 6][1] = sm;
        red[tid >> 6][2] = cnt;
        red[tid >> 6][3] = flag;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            se += red[w][0];
            sm += red[w][1];
            cnt += red[w][2];
            flag |= red[w][3];
        }
        const long long blk = ((long long)blockIdx.z * P.tiles_y + blockIdx.y) * P.tiles_x + blockIdx.x;
        P.partial[blk * 4 + 0] = se;
        P.partial[blk * 4 + 1] = sm;
        P.partial[blk * 4 + 2] = cnt;
        P.partial[blk * 4 + 3] = flag;
    }
}

// totals[img] = {squared error per channel (3), map per channel (3), pixels counted, flag}; one block per image
__global__ __launch_bounds__(kThreads) void total_kernel(const long long* __restrict__ partial, int tiles, int Cp,
                                                         long long* __restrict__ totals) {
    __shared__ long long red[kThreads / 64][4];
    const int tid = threadIdx.x, img = blockIdx.x;
    long long cnt_all = 0, flag_all = 0;
    for (int ch = 0; ch < 3; ++ch) {
        long long se = 0, sm = 0, cnt = 0, flag = 0;
        if (ch < Cp) {
            const long long* p = partial + ((long long)img * Cp + ch) * tiles * 4;
            for (int t = tid; t < tiles; t += kThreads) {
                se += p[t * 4 + 0];
                sm += p[t * 4 + 1];
                cnt += p[t * 4 + 2];
                flag |= p[t * 4 + 3];
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            se += __shfl_down(se, off, 64);
            sm += __shfl_down(sm, off, 64);
            cnt += __shfl_down(cnt, off, 64);
            flag |= __shfl_down(flag, off, 64);
        }
        __syncthreads();      // the words of the channel before have been read
        if ((tid & 63) == 0) {
            red[tid >> 6][0] = se;
            red[tid >> 6][1] = sm;
            red[tid >> 6][2] = cnt;
            red[tid >> 6][3] = flag;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kThreads / 64; ++w) {
                se += red[w][0];
                sm += red[w][1];
                cnt += red[w][2];
                flag |= red[w][3];
            }
            totals[(long long)img * 8 + ch] = se;
            totals[(long long)img * 8 + 3 + ch] = sm;
            cnt_all += cnt;
            flag_all |= flag;
        }
    }
    if (tid == 0) {
        totals[(long long)img * 8 + 6] = cnt_all;
        totals[(long long)img * 8 + 7] = flag_all;
    }
}

}  // namespace imet
}  // namespace nfx

extern "C" int nfx_launch_image_metrics(const void* a, const void* b, int is_float, int B, int H, int W, int C, int Cp, double max_val,
                                        const unsigned char* mask, double* ssim_map, const double* host_weights, long long* totals,
                                        long long* partial, hipStream_t st) {
    using namespace nfx::imet;
    Params P;
    P.a = a;
    P.b = b;
    P.mask = mask;
    P.ssim_map = ssim_map;
    P.partial = partial;
    P.H = H;
    P.W = W;
    P.C = C;
    P.Cp = Cp;
    P.tiles_x = tiles_of(W, kTileX);
    P.tiles_y = tiles_of(H, kTileY);
    P.max_val = max_val;
    const double k1 = 0.01 * max_val, k2 = 0.03 * max_val;
    P.c1 = k1 * k1;
    P.c2 = k2 * k2;
    for (int k = 0; k < kWin; ++k) P.g[k] = host_weights[k];
    const dim3 grid(P.tiles_x, P.tiles_y, B * Cp);
    if (is_float)
        hipLaunchKernelGGL(tile_kernel<float>, grid, dim3(kThreads), 0, st, P);
    else
        hipLaunchKernelGGL(tile_kernel<unsigned char>, grid, dim3(kThreads), 0, st, P);
    hipLaunchKernelGGL(total_kernel, dim3(B), dim3(kThreads), 0, st, partial, P.tiles_x * P.tiles_y, Cp, totals);
    return (int)hipGetLastError();
}
