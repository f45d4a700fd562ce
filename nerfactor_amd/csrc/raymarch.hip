// raymarch.hip — the non-MLP stages of vanilla-NeRF ray marching (all HBM-bound, fp32):
//   l2_normalize3   tf.linalg.l2_normalize                        nerf.py:157, util/math.py:63-64
//   gen_z           Model.gen_z                                   nerf.py:120-136
//   composite       Model.accumulate_sigma + Model._accumulate    nerf.py:184-254, util/math.py:67-68,
//                                                                 util/img.py:76-95
//   sample_fine     inv_transform_sample + Model.gen_z_fine       util/math.py:71-94, nerf.py:138-147
// One wave (64 lanes) per ray for composite / sample_fine: the samples of a ray sit on the lanes,
// loads are one contiguous 256-B / 1-KiB segment per wave, scans and reductions are wave shuffles.
#include "nfx_common.hpp"
#include "launchers.hpp"

namespace nfx {

__global__ void l2_normalize3_kernel(const float* __restrict__ in, float* __restrict__ out,
                                     long long n, float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    const float sq = x * x + y * y + z * z;
    const float inv = 1.0f / sqrtf(fmaxf(sq, eps));
    out[3 * i] = x * inv;
    out[3 * i + 1] = y * inv;
    out[3 * i + 2] = z * inv;
}

// tf.linspace(0,1,n)[i] = i * (1/(n-1)) in fp32 (TF 2.2 LinSpace CPU kernel: start + step*i).
__device__ __forceinline__ float linspace01(int i, int n) { return (float)i * (1.0f / (float)(n - 1)); }

__device__ __forceinline__ float z_of_t(float t, float near, float far, int lin_in_disp) {
    if (lin_in_disp) return 1.0f / (1.0f / near * (1.0f - t) + 1.0f / far * t);
    return near * (1.0f - t) + far * t;
}

__global__ void gen_z_kernel(float near, float far, int n_samples, long long n_rays,
                             int lin_in_disp, const float* __restrict__ u, float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays * n_samples) return;
    const int s = (int)(i % n_samples);
    const float zc = z_of_t(linspace01(s, n_samples), near, far, lin_in_disp);
    if (u == nullptr) {
        z[i] = zc;
        return;
    }
    // nerf.py:130-135: jitter inside [lower, upper] = midpoints to the neighbours
    const float zl = s > 0 ? z_of_t(linspace01(s - 1, n_samples), near, far, lin_in_disp) : zc;
    const float zu = s < n_samples - 1 ? z_of_t(linspace01(s + 1, n_samples), near, far, lin_in_disp) : zc;
    const float lower = s > 0 ? 0.5f * (zc + zl) : zc;
    const float upper = s < n_samples - 1 ? 0.5f * (zu + zc) : zc;
    z[i] = lower + (upper - lower) * u[i];
}

// ---------------------------------------------------------------------------------------
// composite: block = 256 threads = 4 rays (one wave each).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void composite_kernel(
    const float4* __restrict__ rgbs, const float* __restrict__ z, const float* __restrict__ rayd,
    const float* __restrict__ noise, long long n_rays, int S, float bg, float* __restrict__ rgb_out,
    float* __restrict__ occu_out, float* __restrict__ depth_out, float* __restrict__ disp_out,
    float* __restrict__ w_out) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;  // wave-uniform
    const float dx = rayd[3 * ray], dy = rayd[3 * ray + 1], dz = rayd[3 * ray + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);  // nerf.py:192-193
    const long long base = ray * S;
    float carry = 1.0f;  // running exclusive product of (1 - alpha + 1e-6)
    float s_w = 0.f, s_r = 0.f, s_g = 0.f, s_b = 0.f, s_d = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const int sc = valid ? s : S - 1;
        const float4 raw = rgbs[base + sc];
        const float zc = z[base + sc];
        const float zn = (sc < S - 1) ? z[base + sc + 1] : 0.f;
        float dist = (sc < S - 1) ? (zn - zc) : 1e10f;  // nerf.py:188-191
        dist = dist * dnorm;
        float sg = raw.w;
        if (noise) sg = sg + noise[base + sc];
        const float alpha = 1.0f - expf(-fmaxf(sg, 0.0f) * dist);  // nerf.py:199-200
        float t = valid ? (1.0f - alpha + 1e-6f) : 1.0f;            // util/math.py:67-68
        // inclusive product scan across the wave
        float incl = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl *= up;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float w = valid ? alpha * (carry * excl) : 0.0f;
        carry = carry * __shfl(incl, 63, 64);
        if (w_out && valid) w_out[base + s] = w;
        s_w += w;
        s_r += w * sigmoidf(raw.x);  // nerf.py:223,234-235
        s_g += w * sigmoidf(raw.y);
        s_b += w * sigmoidf(raw.z);
        s_d += w * zc;               // nerf.py:237-238
    }
    s_w = wave_sum(s_w);
    s_r = wave_sum(s_r);
    s_g = wave_sum(s_g);
    s_b = wave_sum(s_b);
    s_d = wave_sum(s_d);
    if (lane == 0) {
        if (rgb_out) {  // nerf.py:252-253 + util/img.py:95: rgb*occu + bg*(1-occu)
            const float k = 1.0f - s_w;
            rgb_out[3 * ray] = s_r * s_w + bg * k;
            rgb_out[3 * ray + 1] = s_g * s_w + bg * k;
            rgb_out[3 * ray + 2] = s_b * s_w + bg * k;
        }
        if (occu_out) occu_out[ray] = s_w;
        if (depth_out) depth_out[ray] = s_d;
        if (disp_out) disp_out[ray] = 1.0f / fmaxf(s_d, 1e-10f);  // nerf.py:240-241
    }
}

// ---------------------------------------------------------------------------------------
// surface: the fine pass of the geometry march up to what datasets/nerf_shape.py reads of a test view (alpha, xyz).
// composite_kernel's scan on the densities alone (sigma[n, S], no rgb), reduced to occupancy and expected depth in
// registers — the [n, S] weights are never stored — then process_view's epilogue (geometry_from_nerf.py):
//   occu < occu_thres -> 0;  alpha = clamp(occu, 0, 1);  xyz = (o + d depth) alpha + 0  (_alpha_blend, bg = None);
//   quantize: alpha_out = floor(255 alpha + 0.5) / 255, what alpha.png read back by load_rgba gives (xyz keeps the
//   unquantised alpha, as xyz.npy does).  block = 256 threads = 4 rays (one wave each); S any >= 1.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surface_kernel(
    const float* __restrict__ sigma, const float* __restrict__ z, const float* __restrict__ rayo,
    const float* __restrict__ rayd, long long n_rays, int S, float occu_thres, int quantize,
    float* __restrict__ alpha_out, float* __restrict__ xyz_out, float* __restrict__ depth_out,
    float* __restrict__ occu_out) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;  // wave-uniform
    const float dx = rayd[3 * ray], dy = rayd[3 * ray + 1], dz = rayd[3 * ray + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const long long base = ray * S;
    float carry = 1.0f;
    float s_w = 0.f, s_d = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const int sc = valid ? s : S - 1;
        const float zc = z[base + sc];
        const float zn = (sc < S - 1) ? z[base + sc + 1] : 0.f;
        float dist = (sc < S - 1) ? (zn - zc) : 1e10f;
        dist = dist * dnorm;
        const float alpha = 1.0f - expf(-fmaxf(sigma[base + sc], 0.0f) * dist);
        const float t = valid ? (1.0f - alpha + 1e-6f) : 1.0f;
        float incl = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl *= up;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float w = valid ? alpha * (carry * excl) : 0.0f;
        carry = carry * __shfl(incl, 63, 64);
        s_w += w;
        s_d += w * zc;
    }
    s_w = wave_sum(s_w);
    s_d = wave_sum(s_d);
    if (lane == 0) {
        const float occu = s_w < occu_thres ? 0.0f : s_w;
        const float a = fminf(fmaxf(occu, 0.0f), 1.0f);
        xyz_out[3 * ray] = (rayo[3 * ray] + dx * s_d) * a + 0.0f;
        xyz_out[3 * ray + 1] = (rayo[3 * ray + 1] + dy * s_d) * a + 0.0f;
        xyz_out[3 * ray + 2] = (rayo[3 * ray + 2] + dz * s_d) * a + 0.0f;
        alpha_out[ray] = quantize ? floorf(a * 255.0f + 0.5f) / 255.0f : a;
        depth_out[ray] = s_d;
        if (occu_out) occu_out[ray] = s_w;
    }
}

// ---------------------------------------------------------------------------------------
// refine_select: which COARSE samples decide where the inverse-CDF sampler puts the fine samples (round 6).  One wave
// per ray, the same scan as composite_kernel (alpha_i, exclusive transmittance T_i).  A sample is listed when it is
// VISIBLE (T_i > t_min) and either NOT SATURATED (a_lo < alpha_i < a_hi) — a density error there moves the weights of the
// ray — or UNDECIDED (|sigma_i| < sigma_margin: the bf16 kernel cannot tell which side of the relu the sample is on; on a
// near-miss ray, whose weights sum to almost nothing, one such sample IS the pdf of the inverse-CDF sampler),
// or is the neighbour (`dilate` samples either way) of such a sample: at a density edge the bf16 kernel may say
// sigma < 0 (alpha = 0 exactly) where the fp32 value is positive.  The last sample (dist = 1e10) is never listed: the
// render re-evaluates it anyway (nfx_nerf_sigma_fwd on z[:, -1]).  list[] receives the flat sample indices ray * S + s
// in arbitrary order (one atomicAdd per wave), *count their number.
// ---------------------------------------------------------------------------------------
constexpr int kSelRays = 8;        // rays per wave and workgroup pass: 32 rays share ONE atomicAdd on the list's length
__global__ __launch_bounds__(256) void refine_select_kernel(
    const float4* __restrict__ rgbs, const float* __restrict__ z, const float* __restrict__ rayd, long long n_rays, int S,
    float t_min, float a_lo, float a_hi, float sigma_margin, int dilate, int* __restrict__ list, int* __restrict__ count) {
    // One atomicAdd per wave and ray (the first form of this kernel) serialises on the one counter: 280 000 of them on a fitted
    // 800 x 800 view = 2.9 of the kernel's 3.3 ms.  Now a workgroup marks 4 x kSelRays rays, parks their masks in LDS, reserves
    // its slice of the list with ONE atomic and writes it.
    constexpr int kMaxChunks = 8;                     // S <= 512 (checked by nfx_nerf_refine_select)
    __shared__ unsigned long long s_mask[4 * kSelRays][kMaxChunks];
    __shared__ int s_cnt[4 * kSelRays];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_chunks = (S + 63) / 64;
    for (int r = 0; r < kSelRays; ++r) {
        const int slot = wave * kSelRays + r;
        const long long ray = ((long long)blockIdx.x * 4 + wave) * kSelRays + r;
        int total = 0;
        if (ray < n_rays) {   // wave-uniform
            const float dx = rayd[3 * ray], dy = rayd[3 * ray + 1], dz = rayd[3 * ray + 2];
            const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
            const long long base = ray * S;
            float carry = 1.0f;
            unsigned long long bits[kMaxChunks + 2];      // bits[c + 1] = marks of chunk c; zero guards at both ends
#pragma unroll
            for (int c = 0; c < kMaxChunks + 2; ++c) bits[c] = 0ull;
            for (int c = 0; c < n_chunks; ++c) {
                const int s = c * 64 + lane;
                const bool valid = s < S;
                const int sc = valid ? s : S - 1;
                const float sg = rgbs[base + sc].w;
                const float zc = z[base + sc];
                const float zn = (sc < S - 1) ? z[base + sc + 1] : 0.f;
                const float dist = ((sc < S - 1) ? (zn - zc) : 1e10f) * dnorm;
                const float alpha = 1.0f - expf(-fmaxf(sg, 0.0f) * dist);
                const float t = valid ? (1.0f - alpha + 1e-6f) : 1.0f;
                float incl = t;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl *= up;
                }
                float excl = __shfl_up(incl, 1, 64);
                if (lane == 0) excl = 1.0f;
                const float T = carry * excl;
                carry = carry * __shfl(incl, 63, 64);
                const bool m = valid && T > t_min && ((alpha > a_lo && alpha < a_hi) || fabsf(sg) < sigma_margin);
                const unsigned long long b = __ballot(m);
#pragma unroll
                for (int k = 0; k < kMaxChunks; ++k)
                    if (k == c) bits[k + 1] = b;
            }
            for (int c = 0; c < n_chunks; ++c) {
                unsigned long long own = 0ull, before = 0ull, after = 0ull;
#pragma unroll
                for (int k = 0; k < kMaxChunks; ++k)
                    if (k == c) { before = bits[k]; own = bits[k + 1]; after = bits[k + 2]; }
                unsigned long long grown = own;
                for (int k = 1; k <= dilate; ++k) grown |= (own << k) | (own >> k) | (before >> (64 - k)) | (after << (64 - k));
                // only samples of the ray, and never its last one
                const int left = S - 1 - c * 64;
                if (left < 64) grown &= left <= 0 ? 0ull : ((1ull << left) - 1ull);
                if (lane == 0) s_mask[slot][c] = grown;
                total += __popcll(grown);
            }
        }
        if (lane == 0) s_cnt[slot] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int i = 0; i < 4 * kSelRays; ++i) {
            const int c = s_cnt[i];
            s_cnt[i] = sum;          // exclusive prefix
            sum += c;
        }
        s_base = sum ? atomicAdd(count, sum) : 0;
    }
    __syncthreads();
    for (int r = 0; r < kSelRays; ++r) {
        const int slot = wave * kSelRays + r;
        const long long ray = ((long long)blockIdx.x * 4 + wave) * kSelRays + r;
        if (ray >= n_rays) continue;
        int at = s_base + s_cnt[slot];
        for (int c = 0; c < n_chunks; ++c) {
            const unsigned long long sel = s_mask[slot][c];
            if ((sel >> lane) & 1ull) list[at + __popcll(sel & ((1ull << lane) - 1ull))] = (int)(ray * S + c * 64 + lane);
            at += __popcll(sel);
        }
    }
}

// ---------------------------------------------------------------------------------------
// composite_bwd: gradient of the composited colour (nerf.py:184-254) w.r.t. the raw network outputs.
// One wave per ray.  Pass 1 re-runs the forward scan (weights w_i and transmittances T_i parked in LDS, sums R_c, O);
// pass 2 walks the samples backwards with a suffix sum:
//   out_c = R_c O + bg (1 - O);  dR_c = g_c O;  dO = sum_c g_c (R_c - bg);  G_i = sum_c dR_c c_ic + dO
//   d raw_ic = dR_c w_i c_ic (1 - c_ic);  d alpha_i = G_i T_i - (sum_{k>i} G_k w_k) / t_i
//   d sigma_i = [sigma_i + noise_i > 0] dist_i exp(-relu(.) dist_i) d alpha_i
// z carries no gradient (nerf.py:145 stop_gradient; coarse z are constants).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void composite_bwd_kernel(
    const float4* __restrict__ rgbs, const float* __restrict__ z, const float* __restrict__ rayd,
    const float* __restrict__ noise, long long n_rays, int S, float bg, const float* __restrict__ d_rgb,
    float4* __restrict__ d_rgbs) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * 4 + wv;
    if (ray >= n_rays) return;  // wave-uniform
    float* w_s = reinterpret_cast<float*>(smem_raw) + (size_t)wv * 2 * S;
    float* T_s = w_s + S;
    const float dx = rayd[3 * ray], dy = rayd[3 * ray + 1], dz = rayd[3 * ray + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const long long base = ray * S;
    float carry = 1.0f, s_w = 0.f, s_r = 0.f, s_g = 0.f, s_b = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const int sc = valid ? s : S - 1;
        const float4 raw = rgbs[base + sc];
        const float zc = z[base + sc];
        const float zn = (sc < S - 1) ? z[base + sc + 1] : 0.f;
        const float dist = ((sc < S - 1) ? (zn - zc) : 1e10f) * dnorm;
        float sg = raw.w;
        if (noise) sg = sg + noise[base + sc];
        const float alpha = 1.0f - expf(-fmaxf(sg, 0.0f) * dist);
        const float t = valid ? (1.0f - alpha + 1e-6f) : 1.0f;
        float incl = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl *= up;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float T = carry * excl;
        const float w = valid ? alpha * T : 0.0f;
        carry = carry * __shfl(incl, 63, 64);
        if (valid) {
            w_s[s] = w;
            T_s[s] = T;
        }
        s_w += w;
        s_r += w * sigmoidf(raw.x);
        s_g += w * sigmoidf(raw.y);
        s_b += w * sigmoidf(raw.z);
    }
    s_w = wave_sum(s_w);
    s_r = wave_sum(s_r);
    s_g = wave_sum(s_g);
    s_b = wave_sum(s_b);
    const float g0 = d_rgb[3 * ray], g1 = d_rgb[3 * ray + 1], g2 = d_rgb[3 * ray + 2];
    const float dR0 = g0 * s_w, dR1 = g1 * s_w, dR2 = g2 * s_w;
    const float dO = g0 * (s_r - bg) + g1 * (s_g - bg) + g2 * (s_b - bg);
    float tail = 0.f;  // sum of G_k w_k over the chunks behind the current one
    const int n_chunks = (S + 63) / 64;
    for (int c = n_chunks - 1; c >= 0; --c) {
        const int s = c * 64 + lane;
        const bool valid = s < S;
        const int sc = valid ? s : S - 1;
        const float4 raw = rgbs[base + sc];
        const float zc = z[base + sc];
        const float zn = (sc < S - 1) ? z[base + sc + 1] : 0.f;
        const float dist = ((sc < S - 1) ? (zn - zc) : 1e10f) * dnorm;
        float sg = raw.w;
        if (noise) sg = sg + noise[base + sc];
        const float e = expf(-fmaxf(sg, 0.0f) * dist);
        const float t = 1.0f - (1.0f - e) + 1e-6f;
        const float w = valid ? w_s[sc] : 0.f, T = valid ? T_s[sc] : 0.f;
        const float c0 = sigmoidf(raw.x), c1 = sigmoidf(raw.y), c2 = sigmoidf(raw.z);
        const float G = dR0 * c0 + dR1 * c1 + dR2 * c2 + dO;
        const float v = valid ? G * w : 0.f;
        float incl = v;  // inclusive suffix sum inside the chunk
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float dn = __shfl_down(incl, o, 64);
            if (lane + o < 64) incl += dn;
        }
        const float suffix = incl - v + tail;  // strictly behind this sample
        tail += __shfl(incl, 0, 64);
        const float d_alpha = G * T - suffix / t;
        const float d_sg = sg > 0.f ? dist * e * d_alpha : 0.f;
        if (valid)
            d_rgbs[base + s] = make_float4(dR0 * w * c0 * (1.f - c0), dR1 * w * c1 * (1.f - c1),
                                           dR2 * w * c2 * (1.f - c2), d_sg);
    }
}

// ---------------------------------------------------------------------------------------
// sample_fine: block = 256 threads = 4 rays.  Dynamic LDS per wave:
//   cdf[nc-1], mid[nc-1], zall[nc+nf]   (floats)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_fine_kernel(
    const float* __restrict__ z, const float* __restrict__ weights, long long n_rays, int nc, int nf,
    const float* __restrict__ u, float* __restrict__ z_all) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* smem = reinterpret_cast<float*>(smem_raw);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = nc - 2;          // pdf bins = weights[:, 1:-1]        (nerf.py:142)
    const int ncdf = nc - 1;        // cdf entries = mids                 (util/math.py:76)
    const int ntot = nc + nf;
    const int per_wave = 2 * ncdf + ntot;
    float* cdf = smem + wave * per_wave;
    float* mid = cdf + ncdf;
    float* zall = mid + ncdf;
    const long long ray = (long long)blockIdx.x * 4 + wave;
    const bool active = ray < n_rays;
    const long long rc = active ? ray : n_rays - 1;
    const float* zr = z + rc * nc;
    const float* wr = weights + rc * nc;

    for (int i = lane; i < nc; i += 64) zall[i] = zr[i];
    for (int i = lane; i < ncdf; i += 64) mid[i] = 0.5f * (zr[i + 1] + zr[i]);  // nerf.py:140
    // util/math.py:72-76 with the oracle's summation order (sequential, left to right).  The two running sums are serial
    // by definition; they run on values held one per lane (weights loaded in parallel, element i fetched with a
    // wave-uniform readlane) instead of lane 0 walking global memory / LDS one dependent access at a time — r01: 12 k
    // cycles per ray, 1.35 ms per 640 000 rays.  Up to 4 x 64 bins.
    constexpr int kMaxSeg = 4;
    float wv[kMaxSeg];
#pragma unroll
    for (int k = 0; k < kMaxSeg; ++k) wv[k] = (64 * k + lane < nb) ? wr[1 + 64 * k + lane] : 0.f;
    float denom = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxSeg; ++k) {
        const int cnt = nb - 64 * k < 64 ? nb - 64 * k : 64;
        for (int i = 0; i < cnt; ++i) denom += __shfl(wv[k], i, 64);
    }
    denom += 1e-5f;
    float pdf[kMaxSeg], cv[kMaxSeg];
#pragma unroll
    for (int k = 0; k < kMaxSeg; ++k) {
        pdf[k] = wv[k] / denom;
        cv[k] = 0.f;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxSeg; ++k) {
        const int cnt = nb - 64 * k < 64 ? nb - 64 * k : 64;
        for (int i = 0; i < cnt; ++i) {
            acc += __shfl(pdf[k], i, 64);
            if (lane == i) cv[k] = acc;
        }
    }
    if (lane == 0) cdf[0] = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxSeg; ++k)
        if (64 * k + lane < nb) cdf[1 + 64 * k + lane] = cv[k];
    __syncthreads();
    for (int i = lane; i < nf; i += 64) {
        const float uu = u ? u[rc * nf + i] : linspace01(i, nf);
        // searchsorted(side='right') = #(cdf <= u); cdf is non-decreasing
        int lo = 0, hi = ncdf;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (cdf[m] <= uu) lo = m + 1; else hi = m;
        }
        const int ind = lo;
        const int below = ind - 1 > 0 ? ind - 1 : 0;
        const int above = ind < ncdf - 1 ? ind : ncdf - 1;
        const float cb = cdf[below], ca = cdf[above];
        float den = ca - cb;
        den = den < 1e-5f ? 1.0f : den;
        const float t = (uu - cb) / den;
        const float vb = mid[below], va = mid[above];
        zall[nc + i] = vb + t * (va - vb);
    }
    __syncthreads();
    // tf.sort(concat(z_coarse, z_fine)): rank of every element, ties by position in the concatenation.
    if (u == nullptr) {
        // deterministic sampling: both lists are already sorted (z_coarse always is; the inverse cdf is monotone in u),
        // so a rank is an index plus one binary search in the other list — same permutation as the general path
        const float* zc = zall;
        const float* zf = zall + nc;
        for (int i = lane; i < ntot; i += 64) {
            const float v = zall[i];
            int lo = 0, hi, rank;
            if (i < nc) {           // coarse element: fine elements strictly below it come first
                hi = nf;
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (zf[m] < v) lo = m + 1; else hi = m;
                }
                rank = i + lo;
            } else {                // fine element: coarse elements below or EQUAL come first (lower index wins ties)
                hi = nc;
                while (lo < hi) {
                    const int m = (lo + hi) >> 1;
                    if (zc[m] <= v) lo = m + 1; else hi = m;
                }
                rank = (i - nc) + lo;
            }
            if (active) z_all[ray * ntot + rank] = v;
        }
        return;
    }
    // random u: z_fine is unsorted -> all-pairs ranking, exact for any input order
    for (int i = lane; i < ntot; i += 64) {
        const float v = zall[i];
        int rank = 0;
        for (int j = 0; j < ntot; ++j) {
            const float o = zall[j];
            rank += (o < v) || (o == v && j < i);
        }
        if (active) z_all[ray * ntot + rank] = v;
    }
}

}  // namespace nfx

extern "C" {
int nfx_launch_l2_normalize3(const float* in, float* out, long long n, float eps, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(nfx::l2_normalize3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       in, out, n, eps);
    return (int)hipGetLastError();
}
int nfx_launch_gen_z(float near, float far, int n_samples, long long n_rays, int lin_in_disp,
                     const float* u, float* z, hipStream_t st) {
    const long long tot = n_rays * n_samples;
    if (tot <= 0) return 0;
    hipLaunchKernelGGL(nfx::gen_z_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, near,
                       far, n_samples, n_rays, lin_in_disp, u, z);
    return (int)hipGetLastError();
}
int nfx_launch_composite(const float* rgbs, const float* z, const float* rayd, const float* noise,
                         long long n_rays, int S, int white_bg, float* rgb, float* occu, float* depth,
                         float* disp, float* w, hipStream_t st) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(nfx::composite_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st,
                       (const float4*)rgbs, z, rayd, noise, n_rays, S, white_bg ? 1.0f : 0.0f, rgb,
                       occu, depth, disp, w);
    return (int)hipGetLastError();
}
int nfx_launch_surface(const float* sigma, const float* z, const float* rayo, const float* rayd, long long n_rays, int S,
                       float occu_thres, int quantize, float* alpha, float* xyz, float* depth, float* occu, hipStream_t st) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(nfx::surface_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st, sigma, z, rayo, rayd,
                       n_rays, S, occu_thres, quantize, alpha, xyz, depth, occu);
    return (int)hipGetLastError();
}
int nfx_launch_refine_select(const float* rgbs, const float* z, const float* rayd, long long n_rays, int S, float t_min,
                             float a_lo, float a_hi, float sigma_margin, int dilate, int* list, int* count, hipStream_t st) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(nfx::refine_select_kernel, dim3((unsigned)((n_rays + 4 * nfx::kSelRays - 1) / (4 * nfx::kSelRays))), dim3(256), 0, st,
                       (const float4*)rgbs, z, rayd, n_rays, S, t_min, a_lo, a_hi, sigma_margin, dilate, list, count);
    return (int)hipGetLastError();
}
int nfx_launch_sample_fine(const float* z, const float* w, long long n_rays, int nc, int nf,
                           const float* u, float* z_all, hipStream_t st) {
    if (n_rays <= 0) return 0;
    const size_t lds = (size_t)4 * (2 * (nc - 1) + nc + nf) * sizeof(float);
    hipLaunchKernelGGL(nfx::sample_fine_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), lds, st,
                       z, w, n_rays, nc, nf, u, z_all);
    return (int)hipGetLastError();
}
int nfx_launch_composite_bwd(const float* rgbs, const float* z, const float* rayd, const float* noise,
                             long long n_rays, int n_samples, int white_bg, const float* d_rgb, float* d_rgbs,
                             hipStream_t st) {
    if (n_rays <= 0) return 0;
    const size_t lds = (size_t)4 * 2 * n_samples * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(nfx::composite_bwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(nfx::composite_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), lds, st,
                       (const float4*)rgbs, z, rayd, noise, n_rays, n_samples, white_bg ? 1.0f : 0.0f, d_rgb,
                       (float4*)d_rgbs);
    return (int)hipGetLastError();
}
}

namespace nfx {
// tf.debugging.check_numerics as ONE pass over the tensor (torch.isfinite(x).all() is abs + compare + reduce with two
// full-size temporaries — 1.1 ms per 800 x 800 NeRFactor view for the [n, 512] visibilities alone): ORs 1 into *flag
// if any element has an all-ones exponent.  16-byte loads, grid-stride.
__global__ __launch_bounds__(256) void nonfinite_kernel(const unsigned* __restrict__ x, long long n, int* __restrict__ flag) {
    const long long n4 = n / 4;
    const uint4* x4 = reinterpret_cast<const uint4*>(x);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const uint4 v = x4[i];
        bad = bad || (v.x & 0x7f800000u) == 0x7f800000u || (v.y & 0x7f800000u) == 0x7f800000u ||
              (v.z & 0x7f800000u) == 0x7f800000u || (v.w & 0x7f800000u) == 0x7f800000u;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4))
        bad = bad || (x[4 * n4 + threadIdx.x] & 0x7f800000u) == 0x7f800000u;
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// tf.scatter_nd of the foreground rows into a zero tensor (nerfactor.py:295-306, shape.py:171-176) as ONE pass: every
// output row is written exactly once — its compact row or zeros.  torch.zeros + index_put_ wrote the [n, 512]
// visibilities twice and read the compact copy once (0.4 + 1.3 ms per 800 x 800 NeRFactor view, the 5th-largest kernel
// of the render legs in round 2).  row_of[i] = compact row of full row i, or -1.  V = 4: rows of d4 float4 each.
// Zero-fill of the BACKGROUND rows only (round 6): the rows of the foreground points are written, once, by the kernel that
// computes them (nfx_lvis_fwd_rows stores every visibility at its final row); row_of[i] < 0 marks a background row.
__global__ __launch_bounds__(256) void zero_rows_kernel(float4* __restrict__ dst, const int* __restrict__ row_of, unsigned n_elems,
                                                        unsigned per_row) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n_elems; i += gridDim.x * 256u)
        if (row_of[i / per_row] < 0) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const T* __restrict__ src, const int* __restrict__ row_of,
                                                           unsigned n_elems, unsigned per_row, T* __restrict__ dst) {
    T zero;
    __builtin_memset(&zero, 0, sizeof(T));
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n_elems; i += gridDim.x * 256u) {
        const unsigned row = i / per_row, col = i - row * per_row;
        const int r = row_of[row];
        dst[i] = r >= 0 ? src[(unsigned long long)r * per_row + col] : zero;
    }
}
}  // namespace nfx

extern "C" int nfx_launch_scatter_rows(const float* src, const int* row_of, long long n_all, int d, float* dst,
                                       hipStream_t st) {
    if (n_all <= 0 || d <= 0) return 0;
    const bool v4 = d % 4 == 0 && (reinterpret_cast<uintptr_t>(src) % 16 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
    const long long per_row = v4 ? d / 4 : d, n_elems = n_all * per_row;
    if (n_elems > (1ll << 31) + (1ll << 20)) return (int)hipErrorInvalidValue;   // (the C-ABI wrapper splits such calls: the 32-bit loop index must not wrap)
    long long blocks = (n_elems + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (v4)
        hipLaunchKernelGGL(nfx::scatter_rows_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(src), row_of, (unsigned)n_elems, (unsigned)per_row,
                           reinterpret_cast<float4*>(dst));
    else
        hipLaunchKernelGGL(nfx::scatter_rows_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, src, row_of,
                           (unsigned)n_elems, (unsigned)per_row, dst);
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_zero_rows(float* dst, const int* row_of, long long n_all, int d, hipStream_t st) {
    if (n_all <= 0 || d <= 0) return 0;
    const long long per_row = d / 4;            // (the C-ABI wrapper checks d % 4 == 0 and the alignment)
    // rows in slices of < 2^31 elements: the kernel's index is 32 bits
    const long long rows_per_call = ((1ll << 31) - 1) / per_row;
    for (long long r0 = 0; r0 < n_all; r0 += rows_per_call) {
        const long long rows = n_all - r0 < rows_per_call ? n_all - r0 : rows_per_call;
        const long long n_elems = rows * per_row;
        long long blocks = (n_elems + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(nfx::zero_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<float4*>(dst) + r0 * per_row, row_of + r0, (unsigned)n_elems, (unsigned)per_row);
    }
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_nonfinite(const float* x, long long n, int* flag, hipStream_t st) {
    if (n <= 0) return 0;
    long long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(nfx::nonfinite_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const unsigned*>(x), n, flag);
    return (int)hipGetLastError();
}
