// brdf_sphere.hip — the BRDF prior rendered on spheres (reference: brdf/renderer.py:167-181 over models/brdf.py:57-66):
//   rgb[b, i, :] = sum over lights l with lweight[l, :] != 0 and local l.z > 0 of  brdf(z[b], rusink(R_i l_i, R_i v_i)) * lweight[l, :] * l.z
// for n_iden identities x n sphere samples, straight to pixels: no [n_iden n, L] intermediate and no atomics.
//
// Rows.  A (sample, light) row is the row of the default nfx_brdf_spec_fwd (brdf_compact_kernel<4, 1, 4>, lvis_v2.hip):
// front-lit decision and cosine from dir_to / world2local / mat3_apply (geom.hpp), closed-form Rusinkiewicz inputs
// (brdf_point_frame + brdf_row_angles below: the same statements as lvis_v2.hip's, which stays untouched because the
// bit-for-bit suites pin its code object; -ffp-contract=off makes equal statements equal bits), the packed fragments of
// mlp128_layout.hpp resident in LDS, bias-initialised accumulators, k-steps in ascending order, bf16 ReLU epilogue
// (mlp_engine.hpp), softplus.  The specular value of a row is the same bits as that kernel's.
//
// Dataflow.  4 waves per workgroup, one per SIMD, network loaded once (138 KiB).  Wave 0 then COMPACTS the lights: the
// indices and positions of the lights with a non-zero weight, ascending, go to LDS (<= 14 KiB); dark lights cost nothing
// afterwards (the 'point' probe lights 16 of 512).  A wave owns the (identity, sample) pairs gw, gw + nw, ...; it walks a
// pair's 32-light tiles of the compacted list in ascending order, drops a tile when a ballot finds none of its lights in
// front of the sample, and queues the others — CT tiles per pass through the network, possibly of consecutive pairs, so a
// pair with one live tile does not run three empty column tiles.  After a pass the 32 softplus values of a tile are
// multiplied by lweight * cos, summed by a fixed butterfly over lanes 0-31 and added to the pair's three fp32
// accumulators; the pair is stored when the queue moves on to the next one.  A pair's value depends on its own tiles, in
// their order, and on nothing else in the launch: bit-reproducible at any batch size and grid.
// A pair without a lit front-facing light stores 0.0.
#include "geom.hpp"
#include "mlp128_layout.hpp"
#include "mlp_engine.hpp"
#include "launchers.hpp"

namespace nfx {
namespace sph {

constexpr int kNW = 4, kCT = 4, kMaxLights = 1024;
constexpr int kLdsNet = m128::kMainWeightBytes + m128::kMainBiasFloats * 4;
constexpr int kLdsLx = kLdsNet, kLdsIdx = kLdsLx + kMaxLights * 12, kLdsCount = kLdsIdx + kMaxLights * 2;
constexpr int kLds = kLdsCount + 16;
static_assert(kLds <= 160 * 1024, "LDS");
// fragment offset of chunk K: L0 0-3 (4 frags), L1 4-7, L2 8-11 (8 frags), L3 12-15 (12 frags), out 16
constexpr int frag_off(int k) { return k < 4 ? 4 * k : k < 12 ? 16 + 8 * (k - 4) : k < 16 ? 80 + 12 * (k - 12) : 128; }

// ---- closed-form row geometry: statement for statement lvis_v2.hip's (acos_poly .. brdf_row_angles)
__device__ __forceinline__ float acos_poly(float x) {   // Abramowitz-Stegun 4.4.46, |err| <= 2e-8 + fp32 rounding
    const float ax = fabsf(x);
    float p = -0.0012624911f;
    p = fmaf(p, ax, 0.0066700901f);
    p = fmaf(p, ax, -0.0170881256f);
    p = fmaf(p, ax, 0.0308918810f);
    p = fmaf(p, ax, -0.0501743046f);
    p = fmaf(p, ax, 0.0889789874f);
    p = fmaf(p, ax, -0.2145988016f);
    p = fmaf(p, ax, 1.5707963050f);
    const float r = sqrtf(1.0f - ax) * p;
    return x < 0.0f ? 3.14159265358979323846f - r : r;
}
__device__ __forceinline__ float atan2_poly(float y, float x) {   // Cephes atanf polynomial, |err| <= 3e-7
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float t = mx > 0.0f ? mn * __builtin_amdgcn_rcpf(mx) : 0.0f;
    const bool big = t > 0.4142135623730950f;
    const float t2 = big ? (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f) : t;
    const float zz = t2 * t2;
    float q = fmaf(8.05374449538e-2f, zz, -1.38776856032e-1f);
    q = fmaf(q, zz, 1.99777106478e-1f);
    q = fmaf(q, zz, -3.33329491539e-1f);
    float r = fmaf(q * zz, t2, t2) + (big ? 0.78539816339744830962f : 0.0f);
    r = ay > ax ? 1.57079632679489661923f - r : r;
    r = x < 0.0f ? 3.14159265358979323846f - r : r;
    return y < 0.0f ? -r : r;
}
__device__ __forceinline__ void nrm_rsq(float (&v)[3]) {
    const float inv = __builtin_amdgcn_rsqf(fmaxf(dot3(v, v), 1e-6f));
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}
// per pair: local frame [t; b; n] of the normal and the view direction in it
__device__ __forceinline__ void brdf_point_frame(const float (&x)[3], const float (&cm)[3], const float (&nr)[3],
                                                 float (&rot)[9], float (&vl)[3]) {
    float vdir[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vdir[k] = cm[k] - x[k];
    nrm_rsq(vdir);
    float n[3] = {nr[0], nr[1], nr[2]}, t[3], b[3];
    nrm_rsq(n);
    const float zax[3] = {0.0f + 1e-6f, 0.0f + 1e-6f, 1.0f + 1e-6f};   // geom.py:128
    cross3(n, zax, t);
    nrm_rsq(t);
    cross3(n, t, b);
    nrm_rsq(b);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rot[k] = t[k];
        rot[3 + k] = b[k];
        rot[6 + k] = n[k];
    }
    mat3_apply(rot, vdir, vl);
    nrm_rsq(vl);
}
// per row: S[q] is input slot q of lane half 0 (sines, phi_d, theta_h), C[q] of half 1 (cosines, theta_d; slot 7 is z_0)
__device__ __forceinline__ void brdf_row_angles(const float (&x)[3], const float (&lp)[3], const float (&rot)[9],
                                                const float (&vl)[3], float (&S)[8], float (&C)[8]) {
    auto nrm = [](float (&v)[3]) { nrm_rsq(v); };
    float ldir[3], ll[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ldir[k] = lp[k] - x[k];
    nrm(ldir);
    mat3_apply(rot, ldir, ll);
    nrm(ll);
    float hv[3] = {(ll[0] + vl[0]) * 0.5f, (ll[1] + vl[1]) * 0.5f, (ll[2] + vl[2]) * 0.5f};
    nrm(hv);
    const float cth = fminf(fmaxf(hv[2], -1.0f), 1.0f);
    const float sxy = sqrtf(hv[0] * hv[0] + hv[1] * hv[1]);
    const float inv = sxy > 0.0f ? __builtin_amdgcn_rcpf(sxy) : 0.0f;
    const float cph = sxy > 0.0f ? hv[0] * inv : 1.0f, sph = hv[1] * inv;
    const float t0 = vl[0] * cph + vl[1] * sph, t1 = vl[1] * cph - vl[0] * sph;
    const float d0 = t0 * cth - vl[2] * sxy, d1 = t1, d2 = vl[2] * cth + t0 * sxy;
    const float ctd = fminf(fmaxf(d2, -1.0f), 1.0f);
    const float rxy = sqrtf(d0 * d0 + d1 * d1);
    const float theta_h = acos_poly(cth), theta_d = acos_poly(ctd);
    const float pi = 3.14159265358979323846f;
    float phi_d = atan2_poly(d1, d0);
    phi_d = phi_d - floorf(phi_d / pi) * pi;
    const float rinv = rxy > 0.0f ? __builtin_amdgcn_rcpf(rxy) : 0.0f;
    const bool flip = d1 < 0.0f || (d1 == 0.0f && d0 < 0.0f);
    const float cpd0 = rxy > 0.0f ? d0 * rinv : 1.0f, spd0 = d1 * rinv;
    const float cpd = flip ? -cpd0 : cpd0, spd = flip ? -spd0 : spd0;
    S[0] = spd; S[1] = sxy; S[2] = rxy;
    S[3] = 2.0f * spd * cpd; S[4] = 2.0f * sxy * cth; S[5] = 2.0f * rxy * ctd;
    S[6] = phi_d; S[7] = theta_h;
    C[0] = cpd; C[1] = cth; C[2] = ctd;
    C[3] = cpd * cpd - spd * spd; C[4] = cth * cth - sxy * sxy; C[5] = ctd * ctd - rxy * rxy;
    C[6] = theta_d; C[7] = 0.0f;
}

struct Args {
    const float* xyz;      // [n,3] sphere samples
    const float* normal;   // [n,3]
    long long n;
    float cam[3];
    const float* z;        // [n_iden, z_dim]
    int z_dim, n_iden;
    const float* lxyz;     // [L,3]
    const float* lweight;  // [L,3] light * area
    int n_lights;
    const char* blob;
    float* rgb;            // [n_iden, n, 3]
};

template <int CT>
__global__ __launch_bounds__(kNW * 64, kNW / 4) void brdf_sphere_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace m128;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* lx_w = reinterpret_cast<float*>(smem + kLdsLx);
    unsigned short* lidx_w = reinterpret_cast<unsigned short*>(smem + kLdsIdx);
    {   // the whole network, once
        const u32x4* src = reinterpret_cast<const u32x4*>(a.blob);
        u32x4* dst = reinterpret_cast<u32x4*>(smem);
        for (int i = tid; i < kLdsNet / 16; i += kNW * 64) dst[i] = src[i];
        if (wave == 0) {   // the lit lights, ascending
            int cnt = 0;
            for (int l0 = 0; l0 < a.n_lights; l0 += 64) {
                const int l = l0 + lane;
                const bool valid = l < a.n_lights;
                const int lc = valid ? l : 0;
                const float w0 = a.lweight[lc * 3], w1 = a.lweight[lc * 3 + 1], w2 = a.lweight[lc * 3 + 2];
                const bool lit = valid && (w0 != 0.0f || w1 != 0.0f || w2 != 0.0f);
                const unsigned long long mask = __ballot(lit);
                const int pos = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                if (lit) {
                    lidx_w[pos] = (unsigned short)l;
#pragma unroll
                    for (int k = 0; k < 3; ++k) lx_w[pos * 3 + k] = a.lxyz[l * 3 + k];
                }
                cnt += __popcll(mask);
            }
            if (lane == 0) *reinterpret_cast<int*>(smem + kLdsCount) = cnt;
        }
        __syncthreads();
    }
    const char* wlds = smem;
    const float* bias_lds = reinterpret_cast<const float*>(smem + kMainWeightBytes);
    const float* lx = lx_w;
    const unsigned short* lidx = lidx_w;
    const int n_lit = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(smem + kLdsCount));
    const int n_t = (n_lit + 31) / 32;
    const long long total = (long long)a.n_iden * a.n;
    const long long nw = (long long)gridDim.x * kNW, gw = (long long)blockIdx.x * kNW + wave;
    auto store = [&](long long q, float r, float g, float b) {
        if (lane == 0) {
            a.rgb[q * 3] = r;
            a.rgb[q * 3 + 1] = g;
            a.rgb[q * 3 + 2] = b;
        }
    };
    // the pair the tile walk stands in
    long long kq = 0, pq = -1;
    int t = n_t, live = 1;
    float x[3], rot[9], prot[9], pvl[3], zv[17];
    // the pair the sums belong to
    long long cur = -1;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (;;) {
        bf16x8 pl[2][CT];
        float wc[CT][3];
        bool fq[CT];
        long long qid[CT];
        // ---- queue: the next CT live tiles
        static_for<0, CT>([&](auto C_) {
            constexpr int c = decltype(C_)::value;
            qid[c] = -1;
            fq[c] = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) wc[c][k] = 0.0f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) pl[s][c][j] = (__bf16)0.0f;
            for (;;) {
                if (t >= n_t) {   // next pair
                    if (pq >= 0 && live == 0) store(pq, 0.0f, 0.0f, 0.0f);
                    pq = gw + kq * nw;
                    if (pq >= total) {
                        pq = -1;
                        break;
                    }
                    ++kq;
                    const long long ib = pq / a.n, is = pq - ib * a.n;
                    float nr[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        x[k] = a.xyz[is * 3 + k];
                        nr[k] = a.normal[is * 3 + k];
                    }
                    world2local(nr, rot);
                    brdf_point_frame(x, a.cam, nr, prot, pvl);
#pragma unroll
                    for (int i = 0; i < 17; ++i) zv[i] = i < a.z_dim ? a.z[ib * a.z_dim + (i < a.z_dim ? i : 0)] : 0.0f;
                    t = 0;
                    live = 0;
                    if (n_t == 0) continue;
                }
                const int li = t * 32 + p;
                const bool valid = li < n_lit;
                const int lc = valid ? li : 0;
                const float lp[3] = {lx[lc * 3], lx[lc * 3 + 1], lx[lc * 3 + 2]};
                float ldir[3], ll[3];
                dir_to(lp, x, ldir);
                mat3_apply(rot, ldir, ll);
                const bool fr = valid && ll[2] > 0.0f;                    // nerfactor.py:429-432
                ++t;
                if (__ballot(fr) == 0ull) continue;
                ++live;
                float S[8], C[8], v[16];
                brdf_row_angles(x, lp, prot, pvl, S, C);
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = h ? C[q] : S[q];
                if (h) v[7] = zv[0];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[8 + j] = h ? zv[2 + 2 * j] : zv[1 + 2 * j];
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j) pl[s][c][j] = (__bf16)v[8 * s + j];
                const int gl = lidx[lc];
#pragma unroll
                for (int k = 0; k < 3; ++k) wc[c][k] = a.lweight[gl * 3 + k] * ll[2];
                fq[c] = fr && h == 0;
                qid[c] = pq;
                break;
            }
        });
        if (qid[0] < 0) break;
        // ---- the network on CT x 32 rows: L0 pl -> ha, L1 ha -> hb, L2 hb -> ha, L3 [ha ; pl] -> hb, out hb
        bf16x8 ha[8][CT], hb[8][CT];
        f32x16 acc[CT];
        const char* lf = wlds + lane * 16;
        static_for<0, 4>([&](auto T) {
            constexpr int tt = decltype(T)::value;
            bias_init<CT>(bias_lds + 32 * tt, h, acc);
            mma_k<2>(lf + frag_off(tt) * kFragBytes, pl, acc);
            acc_to_b<true>(acc, ha[2 * tt], ha[2 * tt + 1]);
        });
        static_for<0, 4>([&](auto T) {
            constexpr int tt = decltype(T)::value;
            bias_init<CT>(bias_lds + 128 + 32 * tt, h, acc);
            mma_k<8>(lf + frag_off(4 + tt) * kFragBytes, ha, acc);
            acc_to_b<true>(acc, hb[2 * tt], hb[2 * tt + 1]);
        });
        static_for<0, 4>([&](auto T) {
            constexpr int tt = decltype(T)::value;
            bias_init<CT>(bias_lds + 256 + 32 * tt, h, acc);
            mma_k<8>(lf + frag_off(8 + tt) * kFragBytes, hb, acc);
            acc_to_b<true>(acc, ha[2 * tt], ha[2 * tt + 1]);
        });
        static_for<0, 4>([&](auto T) {
            constexpr int tt = decltype(T)::value;
            bias_init<CT>(bias_lds + 384 + 32 * tt, h, acc);
            mma_k<8>(lf + frag_off(12 + tt) * kFragBytes, ha, acc);
            mma_k<2>(lf + (frag_off(12 + tt) + 8) * kFragBytes, pl, acc);
            acc_to_b<true>(acc, hb[2 * tt], hb[2 * tt + 1]);
        });
        bias_init<CT>(bias_lds + 512, h, acc);
        mma_k<8>(lf + frag_off(16) * kFragBytes, hb, acc);
        // ---- a tile's 32 rows (lanes 0-31, register 0) into its pair's sums
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (qid[c] < 0) continue;
            const float sp = softplusf(acc[c][0]);                        // brdf.py:65
            float r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float term = fq[c] ? sp * wc[c][k] : 0.0f;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
                r[k] = __shfl(term, 0, 64);
            }
            if (qid[c] != cur) {
                if (cur >= 0) store(cur, sum[0], sum[1], sum[2]);
                cur = qid[c];
                sum[0] = sum[1] = sum[2] = 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) sum[k] += r[k];
        }
    }
    if (cur >= 0) store(cur, sum[0], sum[1], sum[2]);
}

}  // namespace sph
}  // namespace nfx

extern "C" int nfx_launch_brdf_sphere(const float* xyz, const float* normal, long long n, const float* cam3, const float* z, int z_dim,
                                      int n_iden, const float* lxyz, const float* lweight, int n_lights, const void* blob, float* rgb,
                                      int max_blocks, hipStream_t st) {
    using namespace nfx;
    if (n <= 0 || n_iden <= 0) return 0;
    if (n_lights > sph::kMaxLights) return (int)hipErrorInvalidValue;
    sph::Args a{xyz, normal, n, {cam3[0], cam3[1], cam3[2]}, z, z_dim, n_iden, lxyz, lweight, n_lights, (const char*)blob, rgb};
    const long long pairs = n * n_iden, want = (pairs + sph::kNW - 1) / sph::kNW;
    const int grid = (int)(want < max_blocks ? want : (max_blocks > 0 ? max_blocks : 1));
    auto k = sph::brdf_sphere_kernel<sph::kCT>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, sph::kLds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(sph::kNW * 64), sph::kLds, st, a);
    return (int)hipGetLastError();
}
