// brdf_sphere.hip — the BRDF prior rendered on spheres (reference: brdf/renderer.py:167-181 over models/brdf.py:57-66):
//   rgb[b, i, :] = sum over lights l with lweight[l, :] != 0 and local l.z > 0 of  brdf(z[b], rusink(R_i l_i, R_i v_i)) * lweight[l, :] * l.z
// for n_iden identities x n sphere samples, straight to pixels: no [n_iden n, L] intermediate and no atomics.
//
// Rows.  A (sample, light) row is the row of the default nfx_brdf_spec_fwd (brdf_compact_kernel<4, 1, 4>, lvis_v2.hip):
// front-lit decision and cosine from dir_to / world2local / mat3_apply (geom.hpp), closed-form Rusinkiewicz inputs
// (brdf_point_frame + brdf_row_angles of brdf_row.hpp, the functions that kernel calls), the packed fragments of
// mlp128_layout.hpp resident in LDS (mlp128_resident.hpp: size and fragment offsets), bias-initialised accumulators,
// k-steps in ascending order, bf16 ReLU epilogue (mlp_engine.hpp's plain network pass, not the pipelined ladder), softplus.
// The specular value of a row is the same bits as that kernel's.
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
#include "brdf_row.hpp"
#include "mlp128_resident.hpp"
#include "launchers.hpp"

namespace nfx {
namespace sph {

constexpr int kNW = 4, kCT = 4, kMaxLights = 1024;
using res128::kLdsNet;
using res128::frag_off;
constexpr int kLdsLx = kLdsNet, kLdsIdx = kLdsLx + kMaxLights * 12, kLdsCount = kLdsIdx + kMaxLights * 2;
constexpr int kLds = kLdsCount + 16;
static_assert(kLds <= 160 * 1024, "LDS");

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
