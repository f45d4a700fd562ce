// nerf_geom_body.hpp — density and its spatial gradient at sample points, once: sigma_raw(x) = sigma_out(enc(posenc(x)))
// and n(x) = -normalize(d relu(sigma_raw) / dx), the per-sample "normal" of geometry_from_nerf.py:280-297 (there a
// GradientTape.batch_jacobian through embedder + fine_enc + fine_sigma_out).  One fused body: forward through the 8 x 256
// encoder keeping 1-bit ReLU masks, reverse sweep with the transposed weights in the same register-resident MFMA
// dataflow, input-gradient tiles landing in the positional-encoding SLOT layout, analytic posenc Jacobian.  GRAD = false
// stops after the sigma tile (eval_sigma_mlp, geometry_from_nerf.py:322-350, before its relu): no masks are kept and
// the weight stream wraps right after the sigma tile — none of the reverse-sweep chunks is fetched.
//
// The arithmetic is the policy A: geo::Bf16<NW> (nerf_geom.hip) or geo3::X3 (nerf_geom_x3.hip: hi / lo pairs, three
// MFMAs per product).  A policy supplies
//   Op, Stream, kNW                          the operand of 8 features, the weight stream, the waves of a workgroup
//   kFloatOffset, n_floats<GRAD>(), floats(smem)         the floats in the blob, how many are staged, and where
//   open<GRAD>(st, smem, blob, fl, tid)      stream set-up and first chunk
//   kMasks<GRAD>                             does the forward keep the ReLU masks
//   posenc(x, h, pe), relu_to(acc, lo8, hi8), put(dst, t, r, v), sigma(acc, p)    values into operands and out of a tile
//   tile<KS1, KS2, NL>(st, tid, bias, b1, b2, acc)       a forward tile from its bias
//   tile_zero<NL>(st, tid, fl, dz, acc)                  a reverse-sweep tile from zero
//   tile_add<NL>(st, tid, fl, dz, sum)                   an input-gradient tile added to `sum`
// and keeps its own order of additions in them.
//
// What the compiler forced (profiles/geom_body/code_objects.txt): a function that is inlined into a kernel is optimised on its
// own first, without the kernel's launch bounds, and the march's small run-time-indexed arrays then take another road through
// the optimiser than the same lines written in the kernel.  The density kernels come out of nerf_sigma_body() with the
// parent's code objects.  The gradient kernels do not: the fp32-class one goes from 328 to 1192 bytes of scratch, the bf16
// ones get another VALU selection that measures 0.9 % slower.  So each gradient __global__ function holds its own tile loop
// around the shared pieces — forward(), reverse_sweep() and, fp32-class, grad_point() / normal_sigma(); the bf16 kernel
// needs the Jacobian's lines in the __global__ function as well.
#pragma once
#include "feat_store.hpp"
#include "nerf_geom_layout.hpp"
#include "nerf_points.hpp"

namespace nfx {
namespace geo {

constexpr int kNLD = 4;  // every backward chunk: 16 fragments

// a Dense + ReLU layer of 8 tiles; MASKS: keep the sign of every pre-activation, one bit each
template <typename A, bool MASKS, int KS1, int KS2, int NL_SELF, int NL_NEXT, int KS1A, int KS2A>
__device__ __forceinline__ void fwd_layer(typename A::Stream& st, int tid, const float* bias, const typename A::Op (&b1)[KS1A],
                                          const typename A::Op (&b2)[KS2A], typename A::Op (&bout)[16], unsigned (&m)[4]) {
    static_for<0, 8>([&](auto T) {
        constexpr int t = decltype(T)::value;
        f32x16 acc;
        A::template tile<KS1, KS2, (t == 7 ? NL_NEXT : NL_SELF)>(st, tid, bias + 32 * t, b1, b2, acc);
        if constexpr (MASKS) {
            const unsigned bits = bwd::relu_bits16(acc);
            if constexpr (t & 1) m[t >> 1] |= bits << 16;
            else m[t >> 1] = bits;
        }
        A::relu_to(acc, bout[2 * t], bout[2 * t + 1]);
    });
}

template <typename A>
__device__ __forceinline__ void dgrad(typename A::Stream& st, int tid, const float* fl, const typename A::Op (&dz)[16],
                                      const unsigned (&m)[4], typename A::Op (&dout)[16]) {
    static_for<0, 8>([&](auto T) {
        constexpr int t = decltype(T)::value;
        f32x16 acc;
        A::template tile_zero<kNLD>(st, tid, fl, dz, acc);
        static_for<0, 16>([&](auto R) {
            constexpr int r = decltype(R)::value;
            A::put(dout, t, r, bwd::mask_bit(m, t, r) ? acc[r] : 0.f);
        });
    });
}

// d posenc-slot accumulators += (input rows of a layer)^T dz: 2 tiles = 32 slots per lane half
template <typename A, int NL_LAST>
__device__ __forceinline__ void input_grad(typename A::Stream& st, int tid, const float* fl, const typename A::Op (&dz)[16],
                                           f32x16 (&dpe)[2]) {
    static_for<0, 2>([&](auto T) {
        constexpr int t = decltype(T)::value;
        A::template tile_add<(t == 1 ? NL_LAST : kNLD)>(st, tid, fl, dz, dpe[t]);
    });
}

// The encoder and the sigma tile: the raw density of this lane's point (row 0 of the tile, on the h = 0 lanes).  GRAD: the
// chunk after the sigma tile is the reverse sweep's first, else enc[0] tile 0 again.
template <typename A, bool GRAD>
__device__ __forceinline__ float forward(typename A::Stream& st, int tid, const float* fl, int p, const typename A::Op (&pe)[4],
                                         typename A::Op (&ha)[16], typename A::Op (&hb)[16], unsigned (&mk)[8][4]) {
    using namespace nerf;
    constexpr bool M = A::template kMasks<GRAD>;
    fwd_layer<A, M, 4, 0, kNL0, kNLH>(st, tid, fl + 256 * 0, pe, pe, ha, mk[0]);
    fwd_layer<A, M, 16, 0, kNLH, kNLH>(st, tid, fl + 256 * 1, ha, pe, hb, mk[1]);
    fwd_layer<A, M, 16, 0, kNLH, kNLH>(st, tid, fl + 256 * 2, hb, pe, ha, mk[2]);
    fwd_layer<A, M, 16, 0, kNLH, kNLH>(st, tid, fl + 256 * 3, ha, pe, hb, mk[3]);
    fwd_layer<A, M, 16, 0, kNLH, kNL5>(st, tid, fl + 256 * 4, hb, pe, ha, mk[4]);
    fwd_layer<A, M, 16, 4, kNL5, kNLH>(st, tid, fl + 256 * 5, ha, pe, hb, mk[5]);
    fwd_layer<A, M, 16, 0, kNLH, kNLH>(st, tid, fl + 256 * 6, hb, pe, ha, mk[6]);
    fwd_layer<A, M, 16, 0, kNLH, kNLH>(st, tid, fl + 256 * 7, ha, pe, hb, mk[7]);
    f32x16 acc;
    A::template tile<16, 0, (GRAD ? kNLD : kNL0)>(st, tid, fl + kGeoBiasSig, hb, pe, acc);
    return A::sigma(acc, p);
}

// dZ7 = mask7 . W_sigma (the same vector for every point: no MFMA), then the reverse sweep into the posenc-slot sums dpe
template <typename A>
__device__ __forceinline__ void reverse_sweep(typename A::Stream& st, int tid, const float* fl, int h, const unsigned (&mk)[8][4],
                                              typename A::Op (&ha)[16], typename A::Op (&hb)[16], f32x16 (&dpe)[2]) {
    using namespace nerf;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float wv = fl[kGeoWSig + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h];
            A::put(ha, t, r, bwd::mask_bit(mk[7], t, r) ? wv : 0.f);
        }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dpe[t][r] = 0.f;
    dgrad<A>(st, tid, fl, ha, mk[6], hb);          // enc[7]^T -> dZ6
    dgrad<A>(st, tid, fl, hb, mk[5], ha);          // enc[6]^T -> dZ5
    input_grad<A, kNLD>(st, tid, fl, ha, dpe);     // enc[5][256:]^T dZ5 -> posenc slots
    dgrad<A>(st, tid, fl, ha, mk[4], hb);          // enc[5][:256]^T -> dZ4
    dgrad<A>(st, tid, fl, hb, mk[3], ha);          // enc[4]^T -> dZ3
    dgrad<A>(st, tid, fl, ha, mk[2], hb);          // enc[3]^T -> dZ2
    dgrad<A>(st, tid, fl, hb, mk[1], ha);          // enc[2]^T -> dZ1
    dgrad<A>(st, tid, fl, ha, mk[0], hb);          // enc[1]^T -> dZ0
    input_grad<A, kNL0>(st, tid, fl, hb, dpe);     // enc[0]^T dZ0 -> posenc slots; next chunk = L0 of the next tile
}

// posenc Jacobian (slot q = 8 s + j) of the slot sums, both lane halves added: (-normalize(d relu(sigma) / dx), sigma)
__device__ __forceinline__ float4 normal_sigma(const f32x16 (&dpe)[2], const float (&x)[3], int h, float sigma) {
    float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const float dq = dpe[q >> 4][q & 15];
        if (q < 30) {
            const float freq = (float)(1 << (q / 3));
            // half 0 holds sin(f x): d/dx = f cos(f x); half 1 holds cos(f x): d/dx = -f sin(f x)
            const float other = sin_shifted(x[q % 3] * freq, h ^ 1);
            g[q % 3] += dq * freq * (h ? -other : other);
        } else if (q == 30) {
            if (h) g[2] += dq; else g[0] += dq;
        } else {
            if (!h) g[1] += dq;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += __shfl_xor(g[k], 32, 64);
    const float on = sigma > 0.f ? 1.f : 0.f;           // gradient of relu(sigma_raw)
    const float gx = g[0] * on, gy = g[1] * on, gz = g[2] * on;
    const float inv = -1.0f / sqrtf(fmaxf(gx * gx + gy * gy + gz * gz, 1e-12f));  // -l2_normalize(., eps 1e-12)
    return make_float4(gx * inv, gy * inv, gz * inv, sigma);
}

// the floats of the blob to LDS, the weight stream opened on its first chunk: the staged floats
template <typename A, bool GRAD>
__device__ __forceinline__ float* start(typename A::Stream& st, char* smem, const char* blob, int tid) {
    float* fl = A::floats(smem);
    const float* src = reinterpret_cast<const float*>(blob + A::kFloatOffset);
    for (int i = tid; i < A::template n_floats<GRAD>(); i += A::kNW * 64) fl[i] = src[i];
    A::template open<GRAD>(st, smem, blob, fl, tid);
    return fl;
}

// One point of the gradient march: (normal, sigma) of flat sample mm
template <typename A>
__device__ __forceinline__ float4 grad_point(typename A::Stream& st, int tid, const float* fl, const Points& pts, long long mm) {
    const int lane = tid & 63, h = lane >> 5, p = lane & 31;
    float x[3];
    pts.position(mm, x);
    typename A::Op pe[4], ha[16], hb[16];
    A::posenc(x, h, pe);
    unsigned mk[8][4];
    const float sigma = forward<A, true>(st, tid, fl, p, pe, ha, hb, mk);
    f32x16 dpe[2];
    reverse_sweep<A>(st, tid, fl, h, mk, ha, hb, dpe);
    return normal_sigma(dpe, x, h, sigma);
}

// The density march over the points of a launch, 32 per wave and trip: no masks, no reverse sweep (nerf_points.hpp says
// where a density goes).  The gradient kernels write this loop out in their __global__ functions (see the top of the file);
// the lines from counted() to sample() are the same there and change together.
template <typename A>
__device__ __forceinline__ void nerf_sigma_body(const Points& pts, const char* blob, float* out, char* smem) {
    constexpr int kRows = A::kNW * 32;
    long long n_pts;
    if (!pts.counted(kRows, n_pts)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    typename A::Stream st;
    const float* fl = start<A, false>(st, smem, blob, tid);
    const long long n_tiles = (n_pts + kRows - 1) / kRows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row = tile * kRows + wave * 32 + p;
        const bool valid = row < n_pts;
        const long long mm = pts.sample(row, n_pts);
        float x[3];
        pts.position(mm, x);
        typename A::Op pe[4], ha[16], hb[16];
        A::posenc(x, h, pe);
        unsigned mk[8][4];
        const float sigma = forward<A, false>(st, tid, fl, p, pe, ha, hb, mk);
        if (valid && h == 0) pts.store_sigma(out, row, mm, sigma);
    }
}

}  // namespace geo
}  // namespace nfx
