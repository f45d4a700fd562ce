// nerf_geom.hip — density and its spatial gradient at sample points: sigma_raw(x) = sigma_out(enc(posenc(x))) and
// n(x) = -normalize(d relu(sigma_raw) / dx), with bf16 operands: the policy geo::Bf16 of nerf_geom_body.hpp (which holds
// the density march, the forward ladder and the reverse sweep), the gradient kernel's tile loop and posenc Jacobian, the
// density kernel as a wrapper of the body, their launchers, and the selection of the samples with a density for the list form.
#include "mlp_engine.hpp"
#include "rowsel.hpp"
#include "nerf_geom_body.hpp"
#include "launchers.hpp"

namespace nfx {
namespace geo {

constexpr int kNW = 4;
constexpr int kRows = kNW * 32;

// bf16 operands: one MFMA per product, tiles on mlp_engine.hpp's register-staged WStream
template <int NW>
struct Bf16 {
    using Op = bf16x8[1];
    using Stream = WStream;
    static constexpr int kNW = NW;
    static constexpr size_t kFloatOffset = nerf::kGeoWeightBytes;
    // density only: encoder biases + the sigma bias tile
    template <bool GRAD>
    static constexpr int n_floats() { return GRAD ? nerf::kGeoFloats : nerf::kGeoWSig; }
    template <bool GRAD>
    static constexpr bool kMasks = GRAD;
    __device__ __forceinline__ static float* floats(char* smem) { return reinterpret_cast<float*>(smem + 2 * kSlotBytes); }
    template <bool GRAD>
    __device__ __forceinline__ static void open(WStream& ws, char* smem, const char* blob, float*, int tid) {
        ws.gbase = reinterpret_cast<const u32x4*>(blob);
        ws.gend = reinterpret_cast<const u32x4*>(blob + (GRAD ? (size_t)nerf::kGeoWeightBytes : (size_t)nerf::kGeoFwdFrags * kFragBytes));
        ws.gnext = ws.gbase;
        ws.ring = smem;
        stream_prologue<nerf::kNL0, NW>(ws, tid);
    }
    __device__ __forceinline__ static void posenc(const float (&x)[3], int h, Op (&pe)[4]) { nfx::posenc<10, 1>(x, h, 0, pe); }
    __device__ __forceinline__ static void relu_to(const f32x16& acc, Op& lo8, Op& hi8) {
        const f32x16 a[1] = {acc};
        acc_to_b<true, 1>(a, lo8, hi8);
    }
    __device__ __forceinline__ static void put(Op (&dst)[16], int t, int r, float v) { dst[2 * t + (r >> 3)][0][r & 7] = (__bf16)v; }
    __device__ __forceinline__ static float sigma(const f32x16& acc, int p) { return __shfl(acc[0], p, 64); }
    template <int KS1, int KS2, int NL, int KS1A, int KS2A>
    __device__ __forceinline__ static void tile(WStream& ws, int tid, const float* bias, const Op (&b1)[KS1A], const Op (&b2)[KS2A], f32x16& acc) {
        f32x16 a[1];
        tile_raw<KS1, KS2, NL, NW>(ws, tid, bias, b1, b2, a);
        acc = a[0];
    }
    template <int NL>
    __device__ __forceinline__ static void tile_zero(WStream& ws, int tid, const float*, const Op (&dz)[16], f32x16& acc) {
        f32x16 a[1];
        tile_init<16, 0, NL, NW>(ws, tid, [&](f32x16(&i)[1]) { bwd::zero_init<1>(i); }, dz, dz, a);
        acc = a[0];
    }
    // the accumulators start from `sum`: the addition happens inside the MFMA chain
    template <int NL>
    __device__ __forceinline__ static void tile_add(WStream& ws, int tid, const float*, const Op (&dz)[16], f32x16& sum) {
        f32x16 a[1];
        tile_init<16, 0, NL, NW>(ws, tid, [&](f32x16(&i)[1]) { i[0] = sum; }, dz, dz, a);
        sum = a[0];
    }
};

// LIST: the points are the listed samples (nerf_points.hpp); a compile-time argument here, so that the every-sample kernel
// holds no list code
template <bool LIST>
__global__ __launch_bounds__(kNW * 64, 1) void nerf_sigma_grad_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float4* __restrict__ out, const int* __restrict__ list,
    const int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the gradient forms of nerf_points.hpp: every sample or a list; stride and last-sample do not apply
    if constexpr (LIST) __builtin_assume(list != nullptr);   // Points tests the pointer: the list kernel keeps no every-sample code
    const Points pts{rayo, rayd, zbuf, n_pts, n_samples, LIST ? list : nullptr, count, 4, 0};
    using A = Bf16<kNW>;
    // The tile loop and the Jacobian stand in the kernel itself, not behind a function: only so does the compiler give the
    // parent's instruction selection (nerf_geom_body.hpp, profiles/geom_body/).  The lines from counted() to sample() are
    // nerf_sigma_body()'s, the Jacobian is normal_sigma()'s: they change together.
    long long n;
    if (!pts.counted(kRows, n)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    WStream st;
    const float* fl = start<A, true>(st, smem, blob, tid);
    const long long n_tiles = (n + kRows - 1) / kRows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row = tile * kRows + wave * 32 + p;
        const bool valid = row < n;
        const long long mm = pts.sample(row, n);
        float x[3];
        pts.position(mm, x);
        A::Op pe[4], ha[16], hb[16];
        A::posenc(x, h, pe);
        unsigned mk[8][4];
        const float sigma = forward<A, true>(st, tid, fl, p, pe, ha, hb, mk);
        f32x16 dpe[2];
        reverse_sweep<A>(st, tid, fl, h, mk, ha, hb, dpe);
        // ------------------------------------------------------------------ posenc Jacobian (slot q = 8 s + j)
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
        if (valid && h == 0) {
            const float on = sigma > 0.f ? 1.f : 0.f;           // gradient of relu(sigma_raw)
            const float gx = g[0] * on, gy = g[1] * on, gz = g[2] * on;
            const float inv = -1.0f / sqrtf(fmaxf(gx * gx + gy * gy + gz * gz, 1e-12f));  // -l2_normalize(., eps 1e-12)
            out[pts.grad_row(row, mm)] = make_float4(gx * inv, gy * inv, gz * inv, sigma);
        }
    }
}

// Density only, for the shadow-ray and coarse camera marches; the sigma_variant = 0 identity reference of nerf_sigma_v6.hip.
// 8 waves x 32 points like nerf_mlp_bf16_kernel<1, 8>; same arithmetic: bit-identical sigma.
__global__ __launch_bounds__(512, 2) void nerf_sigma_geo_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = 8;
    constexpr int kTilePts = NW * 32;
    static_assert(kTilePts == 256, "the launcher's tile");
    const Points pts{rayo, rayd, zbuf, n_pts, n_samples, nullptr, nullptr, 1, 0};
    nerf_sigma_body<Bf16<NW>>(pts, blob, out, smem);
}

}  // namespace geo
}  // namespace nfx

// (normal, sigma) rows of every sample (pts.list null) or of the listed ones
extern "C" int nfx_launch_nerf_sigma_grad(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks,
                                          hipStream_t st) {
    using namespace nfx;
    if (pts->last_sample) return (int)hipErrorInvalidValue;   // the gradient has the every-sample and the list form only
    if (pts->n_pts <= 0) return 0;
    const long long tiles = (pts->n_pts + geo::kRows - 1) / geo::kRows;
    const int grid = (int)(tiles < max_blocks ? tiles : max_blocks);
    auto k = pts->list ? geo::nerf_sigma_grad_kernel<true> : geo::nerf_sigma_grad_kernel<false>;
    constexpr int lds = 2 * kSlotBytes + nerf::kGeoFloats * 4;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(geo::kNW * 64), lds, st, pts->rayo, pts->rayd, pts->z, pts->n_pts, pts->n_samples,
                       (const char*)blob, (float4*)out, pts->list, pts->count);
    return (int)hipGetLastError();
}

// The samples with a positive density, ascending (rowsel.hpp), for the LIST form of the gradient kernels; the same pass
// writes the output row of every sample without density: relu has no slope there, the gradient is zero and
// -l2_normalize(0) = 0 * (-1 / sqrt(1e-12)) = (-0, -0, -0) (the every-sample kernel forms g * 0 and so keeps g's signs on
// its zeros: equal as numbers); the density channel keeps the raw value.
// (A NaN density is listed: the gradient kernel then writes what it always wrote for it.)
namespace nfx {
namespace geo {
struct HasDensity {
    const float* sigma;
    float4* out;
    __device__ bool operator()(long long r) const { return !(sigma[r] <= 0.f); }
    __device__ void visit(long long r, bool on) const {
        if (!on) out[r] = make_float4(-0.f, -0.f, -0.f, sigma[r]);
    }
};
}  // namespace geo
}  // namespace nfx
extern "C" int nfx_launch_select_density(const float* sigma, long long n_pts, float* out, void* list_ws, hipStream_t st) {
    return nfx::rowsel::build(nfx::geo::HasDensity{sigma, (float4*)out}, n_pts, list_ws, st);
}

extern "C" int nfx_launch_nerf_sigma_geo(const float* rayo, const float* rayd, const float* z, long long n_pts,
                                         int n_samples, const void* blob, float* out, int max_blocks, hipStream_t st) {
    using namespace nfx;
    if (n_pts <= 0) return 0;
    const long long tiles = (n_pts + 255) / 256;
    const int grid = (int)(tiles < max_blocks ? tiles : max_blocks);
    constexpr int lds = 2 * kSlotBytes + nerf::kGeoWSig * 4;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(geo::nerf_sigma_geo_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(geo::nerf_sigma_geo_kernel, dim3(grid), dim3(512), lds, st, rayo, rayd, z, n_pts, n_samples,
                       (const char*)blob, out);
    return (int)hipGetLastError();
}
