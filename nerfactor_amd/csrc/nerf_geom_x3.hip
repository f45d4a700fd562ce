// nerf_geom_x3.hip — NFX_PREC_FP32 of nerf_geom.hip: density and its spatial gradient at sample points with fp32-class
// arithmetic on the bf16 matrix pipe (mlp_x3.hpp: hi / lo operand pairs, three MFMAs per product) — forward
// activations, the back-propagated dZ and both weight orientations.  The schedule is nerf_geom_body.hpp's; the blob is
// nerf_geom_layout.hpp's chunk sequence twice, [hi fragments | lo fragments | floats], the sigma_out kernel among the
// floats in full fp32 (geometry_from_nerf.py:280-297, 322-350: the reference differentiates in fp32).  Register budget:
// two 256-feature activations as pairs are 256 VGPRs, with masks, staging and accumulators the gradient kernel spills
// 82 dwords per lane to scratch — accepted for a precision option (the bf16 kernel is the fast path).
#include "mlp_x3.hpp"
#include "nerf_geom_body.hpp"
#include "launchers.hpp"

namespace nfx {
namespace geo3 {

using x3::Pair;
constexpr int kNW = x3::kNW;
constexpr int kRows = kNW * 32;

// hi / lo pairs: three MFMAs per product, small terms first (x3::tile); every tile starts from a bias tile in LDS
struct X3 {
    using Op = Pair;
    using Stream = x3::Stream;
    static constexpr int kNW = x3::kNW;
    static constexpr size_t kFloatOffset = 2 * (size_t)nerf::kGeoWeightBytes;
    static constexpr int kZeroTile = nerf::kGeoFloats;          // 32 zero floats: the "bias" of the reverse-sweep tiles
    template <bool>
    static constexpr int n_floats() { return nerf::kGeoFloats; }
    template <bool>
    static constexpr bool kMasks = true;   // also where nothing reads them: relu_bits16 is opaque, and the density kernel's registers are settled with it
    __device__ __forceinline__ static float* floats(char* smem) { return reinterpret_cast<float*>(smem + 2 * x3::kSlot); }
    template <bool GRAD>
    __device__ __forceinline__ static void open(x3::Stream& st, char* smem, const char* blob, float* fl, int tid) {
        if (tid < 32) fl[kZeroTile + tid] = 0.f;
        st.base = reinterpret_cast<const u32x4*>(blob);
        st.end = reinterpret_cast<const u32x4*>(blob + (GRAD ? (size_t)nerf::kGeoWeightBytes : (size_t)nerf::kGeoFwdFrags * kFragBytes));
        st.ghi = st.base;
        st.lo_off = nerf::kGeoWeightBytes / 16;
        st.ring = smem;
        x3::prologue<nerf::kNL0>(st, tid);
    }
    __device__ __forceinline__ static void posenc(const float (&x)[3], int h, Pair (&pe)[4]) { x3::posenc_pair<10>(x, h, pe); }
    __device__ __forceinline__ static void relu_to(const f32x16& acc, Pair& lo8, Pair& hi8) { x3::acc_to_pair<true>(acc, lo8, hi8); }
    __device__ __forceinline__ static void put(Pair (&dst)[16], int t, int r, float v) {
        __bf16 a, b;
        x3::split(v, a, b);
        dst[2 * t + (r >> 3)].hi[r & 7] = a;
        dst[2 * t + (r >> 3)].lo[r & 7] = b;
    }
    __device__ __forceinline__ static float sigma(const f32x16& acc, int) { return acc[0]; }
    template <int KS1, int KS2, int NL, int KS1A, int KS2A>
    __device__ __forceinline__ static void tile(x3::Stream& st, int tid, const float* bias, const Pair (&b1)[KS1A],
                                                const Pair (&b2)[KS2A], f32x16& acc) {
        x3::tile<KS1, KS2, NL>(st, tid, bias, b1, b2, acc);
    }
    template <int NL>
    __device__ __forceinline__ static void tile_zero(x3::Stream& st, int tid, const float* fl, const Pair (&dz)[16], f32x16& acc) {
        x3::tile<16, 0, NL>(st, tid, fl + kZeroTile, dz, dz, acc);
    }
    // the sum is added after the chain: the tile's own small terms meet each other first
    template <int NL>
    __device__ __forceinline__ static void tile_add(x3::Stream& st, int tid, const float* fl, const Pair (&dz)[16], f32x16& sum) {
        f32x16 acc;
        tile_zero<NL>(st, tid, fl, dz, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[r] += acc[r];
    }
};

// list != nullptr is a run-time test here (nerf_points.hpp); GRAD has no last-sample form
template <bool GRAD>
__global__ __launch_bounds__(kNW * 64, 1) void nerf_sigma_x3_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float* __restrict__ out, const int* __restrict__ list,
    const int* __restrict__ count, int list_stride, int last_sample) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const geo::Points pts{rayo, rayd, zbuf, n_pts, n_samples, list, count, list_stride, GRAD ? 0 : last_sample};
    if constexpr (!GRAD) {
        geo::nerf_sigma_body<X3>(pts, blob, out, smem);
    } else {
        // The tile loop stands in the kernel itself: behind a function the compiler needs 1192 instead of 328 bytes of scratch
        // (nerf_geom_body.hpp, profiles/geom_body/code_objects.txt).  The lines from counted() to sample() are
        // nerf_sigma_body()'s and change together with them.
        long long n;
        if (!pts.counted(kRows, n)) return;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
        x3::Stream st;
        const float* fl = geo::start<X3, true>(st, smem, blob, tid);
        const long long n_tiles = (n + kRows - 1) / kRows;
        for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
            const long long row = tile * kRows + wave * 32 + p;
            const bool valid = row < n;
            const long long mm = pts.sample(row, n);
            const float4 ns = geo::grad_point<X3>(st, tid, fl, pts, mm);
            if (valid && h == 0) reinterpret_cast<float4*>(out)[pts.grad_row(row, mm)] = ns;
        }
    }
}

constexpr int kLds = 2 * x3::kSlot + (nerf::kGeoFloats + 32) * 4;   // two [hi | lo] slots, the floats, the zero tile

template <bool GRAD>
static int launch(const geo::Points& pts, const void* blob, float* out, int max_blocks, hipStream_t st) {
    if (GRAD && pts.last_sample) return (int)hipErrorInvalidValue;   // the gradient has the every-sample and the list form only
    if (pts.n_pts <= 0) return 0;
    const long long tiles = (pts.n_pts + kRows - 1) / kRows;
    const int grid = (int)(tiles < max_blocks ? tiles : max_blocks);
    auto k = nerf_sigma_x3_kernel<GRAD>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kNW * 64), kLds, st, pts.rayo, pts.rayd, pts.z, pts.n_pts, pts.n_samples,
                       (const char*)blob, out, pts.list, pts.count, pts.list_stride, pts.last_sample);
    return (int)hipGetLastError();
}

}  // namespace geo3
}  // namespace nfx

// (normal, sigma) rows of every sample, or of the listed ones (nfx_nerf_sigma_grad_rows)
extern "C" int nfx_launch_nerf_sigma_grad_x3(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks,
                                             hipStream_t st) {
    return nfx::geo3::launch<true>(*pts, blob, out, max_blocks, st);
}
// density only: the pipelined kernel (nerf_sigma_x3_pipe.hip) unless option sigma_x3_variant = 0; bit-identical
extern "C" int nfx_launch_nerf_sigma_x3(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks, hipStream_t st) {
    if (nfx_option_int("sigma_x3_variant", 1) != 0) return nfx_launch_nerf_sigma_x3_pipe(pts, blob, out, max_blocks, st);
    return nfx::geo3::launch<false>(*pts, blob, out, max_blocks, st);
}
