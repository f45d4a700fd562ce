// nerf_sigma_v6.hip — density only, in the dataflow of the headline render kernel (round 6).
//   sigma_raw(x) = sigma_out(enc(posenc(x)))   (eval_sigma_mlp, geometry_from_nerf.py:322-350, before its relu)
// nerf_sigma_geo_kernel (nerf_geom.hip: two workgroups of eight waves per CU, register-staged weight stream) runs the 65
// encoder + sigma tiles at 1.11 PFLOP/s; the render kernel (nerf_mlp_v6.hip, DMA = 1: one wave per SIMD, 64 points per
// wave, LDS-DMA weight ring with counted vmcnt, the epilogue of tile i-1 under the MFMAs of tile i) sustains 1.45 on the
// same layers.  This translation unit is that kernel's tile / layer machinery (nerf_v6_engine.hpp, Seq::Geom) over the GEOM
// blob: chunks 0..63 are the render blob's encoder chunks byte for byte, chunk 64 is the sigma tile, and chunk 65 — the first
// reverse-sweep chunk of the blob — is fetched into the ring and not multiplied, so that the 66-chunk sequence wraps on
// the 6-slot ring.  Same MFMAs on the same operands as every other density kernel: bit-identical sigma
// (tests/test_gpu_nerf.py::test_sigma_only_kernel_is_the_full_kernel_s_density).
#include "nerf_v6_engine.hpp"
#include "nerf_geom_layout.hpp"
#include "launchers.hpp"

namespace nfx {
namespace v6 {

constexpr int kDma = 1;
constexpr Seq kSeq = Seq::Geom;

static_assert(seq_frags<kSeq>(64) == 16 && seq_frags<kSeq>(65) == 16 && used_frags<kSeq>(64) == 16 && used_frags<kSeq>(65) == 16,
              "the sigma tile and the idle chunk are 16-fragment chunks");
static_assert(nerf::kGeoFwdFrags == seq_frag_offset<kSeq>(65) && nerf::kGeoFrags >= seq_frag_offset<kSeq>(66),
              "GEOM blob: sigma tile at chunk 64, a whole chunk behind it");
static_assert(nerf::kGeoFloats <= nerf::kBiasFloats, "the float section fits the render kernel's bias area");

// Where a lane's sample comes from: position m of a kernel's n_pts points is the flat sample src(m) — the point
// rayo[i / S] + rayd[i / S] z[i] of sample i, whose density goes to out[i].  A lane past the end of the points recomputes the
// last one and stores nothing; what it keeps until the store (Dst) is its position m, or the listed sample and -1 past the end.
// (One rule for both — the sample, or -1 — costs the every-sample kernel two selects per tile and four registers.)
struct EverySample {
    typedef long long Dst;
    __device__ __forceinline__ long long operator()(long long m) const { return m; }
    static __device__ __forceinline__ Dst dst(long long m, long long, long long) { return m; }
    static __device__ __forceinline__ bool stores(Dst d, long long n_pts) { return d < n_pts; }
};
struct ListedSample {
    typedef int Dst;
    const int* __restrict__ list;
    __device__ __forceinline__ long long operator()(long long m) const { return list[m]; }
    static __device__ __forceinline__ Dst dst(long long m, long long mm, long long n_pts) { return m < n_pts ? (int)mm : -1; }
    static __device__ __forceinline__ bool stores(Dst d, long long) { return d >= 0; }
};

template <typename Src>
__device__ __forceinline__ void nerf_sigma_v6_body(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float* __restrict__ out, Src src) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace nerf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    float* fl = floats_of<kDma, kSeq>(smem);
    Acc accs[2];
    Pre pre;
    Regs rg;
    const Ctx cx = prologue<kDma, kSeq>(smem, blob, kGeoWeightBytes, kGeoFloats, tid, lane, rg, pre, accs[0]);
    const long long n_tiles = (n_pts + kTilePts - 1) / kTilePts;
    for (long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        bf16x8 pe[4][kCT];
        typename Src::Dst dst[kCT];
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
            const long long m = tl * kTilePts + wave * (32 * kCT) + c * 32 + p;
            const long long mm = src(m < n_pts ? m : n_pts - 1);
            const long long ray = mm / n_samples;
            dst[c] = Src::dst(m, mm, n_pts);
            const float zz = zbuf[mm];
            float x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = rayo[ray * 3 + k] + rayd[ray * 3 + k] * zz;
            posenc<10, kCT>(x, h, c, pe);
        }
        bf16x8 ha[16][kCT], hb[16][kCT];
        float sigma[kCT];
        auto pend = [&](const Acc& a, bf16x8(&lo)[kCT], bf16x8(&hi)[kCT]) { return EpiB<true>{a, lo, hi}; };
        // chunk index K: L0 0-7, L1-4 8-39, L5 40-47, L6-7 48-63, sigma 64, idle 65; tile K accumulates in accs[K & 1]
        layer<0, 4, 0, 8, true, kDma, kSeq>(cx, rg, fl, fl + 256 * 1, pe, pe, ha, accs, pre, EpiNone{});
        layer<8, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 1, fl + 256 * 2, ha, pe, hb, accs, pre, pend(accs[1], ha[14], ha[15]));
        layer<16, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 2, fl + 256 * 3, hb, pe, ha, accs, pre, pend(accs[1], hb[14], hb[15]));
        layer<24, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 3, fl + 256 * 4, ha, pe, hb, accs, pre, pend(accs[1], ha[14], ha[15]));
        layer<32, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 4, fl + 256 * 5, hb, pe, ha, accs, pre, pend(accs[1], hb[14], hb[15]));
        layer<40, 16, 4, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 5, fl + 256 * 6, ha, pe, hb, accs, pre, pend(accs[1], ha[14], ha[15]));
        layer<48, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 6, fl + 256 * 7, hb, pe, ha, accs, pre, pend(accs[1], hb[14], hb[15]));
        layer<56, 16, 0, 8, true, kDma, kSeq>(cx, rg, fl + 256 * 7, fl + kGeoBiasSig, ha, pe, hb, accs, pre, pend(accs[1], ha[14], ha[15]));
        // the sigma tile (K = 64 -> accs[0]); pending: the last tile of enc[7] (accs[1] -> hb[14], hb[15]); the bias handed to
        // the idle tile's accumulators is never used
        tile<64, 16, 0, kDma, kSeq>(cx, rg, fl + kGeoBiasSig, hb, pe, accs[0], accs[1], pre, pend(accs[1], hb[14], hb[15]));
        // the idle tile (K = 65 -> accs[1]: A fragments read, no MFMA): chunk 2 of the next pass is fetched, sigma leaves
        // accs[0], accs[0] gets the bias of L0's first tile
        {
            EpiSigma es{accs[0], sigma};
            tile<65, 16, 0, kDma, kSeq, /* IDLE */ true>(cx, rg, fl, hb, pe, accs[1], accs[0], pre, es);
        }
        if (h == 0) {
#pragma unroll
            for (int c = 0; c < kCT; ++c)
                if (Src::stores(dst[c], n_pts)) out[dst[c]] = sigma[c];
        }
    }
}

// The density of every flat sample 0 .. n_pts.
__global__ __launch_bounds__(kNW * 64, 1) void nerf_sigma_v6_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float* __restrict__ out) {
    nerf_sigma_v6_body(rayo, rayd, zbuf, n_pts, n_samples, blob, out, EverySample{});
}

// The same over the flat sample indices list[0 .. *count) (list and count in device memory: the number of listed samples
// never visits the host); a persistent loop over the list's tiles.  Every point goes through the same posenc, tiles and MFMAs
// as in nerf_sigma_v6_kernel, so a listed sample gets its bits (the occupancy-grid march).
__global__ __launch_bounds__(kNW * 64, 1) void nerf_sigma_v6_list_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, int n_samples,
    const char* __restrict__ blob, float* __restrict__ out, const int* __restrict__ list, const int* __restrict__ count) {
    const long long n_pts = *count;
    if ((long long)blockIdx.x * kTilePts >= n_pts) return;      // no tile for this workgroup: before the weight stream
    nerf_sigma_v6_body(rayo, rayd, zbuf, n_pts, n_samples, blob, out, ListedSample{list});
}

}  // namespace v6
}  // namespace nfx

extern "C" int nfx_launch_nerf_sigma_v6(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples,
                                        const void* blob, float* out, int max_blocks, hipStream_t stream) {
    using namespace nfx::v6;
    if (n_pts <= 0) return 0;
    return launch_tiles(nerf_sigma_v6_kernel, lds_of<kDma, kSeq>, n_pts, max_blocks, stream, rayo, rayd, z, n_pts, n_samples,
                        (const char*)blob, out);
}

// list / count: device memory; capacity = the list's length (sizes the grid; the kernel reads the real count on the device)
extern "C" int nfx_launch_nerf_sigma_v6_list(const float* rayo, const float* rayd, const float* z, long long capacity,
                                             int n_samples, const void* blob, float* out, const int* list, const int* count,
                                             int max_blocks, hipStream_t stream) {
    using namespace nfx::v6;
    if (capacity <= 0) return 0;
    return launch_tiles(nerf_sigma_v6_list_kernel, lds_of<kDma, kSeq>, capacity, max_blocks, stream, rayo, rayd, z, n_samples,
                        (const char*)blob, out, list, count);
}
