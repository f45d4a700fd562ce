// nerf_sigma_x3_pipe.hip — the density-only fp32-class kernel (nerf_geom_x3.hip:nerf_sigma_x3_kernel<false>) with the
// serialisations of mlp_x3.hpp:tile removed, the way nerf_mlp_v6.hip removed them from the bf16 forward kernel.
// Same geometry (4 waves x 32 points, activations as x3::Pair in registers), same GEOM blob ([hi fragments | lo fragments
// | floats] of pack_nerf_geom_weights(prec = 'fp32')), same arithmetic in the same order — every accumulator starts from
// its bias and takes, per k-step in ascending order, a_lo b_hi, a_hi b_lo, a_hi b_hi; ReLU by fmed3; x3::split — so the
// densities are bit-identical (tests/test_gpu_sigma_x3_pipelined.py).  The schedule:
//   * two accumulator sets: the epilogue of tile K-1 (fmed3 + split into the output pairs) is issued in pieces between
//     the MFMAs of tile K, and tile K+1's bias goes to the set it frees;
//   * the A pairs run kPreA k-steps ahead of their MFMAs in ONE four-pair buffer that carries across tiles (every tile
//     has a multiple of four k-steps): the last kPreA k-steps of tile K read the head of chunk K+1;
//   * the weights go global -> LDS by LDS-DMA (lds_dma.hpp, one statement per chunk half) into a ring of three
//     [hi | lo] slots, chunk K in slot K % 3; chunk K+2 is issued at the start of tile K and awaited (vmcnt(0)) at its end.
// The sequence is the 64 encoder chunks, the sigma tile and one IDLE position (66 = 3 x 22): nothing is fetched or
// multiplied there; it is the top of the point-tile loop, where chunk 1 of the pass is issued over the sigma tile's slot
// and the next points' positional encoding runs while it lands.
// What is NOT carried over from nerf_mlp_v6.hip: the bare s_barrier.  Three slots leave fetch distance 2, so the DMA over a
// slot is issued directly behind the barrier that ends the tile which read it; a bare s_barrier does not order a wave's
// outstanding LDS reads before another wave's DMA, lgkmcnt(0) in front of it does (the reads still in flight there are
// the next tile's first A pairs, issued three k-steps earlier).  tests/test_cpu_sigma_x3_ring.py restates the protocol.
#include "mlp_x3.hpp"
#include "lds_dma.hpp"
#include "nerf_geom_layout.hpp"
#include "nerf_points.hpp"
#include "launchers.hpp"

namespace nfx {
namespace geo3p {

using x3::Pair;
constexpr int kNW = x3::kNW;
constexpr int kRows = kNW * 32;
constexpr int kRing = 3;      // [hi | lo] slots
constexpr int kDist = 2;      // chunk K + kDist is issued at the start of tile K
constexpr int kPreA = 3;      // A pairs in flight ahead of their MFMAs
constexpr int kABuf = kPreA + 1;
constexpr int kNChunks = 65;  // 64 encoder chunks + the sigma tile
constexpr int kSeq = 66;      // ... + one idle position: a multiple of the ring
constexpr int kLds = kRing * x3::kSlot + nerf::kGeoFloats * 4;
static_assert(kSeq % kRing == 0, "the chunk sequence wraps on the ring");
static_assert(kLds <= 160 * 1024, "LDS");

constexpr int slot_of(int k) { return k % kRing; }
// k-steps a tile multiplies = fragments fetched per chunk half (layer 0 and layer 5 are padded to 8 / 24 in the blob)
constexpr int used_frags(int k) { return k < 8 ? 4 : k < 40 ? 16 : k < 48 ? 20 : 16; }
constexpr int bias_of(int k) { return k < 64 ? 32 * k : nerf::kGeoBiasSig; }
static_assert(used_frags(0) % kABuf == 0 && used_frags(8) % kABuf == 0 && used_frags(40) % kABuf == 0,
              "the A-pair buffer carries across tiles");

struct Ctx {
    char* smem;
    const char* blob;
    unsigned smem_lds;   // LDS byte address of smem (for M0)
    int wave;            // wave-uniform
    int lane;
};

template <int K>
__device__ __forceinline__ void dma_chunk(const Ctx& cx) {
    constexpr int n = used_frags(K) / kNW;      // 1-KiB pieces per wave and chunk half: 1 | 4 | 5
    unsigned long long base = reinterpret_cast<unsigned long long>(cx.blob);
    unsigned lds = cx.smem_lds;
    asm volatile("" : "+s"(base), "+s"(lds));   // per tile, as an integer: keeps the piece addresses out of the loop preheader
    const char* g = reinterpret_cast<const char*>(base) + (size_t)nerf::chunk_frag_offset(K) * kFragBytes + cx.wave * (n * 1024);
    const unsigned l = lds + slot_of(K) * x3::kSlot + cx.wave * (n * 1024);
    lds_dma_pieces<n>(cx.lane * 16, g, l);
    lds_dma_pieces<n>(cx.lane * 16, g + nerf::kGeoWeightBytes, l + kSlotBytes);
}

// A pair E of tile K's stream: k-step E of chunk K, or (E >= the tile's k-steps) the head of chunk K + 1
template <int K, int E>
__device__ __forceinline__ void read_a(const Ctx& cx, Pair (&ab)[kABuf]) {
    constexpr int KS = used_frags(K);
    constexpr int C = E < KS ? K : K + 1, F = E < KS ? E : E - KS;
    if constexpr (C < kNChunks) {
        const char* f = cx.smem + slot_of(C) * x3::kSlot + F * kFragBytes + cx.lane * 16;
        ab[E % kABuf].hi = *reinterpret_cast<const bf16x8*>(f);
        ab[E % kABuf].lo = *reinterpret_cast<const bf16x8*>(f + kSlotBytes);
    }
}

__device__ __forceinline__ void bias_to_acc(const float* bias_tile, int lane, f32x16& acc) {
    const float* bt = bias_tile + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(bt + 8 * g);
        acc[4 * g + 0] = v[0];
        acc[4 * g + 1] = v[1];
        acc[4 * g + 2] = v[2];
        acc[4 * g + 3] = v[3];
    }
}

// x3::acc_to_pair<true> on two neighbouring values: relu by fmed3, hi = bf16(v), lo = bf16(v - hi)
__device__ __forceinline__ void relu_split2(float v0, float v1, Pair& dst, int j) {
    v0 = __builtin_amdgcn_fmed3f(v0, 0.0f, __builtin_inff());
    v1 = __builtin_amdgcn_fmed3f(v1, 0.0f, __builtin_inff());
    const f32x2 v = {v0, v1};
    const bf16x2 hi = __builtin_convertvector(v, bf16x2);
    const f32x2 back = __builtin_convertvector(hi, f32x2);
    const bf16x2 lo = __builtin_convertvector(v - back, bf16x2);
    dst.hi[j] = hi[0];
    dst.hi[j + 1] = hi[1];
    dst.lo[j] = lo[0];
    dst.lo[j + 1] = lo[1];
}

struct EpiPair {    // accumulator rows 0..7 -> lo8, 8..15 -> hi8 (x3::acc_to_pair)
    const f32x16& acc;
    Pair& lo8;
    Pair& hi8;
    template <int R0, int R1>
    __device__ __forceinline__ void run() {
#pragma unroll
        for (int r = R0; r < R1; r += 2) {
            if (r < 8) relu_split2(acc[r], acc[r + 1], lo8, r);
            else relu_split2(acc[r], acc[r + 1], hi8, r - 8);
        }
    }
};
struct EpiNone {
    template <int R0, int R1>
    __device__ __forceinline__ void run() {}
};

// Tile K.  On entry `acc` holds the tile's bias and `ab` its first kPreA A pairs; on exit `acc_next` / `ab` hold the same
// for tile K + 1.  `prev`: the pending epilogue of tile K - 1 (its accumulators are `acc_next`).
template <int K, int KS1, int KS2, int KS1A, int KS2A, typename Epi>
__device__ __forceinline__ void tile(const Ctx& cx, const float* fl, const Pair (&b1)[KS1A], const Pair (&b2)[KS2A],
                                     f32x16& acc, f32x16& acc_next, Pair (&ab)[kABuf], Epi&& prev) {
    constexpr int KS = KS1 + KS2;
    static_assert(KS == used_frags(K), "k-steps of the chunk");
    constexpr int PIECES = KS >= 16 ? 8 : 4;
    constexpr int SP = PIECES < KS ? PIECES : KS - 1;   // k-step after which the previous tile's epilogue is complete
    constexpr int K2 = (K + kDist) % kSeq;              // 63 -> the idle position: nothing; 64 -> chunk 0 of the next pass
    if constexpr (K2 < kNChunks) dma_chunk<K2>(cx);
    static_for<0, KS>([&](auto S) {
        constexpr int s = decltype(S)::value;
        read_a<K, s + kPreA>(cx, ab);
        const Pair& a = ab[s % kABuf];
        const Pair& b = s < KS1 ? b1[s < KS1 ? s : 0] : b2[s >= KS1 ? s - KS1 : 0];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);   // small terms first
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
        if constexpr (s < PIECES) prev.template run<16 * s / PIECES, 16 * (s + 1) / PIECES>();
        if constexpr (s == SP && K + 1 < kNChunks) bias_to_acc(fl + bias_of(K + 1), cx.lane, acc_next);
    });
    // chunk K + 2 has landed, and no read of chunk K is outstanding when the next tile issues its DMA over a slot
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// A Dense layer of 8 tiles from chunk K0, outputs to bout; `prev0` = the pending epilogue of tile K0 - 1.  On return
// the last tile's epilogue is pending (accs[1] -> bout[14], bout[15]).
template <int K0, int KS1, int KS2, int KS1A, int KS2A, typename Epi0>
__device__ __forceinline__ void layer(const Ctx& cx, const float* fl, const Pair (&b1)[KS1A], const Pair (&b2)[KS2A],
                                      Pair (&bout)[16], f32x16 (&accs)[2], Pair (&ab)[kABuf], Epi0&& prev0) {
    static_for<0, 8>([&](auto T) {
        constexpr int t = decltype(T)::value;
        constexpr int K = K0 + t;
        if constexpr (t == 0) {
            tile<K, KS1, KS2>(cx, fl, b1, b2, accs[K & 1], accs[(K + 1) & 1], ab, prev0);
        } else {
            EpiPair e{accs[(K - 1) & 1], bout[2 * (t - 1)], bout[2 * (t - 1) + 1]};
            tile<K, KS1, KS2>(cx, fl, b1, b2, accs[K & 1], accs[(K + 1) & 1], ab, e);
        }
    });
}

// The points of the launch and where their densities go: nerf_points.hpp, as in nerf_sigma_x3_kernel<false>.
__global__ __launch_bounds__(kNW * 64, 1) void nerf_sigma_x3_pipe_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float* __restrict__ out, const int* __restrict__ list,
    const int* __restrict__ count, int list_stride, int last_sample) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace nerf;
    const geo::Points pts{rayo, rayd, zbuf, n_pts, n_samples, list, count, list_stride, last_sample};
    if (!pts.counted(kRows, n_pts)) return;      // no tile for this workgroup: before the weight stream
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    float* fl = reinterpret_cast<float*>(smem + kRing * x3::kSlot);
    {
        const float* src = reinterpret_cast<const float*>(blob + 2 * (size_t)kGeoWeightBytes);
        for (int i = tid; i < kGeoFloats; i += kNW * 64) fl[i] = src[i];
    }
    typedef __attribute__((address_space(3))) char lds_char;
    const Ctx cx{smem, blob, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_char*)smem),
                 __builtin_amdgcn_readfirstlane(wave), lane};
    dma_chunk<0>(cx);
    const long long n_tiles = (n_pts + kRows - 1) / kRows;
    for (long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        // ------------------------------------------------------------------ the idle position of the sequence
        dma_chunk<1>(cx);     // over the sigma tile's slot: behind the barrier that ended it
        const long long row = tl * kRows + wave * 32 + p;
        const bool valid = row < n_pts;
        const long long mm = pts.sample(row, n_pts);
        float x[3];
        pts.position(mm, x);
        Pair pe[4];
        x3::posenc_pair<10>(x, h, pe);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // chunks 0 and 1 (and the floats) are in
        f32x16 accs[2];
        Pair ab[kABuf];
        bias_to_acc(fl, lane, accs[0]);
        static_for<0, kPreA>([&](auto E) { read_a<0, decltype(E)::value>(cx, ab); });
        // ------------------------------------------------------------------ chunk K: L0 0-7, L1-4 8-39, L5 40-47, L6-7 48-63, sigma 64
        Pair ha[16], hb[16];
        auto pend = [&](Pair& lo8, Pair& hi8) { return EpiPair{accs[1], lo8, hi8}; };
        layer<0, 4, 0>(cx, fl, pe, pe, ha, accs, ab, EpiNone{});
        layer<8, 16, 0>(cx, fl, ha, pe, hb, accs, ab, pend(ha[14], ha[15]));
        layer<16, 16, 0>(cx, fl, hb, pe, ha, accs, ab, pend(hb[14], hb[15]));
        layer<24, 16, 0>(cx, fl, ha, pe, hb, accs, ab, pend(ha[14], ha[15]));
        layer<32, 16, 0>(cx, fl, hb, pe, ha, accs, ab, pend(hb[14], hb[15]));
        layer<40, 16, 4>(cx, fl, ha, pe, hb, accs, ab, pend(ha[14], ha[15]));
        layer<48, 16, 0>(cx, fl, hb, pe, ha, accs, ab, pend(hb[14], hb[15]));
        layer<56, 16, 0>(cx, fl, ha, pe, hb, accs, ab, pend(ha[14], ha[15]));
        // the sigma tile (-> accs[0]); pending: the last tile of enc[7] (accs[1] -> hb[14], hb[15], complete after k-step 7)
        tile<64, 16, 0>(cx, fl, hb, pe, accs[0], accs[1], ab, pend(hb[14], hb[15]));
        const float sigma = accs[0][0];   // row 0 of the tile, on the h = 0 lanes
        if (valid && h == 0) pts.store_sigma(out, row, mm, sigma);
    }
}

}  // namespace geo3p
}  // namespace nfx

// pts.n_pts sizes the grid (nerf_points.hpp)
extern "C" int nfx_launch_nerf_sigma_x3_pipe(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks,
                                             hipStream_t st) {
    using namespace nfx::geo3p;
    if (pts->n_pts <= 0) return 0;
    const long long tiles = (pts->n_pts + kRows - 1) / kRows;
    const int grid = (int)(tiles < max_blocks ? tiles : max_blocks);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(nerf_sigma_x3_pipe_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nerf_sigma_x3_pipe_kernel, dim3(grid), dim3(kNW * 64), kLds, st, pts->rayo, pts->rayd, pts->z, pts->n_pts,
                       pts->n_samples, (const char*)blob, out, pts->list, pts->count, pts->list_stride, pts->last_sample);
    return (int)hipGetLastError();
}
