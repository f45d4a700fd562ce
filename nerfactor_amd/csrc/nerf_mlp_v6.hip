// nerf_mlp_v6.hip — variant 6 of the fused NeRF MLP: variant 5 (one wave per SIMD, 64 points per wave, epilogue of
// tile i-1 in the shadow of tile i's MFMAs) with the serialisation at the tile boundary removed.  The r01 ablation of
// variant 5 (profiles/r01/ablation_variant5.log) showed its non-MFMA stream alone takes longer than the MFMAs:
// ds_write -> s_waitcnt lgkmcnt(0) -> s_barrier -> bias/A ds_read -> first MFMA is ~300 dead cycles per tile.  Here:
//   * 3-slot LDS ring, chunk k lives in slot k % 3 (78 = 3 x 26 chunks): chunk k+2 is fetched global -> VGPR at the
//     start of tile k and written to its slot at the END of the tile; nobody waits for those writes (they are a full
//     tile old when first read),
//   * the first three A fragments and the bias of tile k+1 are read BEFORE the end-of-tile barrier (chunk k+1 has been
//     in LDS for a whole tile), so their latency overlaps the tail MFMAs and the barrier,
//   * the barrier is a bare s_barrier (no lgkmcnt(0) drain).
// Same blob, bit-identical results to variants 0-5.
//
// Three weight-stream modes of the same kernel (template parameter DMA), all built in MFMA VGPR form (build.py):
//   DMA = 0  variant 6   register-staged as described above;
//   DMA = 1  variant 7   THE DEFAULT: LDS-DMA (global_load_lds_dwordx4) into a 6-slot ring, chunk k+3 issued at the
//                        start of tile k, counted s_waitcnt vmcnt before the barrier — no staging VGPRs, no ds_write;
//   DMA = 2  variant 8   register-staged with two staging sets (chunk k+3 fetched during tile k, stored a tile later).
// The r01 experiment switches (second bias read group, A-prefetch depth, epilogue start offset, DMA fetch distance,
// DMA pieces spread over the k-steps) were all measured and left at the values now hard-wired — profiles/HISTORY.md
// section 2 has the numbers.  The cycle-stamp build, its experiment masks and the ablation instantiations that produced
// the r01-r03 measurements of profiles/HISTORY.md sections 2 / 2d left this file in r04 (git history: fdbd16f holds them),
// the tile machinery's ablation mask when it moved to the engine header: the shipped translation unit is the product kernel.
//
// The tile / layer machinery (ring, slot maps, tile, layer, the prologue before the tile loop, the launch) is
// nerf_v6_engine.hpp, shared with the density kernels of nerf_sigma_v6.hip.  This file holds the render body over the packed
// blob (Seq::Packed, 78 tiles) and over the render blob of nerf_fold.hip (Seq::Render, 70 tiles: v6::fold::), and its launchers.
#include "nerf_v6_engine.hpp"
#include "launchers.hpp"

namespace nfx {
namespace v6 {

// What a lane's encoders take of its point: depth, ray direction, ray origin.
struct PointIn {
    float zz, d[3], o[3];
};

template <int DMA, Seq S>
__device__ __forceinline__ void nerf_mlp_bf16_v6_body(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float4* __restrict__ out, unsigned* __restrict__ counter) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace nerf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    constexpr bool FOLD = S == Seq::Render;
    constexpr bool kAhead = DMA == 1;   // fetch the next point tile's inputs one tile ahead (below)
    float* bias_lds = floats_of<DMA, S>(smem);
    // The hand-out of point tiles (DMA == 1 with a counter; a null counter is the static walk tl, tl + gridDim.x, ...).  A
    // workgroup's first tile is blockIdx.x; every further one is gridDim.x + fetch_add(counter, 1), relaxed at agent scope: the
    // claim only numbers the tiles, no data passes between workgroups, so nothing is acquired or released.  Lane 0 of wave 0
    // claims, and the index reaches the other waves through ONE LDS word behind the blob's floats (launch_v6 asks for it):
    //   claim  the atomic of pass k is issued behind layer 0, beside the fetch-ahead loads (see there);
    //   write  its result goes to the word between the barriers of the last two tiles of pass k (behind the last tile of
    //          rgb_out[0], in front of rgb_out[1]), and wave 0 drains its LDS queue there (the tile barrier is a bare s_barrier).
    //          Not at the very end of the pass, where the fetched inputs are taken over: no barrier lies between there and the read;
    //   read   every wave reads the word at the top of pass k + 1, behind the barrier of pass k's last tile: it is the tile of
    //          pass k + 2, whose inputs pass k + 1 fetches.  The write of pass k + 1 lies behind the barriers of that pass's
    //          tiles 0 .. n - 2, which a wave reaches only after its read at the top of the pass (the value feeds the division
    //          there).  The first claim is made and written in front of the prologue's __syncthreads.
    // Depth: at the top of a pass the workgroup knows the tile it starts and the next one; behind layer 0 it claims one more.  So
    // it holds at most TWO claimed tiles it has not started, and a launch ends with at most two passes of one workgroup to wait for.
    // Exit: all four waves take the next index from the same word between the same two barriers, through readfirstlane, so
    // `tl < n_tiles` is the same in every wave of the workgroup: no wave leaves a barrier behind.  A workgroup claims once
    // in front of the loop and once per pass, two of them at or past n_tiles: the counter ends at n_tiles + gridDim.x.
    // (tests/test_cpu_nerf_handout.py walks this protocol under every order of the atomics.)
    bool handout = false;
    unsigned* const next_word = reinterpret_cast<unsigned*>(smem + lds_of<DMA, S>);
    if constexpr (kAhead) {
        handout = counter != nullptr;
        if (handout && tid == 0) *next_word = gridDim.x + __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    Acc accs[2];
    Pre pre;
    Regs rg;
    const Ctx cx = prologue<DMA, S>(smem, blob, FOLD ? nerf::fold::kWeightBytes : nerf::kWeightBytes, kBiasFloats, tid, lane, rg, pre,
                                    accs[0]);
    const long long n_tiles = (n_pts + kTilePts - 1) / kTilePts;
    // The front end: ONE point per lane.  Lanes p and p + 32 hold the points of column tile 0 and 1 at column p; lane (h, p)
    // fetches and encodes the point of column tile h, both slot sets of it, and trades the set of the other half with lane
    // p ^ 32 (mlp_engine.hpp: posenc_sets, exchange_sets).  A lane whose own point lies past n_pts takes point n_pts - 1, encodes
    // it and takes part in the exchange like every other lane: its partner may hold a valid point of the other column tile.
    const int partner = (lane ^ 32) << 2;
    // flat sample `mm` and ray `ray` of the lane's own point of point tile `tl`; a tile past the last one gives n_pts - 1
    auto own_point = [&](long long tl, long long& mm_of, long long& ray_of) {
        long long m[kCT];
        const int c = h;
        m[c] = tl * kTilePts + wave * (32 * kCT) + c * 32 + p;
        const long long mm = m[c] < n_pts ? m[c] : n_pts - 1;
        const long long ray = mm / n_samples;
        mm_of = mm;
        ray_of = ray;
    };
    auto fetch = [&](long long mm, long long ray, PointIn& in) {
        in.zz = zbuf[mm];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            in.d[k] = rayd[ray * 3 + k];
            in.o[k] = rayo[ray * 3 + k];
        }
    };
    // The seven values of the lane's point of the NEXT point tile of this workgroup (tl + gridDim.x) are fetched during the pass
    // and carried across the loop edge; where that tile does not exist every lane fetches point n_pts - 1 and nobody uses it.
    PointIn ahead;
    if constexpr (kAhead) {
        long long mm, ray;
        own_point(blockIdx.x, mm, ray);
        fetch(mm, ray, ahead);
    }
    const bool claims = handout && cx.wave == 0;   // wave-uniform
    for (long long tl = blockIdx.x; tl < n_tiles;) {
        bf16x8 pe[4][kCT], pv[2][kCT];
        long long m[kCT];
#pragma unroll
        for (int c = 0; c < kCT; ++c) m[c] = tl * kTilePts + wave * (32 * kCT) + c * 32 + p;
        long long nxt = 0;   // this workgroup's next point tile (the register-staged variants add the stride at the bottom, as ever)
        if constexpr (kAhead) {
            nxt = tl + gridDim.x;
            if (handout) nxt = (unsigned)__builtin_amdgcn_readfirstlane((int)*next_word);
        }
        // the division stays up here, outside the one basic block of the tiles; only the loads move (below)
        long long mm, ray;
        own_point(kAhead ? nxt : tl, mm, ray);
        PointIn in;
        if constexpr (kAhead) in = ahead;
        else fetch(mm, ray, in);
        {
            float x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = in.o[k] + in.d[k] * in.zz;
            bf16x8 e0[4], e1[4], w0[2], w1[2];
            posenc_sets<10>(x, e0, e1);
            posenc_sets<4>(in.d, w0, w1);
            exchange_sets(h, partner, e0, e1, pe, w0, w1, pv);
        }
        bf16x8 ha[16][kCT], hb[16][kCT], r0[8][kCT];
        float sigma[kCT];
        const float* bl = bias_lds + kBiasL0;
        auto pend = [&](auto relu_tag, const Acc& a, bf16x8(&lo)[kCT], bf16x8(&hi)[kCT]) {
            return EpiB<decltype(relu_tag)::value>{a, lo, hi};
        };
        using T = std::true_type;
        using F = std::false_type;
        unsigned got;   // wave 0, lane 0: the claim of this pass (an AccVGPR the compiler does not know to be in flight: below)
        // the claimed index to the LDS word, between the barriers of the pass's last two tiles (top of the function)
        auto publish = [&] {
            if constexpr (kAhead) {
                if (claims && lane == 0) {
                    // volatile like the tiles' barriers, so it stays behind them: `got` is not read before this statement
                    asm volatile("" : "+a"(got));
                    *next_word = gridDim.x + got;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            }
        };
        // chunk index K: L0 0-7, L1-4 8-39, L5 40-47, L6-7 48-63, bottleneck 64-71, sigma 72, rgb0 73-76, rgb1 77
        // (folded: sigma 64, rgb0 65-68, rgb1 69); tile K accumulates in accs[K & 1]
        layer<0, 4, 0, 8, true, DMA, S>(cx, rg, bl, bl + 256 * 1, pe, pe, ha, accs, pre, EpiNone{});
        if constexpr (kAhead) {
            // Issued HERE, behind the short tiles of layer 0: vmcnt counts these three loads and the weight pieces together, in
            // issue order, so the next counted wait of tile<> (end of tile 8) also waits for them — it is a full 16-k-step tile
            // away.  (The waits can only wait for more with older loads in flight: they stay correct.)  The empty statement
            // keeps the compiler from issuing the loads at the loop top, in front of tile 0's wait.
            // The claim of wave 0 is one more such load, and the same argument holds: a returning atomic counts in vmcnt in issue
            // order with the pieces, so behind it a counted wait of tile<> can only wait for more — and the wait that ends tile 8
            // leaves only that tile's own pieces in flight, so the claim has landed 60 tiles before publish() reads it.
            // Written as one statement with the result in an AccVGPR: given the builtin, the compiler parks the result in an
            // AccVGPR itself, behind an s_waitcnt vmcnt(0) right here that waits for the atomic and every piece in flight (the
            // VGPRs are full), and wraps the atomic in a wave reduction.  EXEC is 1 in the claiming wave and 0 in all others, the
            // static walk included: no branch splits the block of the tiles, and a wave with EXEC = 0 touches no memory.
            unsigned long long exec_saved;
            const unsigned claim_exec = __builtin_amdgcn_readfirstlane((unsigned)claims);   // a scalar register, by construction
            asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %2\n\ts_mov_b32 exec_hi, 0\n\t"
                         "global_atomic_add %0, %3, %4, %5 sc0\n\ts_mov_b64 exec, %1"
                         : "=&a"(got), "=&s"(exec_saved)
                         : "s"(claim_exec), "v"(0u), "a"(1u), "s"(counter)
                         : "memory");
            asm volatile("" : "+v"(mm), "+v"(ray));
            fetch(mm, ray, ahead);
        }
        layer<8, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 1, bl + 256 * 2, ha, pe, hb, accs, pre, pend(T{}, accs[1], ha[14], ha[15]));
        layer<16, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 2, bl + 256 * 3, hb, pe, ha, accs, pre, pend(T{}, accs[1], hb[14], hb[15]));
        layer<24, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 3, bl + 256 * 4, ha, pe, hb, accs, pre, pend(T{}, accs[1], ha[14], ha[15]));
        layer<32, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 4, bl + 256 * 5, hb, pe, ha, accs, pre, pend(T{}, accs[1], hb[14], hb[15]));
        layer<40, 16, 4, 8, true, DMA, S>(cx, rg, bl + 256 * 5, bl + 256 * 6, ha, pe, hb, accs, pre, pend(T{}, accs[1], ha[14], ha[15]));
        layer<48, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 6, bl + 256 * 7, hb, pe, ha, accs, pre, pend(T{}, accs[1], hb[14], hb[15]));
        if constexpr (FOLD) {
        // enc[7] -> hb; next tile = sigma (bias row 256 of the fused [bottleneck | sigma_out] matrix)
        layer<56, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 7, bias_lds + kBiasBott + 256, ha, pe, hb, accs, pre, pend(T{}, accs[1], ha[14], ha[15]));
        // sigma tile (K = 64 -> accs[0]): the unfolded kernel's tile 72 on the same operands; pending: the last tile of enc[7]
        // (accs[1] -> hb[14], hb[15], complete after k-step 8); next: folded rgb_out[0] tile 0
        tile<64, 16, 0, DMA, S>(cx, rg, bias_lds + kBiasRgb0, hb, pe, accs[0], accs[1], pre, pend(T{}, accs[1], hb[14], hb[15]));
        {   // folded rgb_out[0]: [enc[7] output, posenc(view)] -> 128 with W' = Wb W0a, b0' = bb W0a + b0 (nerf_fold.hip)
            EpiSigma es{accs[0], sigma};
            layer<65, 16, 2, 4, true, DMA, S>(cx, rg, bias_lds + kBiasRgb0, bias_lds + kBiasRgb1, hb, pv, r0, accs, pre, es);
        }
        publish();
        // rgb_out[1] (K = 69 -> accs[1]); pending: last rgb_out[0] tile (K = 68 -> accs[0]); next: L0 tile 0
        tile<69, 8, 0, DMA, S>(cx, rg, bl, r0, pe, accs[1], accs[0], pre, pend(T{}, accs[0], r0[6], r0[7]));
        } else {
        layer<56, 16, 0, 8, true, DMA, S>(cx, rg, bl + 256 * 7, bias_lds + kBiasBott, ha, pe, hb, accs, pre, pend(T{}, accs[1], ha[14], ha[15]));
        // bottleneck (no activation) hb -> ha; next tile = sigma (bias row 256 of the fused matrix)
        layer<64, 16, 0, 8, false, DMA, S>(cx, rg, bias_lds + kBiasBott, bias_lds + kBiasBott + 256, hb, pe, ha, accs, pre,
                                       pend(T{}, accs[1], hb[14], hb[15]));
        // sigma tile (K = 72 -> accs[0]); pending: last bottleneck tile (accs[1]); next: rgb_out[0] tile 0
        tile<72, 16, 0, DMA, S>(cx, rg, bias_lds + kBiasRgb0, hb, pe, accs[0], accs[1], pre, pend(F{}, accs[1], ha[14], ha[15]));
        {
            EpiSigma es{accs[0], sigma};
            layer<73, 16, 2, 4, true, DMA, S>(cx, rg, bias_lds + kBiasRgb0, bias_lds + kBiasRgb1, ha, pv, r0, accs, pre, es);
        }
        publish();
        // rgb_out[1] (K = 77 -> accs[1]); pending: last rgb_out[0] tile (K = 76 -> accs[0]); next: L0 tile 0
        tile<77, 8, 0, DMA, S>(cx, rg, bl, r0, pe, accs[1], accs[0], pre, pend(T{}, accs[0], r0[6], r0[7]));
        }
        if constexpr (kAhead) {
            // the fetched values are taken over in front of the stores: behind them the compiler's wait for the loads would
            // be a vmcnt(0) that also waits for the stores to be acknowledged
            asm volatile("" : "+v"(ahead.zz), "+v"(ahead.d[0]), "+v"(ahead.d[1]), "+v"(ahead.d[2]), "+v"(ahead.o[0]),
                         "+v"(ahead.o[1]), "+v"(ahead.o[2]));
        }
        if (h == 0) {
#pragma unroll
            for (int c = 0; c < kCT; ++c)
                if (m[c] < n_pts) out[m[c]] = make_float4(accs[1].v[c][0], accs[1].v[c][1], accs[1].v[c][2], sigma[c]);
        }
        tl = kAhead ? nxt : tl + gridDim.x;
    }
}

// (AB, always 0: the ablation mask the engine once took.  It stays a template argument of the two __global__ kernels alone,
//  so that they keep the names nerf_mlp_bf16_v6_kernel<0, DMA> that the profiles and the kernel-metadata tests know.)
template <int AB, int DMA>
__global__ __launch_bounds__(kNW * 64, 1) void nerf_mlp_bf16_v6_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float4* __restrict__ out, unsigned* __restrict__ counter) {
    nerf_mlp_bf16_v6_body<DMA, Seq::Packed>(rayo, rayd, zbuf, n_pts, n_samples, blob, out, counter);
}

namespace fold {   // over a render blob: 70 tiles
template <int AB, int DMA>
__global__ __launch_bounds__(kNW * 64, 1) void nerf_mlp_bf16_v6_kernel(
    const float* __restrict__ rayo, const float* __restrict__ rayd, const float* __restrict__ zbuf, long long n_pts,
    int n_samples, const char* __restrict__ blob, float4* __restrict__ out, unsigned* __restrict__ counter) {
    nerf_mlp_bf16_v6_body<DMA, Seq::Render>(rayo, rayd, zbuf, n_pts, n_samples, blob, out, counter);
}
}  // namespace fold

}  // namespace v6
}  // namespace nfx

// counter: null (the static walk) or a zeroed 32-bit word in global memory, DMA == 1 only: tiles handed out (the body's comment).
// The index word rides behind the blob's floats in LDS; a tile count the 32-bit index cannot hold walks statically.
template <int DMA, bool FOLD>
static int launch_v6(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples,
                     const void* blob, float* out, int max_blocks, hipStream_t stream, unsigned* counter = nullptr) {
    using namespace nfx;
    auto kern = FOLD ? v6::fold::nerf_mlp_bf16_v6_kernel<0, DMA> : v6::nerf_mlp_bf16_v6_kernel<0, DMA>;
    constexpr int lds = v6::lds_of<DMA, FOLD ? v6::Seq::Render : v6::Seq::Packed>;
    static_assert(lds % 4 == 0 && lds + 16 <= 160 * 1024, "room for the hand-out's index word");
    const long long n_tiles = (n_pts + v6::kTilePts - 1) / v6::kTilePts;
    if (DMA != 1 || n_tiles >= (1ll << 31) - max_blocks) counter = nullptr;
    return v6::launch_tiles(kern, counter ? lds + 16 : lds, n_pts, max_blocks, stream, rayo, rayd, z, n_pts, n_samples,
                            (const char*)blob, (float4*)out, counter);
}

extern "C" int nfx_launch_nerf_mlp_bf16_v6(const float* rayo, const float* rayd, const float* z, long long n_pts,
                                           int n_samples, const void* blob, float* out, int max_blocks, int dma_mode,
                                           hipStream_t stream) {
    if (n_pts <= 0) return 0;
    if (dma_mode == 1) return launch_v6<1, false>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream);   // variant 7
    if (dma_mode == 2) return launch_v6<2, false>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream);   // variant 8
    return launch_v6<0, false>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream);                      // variant 6
}

// The same three variants over a RENDER blob (nerf_fold.hip): 70 tiles, the bottleneck folded into rgb_out[0].  `counter`
// (variant 7 only, else ignored): see launch_v6.
extern "C" int nfx_launch_nerf_mlp_bf16_v6_fold(const float* rayo, const float* rayd, const float* z, long long n_pts,
                                                int n_samples, const void* blob, float* out, int max_blocks, int dma_mode,
                                                unsigned* counter, hipStream_t stream) {
    if (n_pts <= 0) return 0;
    if (dma_mode == 1) return launch_v6<1, true>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream, counter);
    if (dma_mode == 2) return launch_v6<2, true>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream);
    return launch_v6<0, true>(rayo, rayd, z, n_pts, n_samples, blob, out, max_blocks, stream);
}
