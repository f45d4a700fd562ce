// mlp128_resident.hpp — a width-128 network (mlp128_layout.hpp: 136 fragments + 2 KiB of biases) RESIDENT in LDS: its
// size, the fragment offsets of its 17 chunks, and the barrier-free tile ladder of lvis_v2.hip's kernels — one A
// fragment read from LDS feeds CT MFMAs, the epilogue of tile i-1 runs in the shadow of tile i's MFMAs, the accumulators
// of tile i+1 are initialised one tile ahead.  brdf_sphere.hip takes the constants only.
// (The one-time copy loop stays written out in the three kernels: as an inlined function it reorders their prologues.)
#pragma once
#include "mlp128_layout.hpp"
#include "mlp_engine.hpp"

namespace nfx {
namespace res128 {

constexpr int kLdsNet = m128::kMainWeightBytes + m128::kMainBiasFloats * 4;
// fragment offset of chunk K: L0 0-3 (4 frags), L1 4-7, L2 8-11 (8 frags), L3 12-15 (12 frags), out 16
constexpr int frag_off(int k) { return k < 4 ? 4 * k : k < 12 ? 16 + 8 * (k - 4) : k < 16 ? 80 + 12 * (k - 12) : 128; }

template <int CT>
struct Acc {
    f32x16 v[CT];
};
struct Pre {
    bf16x8 a[2];  // first two A fragments of the next tile (layer 0 has only two k-steps)
};

template <bool RELU>
__device__ __forceinline__ void cvt_pair(float v0, float v1, bf16x8& dst, int j) {
    typedef short s2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 vv = {v0, v1};
    b2 pr = __builtin_convertvector(vv, b2);
    if (RELU) {
        s2 w = __builtin_bit_cast(s2, pr);
        const s2 z = {0, 0};
        w = __builtin_elementwise_max(w, z);
        pr = __builtin_bit_cast(b2, w);
    }
    dst[j] = pr[0];
    dst[j + 1] = pr[1];
}

template <int CT>
struct EpiB {   // ReLU layer output -> next B operand (k-steps lo / hi), in register-pair pieces
    const Acc<CT>& acc;
    bf16x8 (&lo)[CT];
    bf16x8 (&hi)[CT];
    template <int R0, int R1>
    __device__ __forceinline__ void run() {
#pragma unroll
        for (int r = R0; r < R1; r += 2)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (r < 8) cvt_pair<true>(acc.v[c][r], acc.v[c][r + 1], lo[c], r);
                else cvt_pair<true>(acc.v[c][r], acc.v[c][r + 1], hi[c], r - 8);
            }
    }
};
struct EpiNone {
    template <int R0, int R1>
    __device__ __forceinline__ void run() {}
};

// accumulator initialisers for the NEXT tile
struct InitBias {   // broadcast LDS reads of the bias tile
    const float* bias_tile;
    template <int CT>
    __device__ __forceinline__ void operator()(int lane, Acc<CT>& acc) const {
        // one read group, the other column tiles' accumulators by register copy (accumulators are ArchVGPRs here):
        // light-visibility kernel 17.57 -> 17.1 ms on r01 against one read group per column tile
        const float* bt = bias_tile + 4 * (lane >> 5);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(bt + 8 * g);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                acc.v[c][4 * g + 0] = v[0];
                acc.v[c][4 * g + 1] = v[1];
                acc.v[c][4 * g + 2] = v[2];
                acc.v[c][4 * g + 3] = v[3];
            }
        }
    }
};
template <int CT>
struct InitPre {    // per-point pre-activation rows parked in the wave's LDS area (one point per column tile)
    const float* rows;   // [CT][256] floats
    int off;             // 32 t (+128 for layer 3)
    __device__ __forceinline__ void operator()(int lane, Acc<CT>& acc) const {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const float* bt = rows + c * 256 + off + 4 * (lane >> 5);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(bt + 8 * g);
                acc.v[c][4 * g + 0] = v[0];
                acc.v[c][4 * g + 1] = v[1];
                acc.v[c][4 * g + 2] = v[2];
                acc.v[c][4 * g + 3] = v[3];
            }
        }
    }
};

// Tile K: acc (already initialised) += W_K^T [b1 ; b2]; the previous tile's epilogue `prev` is spread over the
// k-steps; once it is complete `init_next` fills acc_next for tile K+1; the first A fragments of chunk K1 are read
// at the end.  No barrier: the weights never change.
template <int K, int K1, int KS1, int KS2, int CT, int KS1A, int KS2A, typename Epi, typename Init>
__device__ __forceinline__ void tile(const char* wlds, int lane, const bf16x8 (&b1)[KS1A][CT],
                                     const bf16x8 (&b2)[KS2A][CT], Acc<CT>& acc, Acc<CT>& acc_next, Pre& pre,
                                     Epi&& prev, Init&& init_next) {
    constexpr int KS = KS1 + KS2;
    // 16 accumulator registers of the previous tile in PIECES groups; at a layer boundary its outputs are this tile's
    // LAST input k-steps, so the epilogue must be complete well before them: 4 pieces (done after k-step 3) for 8-10
    // k-steps
    constexpr int PIECES = KS >= 4 ? 4 : KS;
    static_assert(16 % PIECES == 0 && (16 / PIECES) % 2 == 0, "pairs");
    const char* f0 = wlds + frag_off(K) * kFragBytes + lane * 16;
    bf16x8 abuf[4];
    abuf[0] = pre.a[0];
    abuf[1] = pre.a[1];
    if constexpr (KS > 2) abuf[2] = *reinterpret_cast<const bf16x8*>(f0 + 2 * kFragBytes);
    static_for<0, KS>([&](auto S) {
        constexpr int s = decltype(S)::value;
        if constexpr (s + 3 < KS) abuf[(s + 3) % 4] = *reinterpret_cast<const bf16x8*>(f0 + (s + 3) * kFragBytes);
        const bf16x8 a = abuf[s % 4];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const bf16x8 b = s < KS1 ? b1[s < KS1 ? s : 0][c] : b2[s >= KS1 ? s - KS1 : 0][c];
            acc.v[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc.v[c], 0, 0, 0);
        }
        if constexpr (s < PIECES) prev.template run<16 * s / PIECES, 16 * (s + 1) / PIECES>();
        if constexpr (s == PIECES - 1) {
            // keep the next tile's initial loads BEHIND the epilogue that frees their destination registers (hoisted
            // above it they need 16 CT temporaries and spill at CT = 4)
            __builtin_amdgcn_sched_barrier(0);
            init_next(lane, acc_next);
        }
    });
    const char* f1 = wlds + frag_off(K1) * kFragBytes + lane * 16;
    pre.a[0] = *reinterpret_cast<const bf16x8*>(f1);
    pre.a[1] = *reinterpret_cast<const bf16x8*>(f1 + kFragBytes);
}

// The network on CT x 32 rows whose two input k-steps are pl; the output tile is left in accs[0].  Chunk K accumulates in
// accs[K & 1]; layers: L0 K 0-3 (pl -> ha), L1 4-7 (ha -> hb), L2 8-11 (hb -> ha), L3 12-15 ([ha ; pl] -> hb), out 16
// (hb -> activation).  init03(off_pre, off_bias) is the accumulator initialiser of a layer-0 / layer-3 tile (per-point
// pre-activations or plain biases); after15() runs between tiles 15 and 16, behind the last layer-3 initialiser.
template <int CT, typename Init03, typename After15>
__device__ __forceinline__ void ladder(const char* wlds, const float* bias_lds, int lane, const bf16x8 (&pl)[2][CT],
                                       Acc<CT> (&accs)[2], Init03&& init03, After15&& after15) {
    bf16x8 ha[8][CT], hb[8][CT];
    Pre pre;
    {   // tile 0's operands
        const char* f0 = wlds + lane * 16;
        pre.a[0] = *reinterpret_cast<const bf16x8*>(f0);
        pre.a[1] = *reinterpret_cast<const bf16x8*>(f0 + kFragBytes);
        init03(0, 0)(lane, accs[0]);
    }
#define NFX_RES_TILE(K, KS1, KS2, B1, B2, PREV, NEXT) \
    tile<K, (K + 1) % 17, KS1, KS2, CT>(wlds, lane, B1, B2, accs[(K) & 1], accs[((K) + 1) & 1], pre, PREV, NEXT)
#define NFX_RES_EPI(K, OUT, T) EpiB<CT>{accs[(K) & 1], OUT[2 * (T)], OUT[2 * (T) + 1]}
#define NFX_RES_BIAS(OFF) (InitBias{bias_lds + (OFF)})
    NFX_RES_TILE(0, 2, 0, pl, pl, EpiNone{}, init03(32, 32));
    NFX_RES_TILE(1, 2, 0, pl, pl, NFX_RES_EPI(0, ha, 0), init03(64, 64));
    NFX_RES_TILE(2, 2, 0, pl, pl, NFX_RES_EPI(1, ha, 1), init03(96, 96));
    NFX_RES_TILE(3, 2, 0, pl, pl, NFX_RES_EPI(2, ha, 2), NFX_RES_BIAS(128));
    NFX_RES_TILE(4, 8, 0, ha, pl, NFX_RES_EPI(3, ha, 3), NFX_RES_BIAS(128 + 32));
    NFX_RES_TILE(5, 8, 0, ha, pl, NFX_RES_EPI(4, hb, 0), NFX_RES_BIAS(128 + 64));
    NFX_RES_TILE(6, 8, 0, ha, pl, NFX_RES_EPI(5, hb, 1), NFX_RES_BIAS(128 + 96));
    NFX_RES_TILE(7, 8, 0, ha, pl, NFX_RES_EPI(6, hb, 2), NFX_RES_BIAS(256));
    NFX_RES_TILE(8, 8, 0, hb, pl, NFX_RES_EPI(7, hb, 3), NFX_RES_BIAS(256 + 32));
    NFX_RES_TILE(9, 8, 0, hb, pl, NFX_RES_EPI(8, ha, 0), NFX_RES_BIAS(256 + 64));
    NFX_RES_TILE(10, 8, 0, hb, pl, NFX_RES_EPI(9, ha, 1), NFX_RES_BIAS(256 + 96));
    NFX_RES_TILE(11, 8, 0, hb, pl, NFX_RES_EPI(10, ha, 2), init03(128, 384));
    NFX_RES_TILE(12, 8, 2, ha, pl, NFX_RES_EPI(11, ha, 3), init03(128 + 32, 384 + 32));
    NFX_RES_TILE(13, 8, 2, ha, pl, NFX_RES_EPI(12, hb, 0), init03(128 + 64, 384 + 64));
    NFX_RES_TILE(14, 8, 2, ha, pl, NFX_RES_EPI(13, hb, 1), init03(128 + 96, 384 + 96));
    NFX_RES_TILE(15, 8, 2, ha, pl, NFX_RES_EPI(14, hb, 2), NFX_RES_BIAS(512));
    after15();
    NFX_RES_TILE(16, 8, 0, hb, pl, NFX_RES_EPI(15, hb, 3), [](int, Acc<CT>&) {});
#undef NFX_RES_TILE
#undef NFX_RES_EPI
#undef NFX_RES_BIAS
}

}  // namespace res128
}  // namespace nfx
