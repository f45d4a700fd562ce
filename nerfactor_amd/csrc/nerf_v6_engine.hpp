// nerf_v6_engine.hpp — the tile / layer machinery of the variant-6 NeRF kernels: the render kernels of nerf_mlp_v6.hip (whose
// header describes the dataflow) and the bf16 density kernels of nerf_sigma_v6.hip.  One wave per SIMD, 64 points per wave, a
// ring of weight chunks in LDS, the epilogue of tile K-1 under the MFMAs of tile K, a bare s_barrier per tile.
//
// Seq: the chunk sequence a kernel walks, a compile-time argument of everything that depends on it.
//   Packed  the packed blob (nerf_layout.hpp): 78 chunks = 13 x 6, chunk k lives in slot k % ring;
//   Render  the render blob (nerf_fold_layout.hpp, written by nerf_fold.hip): the linear bottleneck is folded into rgb_out[0],
//           its 8 tiles are gone and the sigma tile and rgb_out[0] both read enc[7]'s output — 70 chunks.  70 is no multiple of
//           the ring, so the chunk -> slot map is no longer k % ring there (slot_of below; tests/test_cpu_nerf_fold.py proves
//           the sequence in the happens-before model of tests/test_cpu_ring_protocol.py);
//   Geom    the GEOM blob (nerf_geom_layout.hpp), density only: chunks 0..63 = the encoder exactly as in the packed blob,
//           chunk 64 = the sigma tile, chunk 65 = the first reverse-sweep chunk, fetched and not multiplied (the weight
//           sequence must be a multiple of the 6-slot ring) — 66 chunks = 11 x 6, slot k % ring; fragment counts and offsets
//           of the chunks k < 66 are the packed blob's.
#pragma once
#include "mlp_engine.hpp"
#include "lds_dma.hpp"
#include "nerf_layout.hpp"
#include "nerf_fold_layout.hpp"

namespace nfx {
namespace v6 {

enum class Seq { Packed, Render, Geom };

constexpr int kNW = 4, kCT = 2;
constexpr int kTilePts = kNW * 32 * kCT;   // points of a tile: every wave takes kCT column tiles of 32
// ring size / fetch distance: register-staged 3 slots, chunk K+2 fetched during tile K; LDS-DMA 6 slots (78 = 6 x 13),
// chunk K+3 issued during tile K and awaited at the end of tile K: when tile K+1 prefetches the head of chunk K+2
// before ITS barrier, every wave's pieces of that chunk have been behind a barrier already
// DMA = 2 (variant 8): register-staged like 0, but chunk K+3 is fetched during tile K into one of TWO register sets and
// written to its slot at the end of tile K+1: the global loads get two tile times to land instead of one, and the
// compiler's counted vmcnt lets the newer set stay in flight across the store of the older one.
// Render sequence (70 chunks): LDS-DMA keeps 6 slots, chunks 66..69 live in slots 1..4: any FIVE consecutive chunks of the
// cyclic sequence sit in different slots, so the slot chunk K+3 is fetched into during tile K was last read in tile K-2 or
// earlier.  Register-staged: a 4th slot for chunk 69 alone: any THREE consecutive chunks sit in different slots, as on the
// 3-slot ring (chunk K+2 is stored at the end of tile K into a slot last read in tile K-1 or earlier).
template <int DMA, Seq S> constexpr int ring_of = DMA == 1 ? 6 : S == Seq::Render ? 4 : 3;
template <int DMA, Seq S> constexpr int slot_of(int k) {
    if (S != Seq::Render) return k % ring_of<DMA, S>;
    return DMA == 1 ? (k < 66 ? k % 6 : k - 65) : (k == 69 ? 3 : k % 3);
}
constexpr int kDmaDist = 3;   // LDS-DMA fetch distance in tiles (4 measured the same; the 6-slot ring holds either)
template <int DMA> constexpr int dist_of = DMA == 1 ? kDmaDist : DMA ? 3 : 2;
template <int DMA, Seq S> constexpr int lds_of = ring_of<DMA, S> * kSlotBytes + nerf::kBiasFloats * 4;
// Geom: 64 encoder chunks + the sigma tile + one idle chunk
template <Seq S> constexpr int n_chunks = S == Seq::Render ? nerf::fold::kNChunks : S == Seq::Geom ? 66 : nerf::kNChunks;
static_assert(n_chunks<Seq::Packed> % 6 == 0 && n_chunks<Seq::Geom> % 6 == 0,
              "a chunk sequence on the k % ring map wraps on the 6-slot (and the 3-slot) ring");
template <Seq S> constexpr int seq_frags(int k) {
    return S == Seq::Render ? nerf::fold::chunk_frags(k) : nerf::chunk_frags(k);
}
template <Seq S> constexpr int seq_frag_offset(int k) {
    return S == Seq::Render ? nerf::fold::chunk_frag_offset(k) : nerf::chunk_frag_offset(k);
}

constexpr int kPreA = 3;   // A fragments in flight ahead of their MFMAs (2 / 3 / 4 measured: 1373 / 1372 / 1363 TFLOP/s)

struct Acc {
    f32x16 v[kCT];
};
struct Pre {
    bf16x8 a[kPreA];  // first A fragments of the next tile
};

template <bool RELU>
__device__ __forceinline__ void cvt_pair(float v0, float v1, bf16x8& dst, int j) {
    typedef short s2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 vv = {v0, v1};
    b2 pr = __builtin_convertvector(vv, b2);  // one v_cvt_pk_bf16_f32
    if (RELU) {                               // a negative bf16 is a negative int16: ReLU = one v_pk_max_i16
        s2 w = __builtin_bit_cast(s2, pr);
        const s2 z = {0, 0};
        w = __builtin_elementwise_max(w, z);
        pr = __builtin_bit_cast(b2, w);
    }
    dst[j] = pr[0];
    dst[j + 1] = pr[1];
}

// The epilogue of a tile, run in pieces (accumulator rows R0..R1) under the first k-steps of the next tile.
template <bool RELU>
struct EpiB {
    const Acc& acc;
    bf16x8 (&lo)[kCT];
    bf16x8 (&hi)[kCT];
    template <int R0, int R1>
    __device__ __forceinline__ void run() {
#pragma unroll
        for (int r = R0; r < R1; r += 2)
#pragma unroll
            for (int c = 0; c < kCT; ++c) {
                if (r < 8) cvt_pair<RELU>(acc.v[c][r], acc.v[c][r + 1], lo[c], r);
                else cvt_pair<RELU>(acc.v[c][r], acc.v[c][r + 1], hi[c], r - 8);
            }
    }
};
struct EpiNone {
    template <int R0, int R1>
    __device__ __forceinline__ void run() {}
};
struct EpiSigma {
    const Acc& acc;
    float (&sigma)[kCT];
    template <int R0, int R1>
    __device__ __forceinline__ void run() {
        if constexpr (R0 == 0) {
#pragma unroll
            for (int c = 0; c < kCT; ++c) sigma[c] = acc.v[c][0];
        }
    }
};

__device__ __forceinline__ void bias_to_acc(const float* bias_tile, int lane, Acc& acc) {
    // one broadcast read group, the second column tile's accumulators copied from the first: +1.8 % on r01 once the
    // accumulators live in ArchVGPRs (MFMA VGPR form); a second read group costs a full LDS pass
    const float* bt = bias_tile + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(bt + 8 * g);
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
            acc.v[c][4 * g + 0] = v[0];
            acc.v[c][4 * g + 1] = v[1];
            acc.v[c][4 * g + 2] = v[2];
            acc.v[c][4 * g + 3] = v[3];
        }
    }
}

typedef __attribute__((address_space(1))) u32x4 gu32x4;   // explicit global address space: global_load, not flat_load

struct Regs {
    u32x4 r[2][6];   // two staging sets of up to six 4-KiB pieces (variant 8)
};

struct Ctx {
    char* smem;
    const char* blob;
    int tid;
    unsigned smem_lds;   // LDS byte address of smem (for M0)
    int wave;            // wave-uniform
};

// DMA = 1: the weight stream goes global -> LDS directly (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPR
// staging, no ds_write, no lgkmcnt drain); completion is tracked with counted s_waitcnt vmcnt (the pieces of chunk
// K+2 must have landed before the barrier that ends tile K+1, those of chunk K+3 may still be in flight).
// r03: all pieces of a chunk in ONE statement — M0 is saved, set and restored once, and the pieces are addressed
// through the instruction's immediate offset, which the hardware adds to the global AND to the LDS address (the pieces of a
// wave are 1 KiB apart in both).  The r02 form issued every piece as its own statement: 8 instructions per piece (two
// 64-bit address adds, one LDS address add, M0 save / set / s_nop / restore) = 32-48 scalar instructions in the first two
// MFMA gaps of every tile, where a lone wave can hide five (MI355X_MICROARCH.md).  Only the fragments a tile really
// multiplies are fetched (the chunks of layer 0, layer 5 and rgb_out[0] are padded to 8 / 24 fragments in the blob):
// 298 pieces per pass instead of 318.
template <Seq S> constexpr int used_frags(int k) {
    constexpr bool fold = S == Seq::Render;
    return k < 8 ? 4 : k < 40 ? 16 : k < 48 ? 20 : k < (fold ? 65 : 73) ? 16 : k < (fold ? 69 : 77) ? 18 : 8;
}
template <Seq S> constexpr int dma_pieces(int k) { return (used_frags<S>(k) + kNW - 1) / kNW; }   // 1-KiB pieces per wave: 1 | 4 | 5 | 2
template <int K, Seq S>
__device__ __forceinline__ void dma_chunk(const Ctx& cx) {
    constexpr int n = dma_pieces<S>(K);
    unsigned long long base = reinterpret_cast<unsigned long long>(cx.blob);
    unsigned lds = cx.smem_lds;
    asm volatile("" : "+s"(base), "+s"(lds));       // per tile: keeps the piece addresses out of the loop preheader
    const int piece0 = cx.wave * n;
    const char* g = reinterpret_cast<const char*>(base) + (size_t)seq_frag_offset<S>(K) * kFragBytes + piece0 * 1024;
    const unsigned l = lds + slot_of<1, S>(K) * kSlotBytes + piece0 * 1024;
    lds_dma_pieces<n>((cx.tid & 63) * 16, g, l);
}
// Tile K (global chunk index).  On entry `acc` holds the tile's bias and `pre` its first three A fragments; on exit
// `acc_next` / `pre` hold the same for tile K+1 (bias from `next_bias`).  IDLE: the tile reads its A fragments and issues no
// MFMA (the density kernels' last chunk: it keeps the ring turning and gives the pending epilogue its k-steps).
template <int K, int KS1, int KS2, int DMA, Seq S, bool IDLE = false, int KS1A, int KS2A, typename Epi>
__device__ __forceinline__ void tile(const Ctx& cx, Regs& rg, const float* next_bias, const bf16x8 (&b1)[KS1A][kCT],
                                     const bf16x8 (&b2)[KS2A][kCT], Acc& acc, Acc& acc_next, Pre& pre, Epi&& prev) {
    constexpr int KS = KS1 + KS2;
    constexpr int PIECES = KS >= 16 ? 8 : 4;
    // (starting the previous tile's epilogue two k-steps into the tile, behind its first MFMAs, measured no gain on r01)
    constexpr int SP = PIECES < KS ? PIECES : KS - 1;  // k-step after which the previous tile's epilogue is complete
    constexpr int K1 = (K + 1) % n_chunks<S>, K2 = (K + dist_of<DMA>) % n_chunks<S>;   // K2: the chunk fetched during this tile
    constexpr int NL2 = seq_frags<S>(K2) / 4;
    const int lane = cx.tid & 63;
    const char* f0 = cx.smem + slot_of<DMA, S>(K) * kSlotBytes + lane * 16;
    Stage<DMA ? 1 : NL2, kNW> st;
    if constexpr (DMA == 1) {
        dma_chunk<K2, S>(cx);
    } else if constexpr (DMA == 2) {
        unsigned long long gb = reinterpret_cast<unsigned long long>(cx.blob);
        asm volatile("" : "+s"(gb));   // (an integer: a laundered generic pointer would turn the loads into flat_load)
        const gu32x4* g = reinterpret_cast<const gu32x4*>(gb + (size_t)seq_frag_offset<S>(K2) * kFragBytes);
#pragma unroll
        for (int k = 0; k < NL2; ++k) rg.r[K & 1][k] = g[k * kPieceThreads + cx.tid];
    } else {
        // opaque per tile: otherwise the ~300 loop-invariant chunk addresses are hoisted out of the point-tile loop
        // and spilled (same cure as variant 2)
        unsigned long long gb = reinterpret_cast<unsigned long long>(cx.blob);
        asm volatile("" : "+s"(gb));
        const gu32x4* g = reinterpret_cast<const gu32x4*>(gb + (size_t)seq_frag_offset<S>(K2) * kFragBytes);
#pragma unroll
        for (int k = 0; k < NL2; ++k) st.r[k] = g[k * kPieceThreads + cx.tid];   // (kNW = 4: one piece group)
    }
    bf16x8 abuf[kPreA + 1];
#pragma unroll
    for (int i = 0; i < kPreA; ++i) abuf[i] = pre.a[i];
    static_for<0, KS>([&](auto St) {
        constexpr int s = decltype(St)::value;
        if constexpr (s + kPreA < KS)
            abuf[(s + kPreA) % (kPreA + 1)] = *reinterpret_cast<const bf16x8*>(f0 + (s + kPreA) * kFragBytes);
        const bf16x8 a = abuf[s % (kPreA + 1)];
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
            const bf16x8 b = s < KS1 ? b1[s < KS1 ? s : 0][c] : b2[s >= KS1 ? s - KS1 : 0][c];
            if constexpr (IDLE) {
                asm volatile("" ::"v"(a), "v"(b));
            } else {
                acc.v[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc.v[c], 0, 0, 0);
            }
        }
        if constexpr (s < PIECES) prev.template run<16 * s / PIECES, 16 * (s + 1) / PIECES>();
        // the other accumulator set is free now: tile K+1's bias goes to its accumulators
        if constexpr (s == SP) bias_to_acc(next_bias, lane, acc_next);
    });
    // chunk K+2 to its slot as late as possible (its global loads had the whole tile to land; measured: storing at
    // mid-tile stalls on vmcnt, L2 latency under this load exceeds half a tile)
    if constexpr (DMA == 1) {
        // the chunk issued one tile ago must be complete before the barrier; this tile's pieces may stay in flight
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(dma_pieces<S>(K2)) : "memory");
    } else if constexpr (DMA == 2) {
        // chunk K+2, fetched during tile K-1 into the other register set, to slot (K+2) % 3 = the slot tile K-1 read
        constexpr int KP = (K + 2) % n_chunks<S>, NLP = seq_frags<S>(KP) / 4;
        u32x4* dst = reinterpret_cast<u32x4*>(cx.smem + slot_of<DMA, S>(KP) * kSlotBytes);
#pragma unroll
        for (int k = 0; k < NLP; ++k) dst[k * kPieceThreads + cx.tid] = rg.r[(K + 1) & 1][k];
    } else {
        st.store(reinterpret_cast<u32x4*>(cx.smem + slot_of<DMA, S>(K2) * kSlotBytes), cx.tid);
    }
    const char* f1 = cx.smem + slot_of<DMA, S>(K1) * kSlotBytes + lane * 16;
#pragma unroll
    for (int i = 0; i < kPreA; ++i) pre.a[i] = *reinterpret_cast<const bf16x8*>(f1 + i * kFragBytes);
    // (a __builtin_amdgcn_sched_barrier(0) here costs 4 %: it stops the scheduler from draining the tail MFMAs of this
    //  tile behind the barrier; the per-tile laundering of the blob base above is what keeps the weight addresses
    //  from being hoisted)
    asm volatile("s_barrier" ::: "memory");
}

// A Dense layer of NT tiles starting at chunk K0, outputs to bout.  `prev0` = pending epilogue of tile K0-1;
// `next_bias` = bias of the tile after this layer's last one.  On return the last tile's epilogue is pending.
template <int K0, int KS1, int KS2, int NT, bool RELU, int DMA, Seq S, int KS1A, int KS2A, int NTA, typename Epi0>
__device__ __forceinline__ void layer(const Ctx& cx, Regs& rg, const float* bias, const float* next_bias,
                                      const bf16x8 (&b1)[KS1A][kCT], const bf16x8 (&b2)[KS2A][kCT],
                                      bf16x8 (&bout)[NTA][kCT], Acc (&accs)[2], Pre& pre, Epi0&& prev0) {
    static_for<0, NT>([&](auto T) {
        constexpr int t = decltype(T)::value;
        constexpr int K = K0 + t;
        const float* nb = t == NT - 1 ? next_bias : bias + 32 * (t + 1);
        if constexpr (t == 0) {
            tile<K, KS1, KS2, DMA, S>(cx, rg, nb, b1, b2, accs[K & 1], accs[(K + 1) & 1], pre, prev0);
        } else {
            EpiB<RELU> e{accs[(K - 1) & 1], bout[2 * (t - 1)], bout[2 * (t - 1) + 1]};
            tile<K, KS1, KS2, DMA, S>(cx, rg, nb, b1, b2, accs[K & 1], accs[(K + 1) & 1], pre, e);
        }
    });
}

// The floats of a kernel's blob (biases; the bias of tile 0 first) live in LDS behind the ring.
template <int DMA, Seq S>
__device__ __forceinline__ float* floats_of(char* smem) {
    return reinterpret_cast<float*>(smem + ring_of<DMA, S> * kSlotBytes);
}

// What a kernel does before its loop over point tiles: the `n_floats` floats that start `float_bytes` into the blob go to
// floats_of(smem), the first chunks go through registers to their slots (as many as the fetch distance: the tile loop fetches
// from chunk dist_of<DMA> on), and tile 0 gets its first A fragments and its bias.  Returns the tiles' context.
// (tid = threadIdx.x and lane = tid & 63 come from the caller: read again here, they cost the LDS-DMA render kernels one SGPR
//  and move the register-staged folded one off its 511 registers.)
template <int DMA, Seq S>
__device__ __forceinline__ Ctx prologue(char* smem, const char* __restrict__ blob, int float_bytes, int n_floats, int tid,
                                        int lane, Regs& rg, Pre& pre, Acc& acc0) {
    static_assert(nerf::kBiasL0 == 0, "the bias of tile 0 is float 0 of every blob");
    float* fl = floats_of<DMA, S>(smem);
    {
        const float* src = reinterpret_cast<const float*>(blob + float_bytes);
        for (int i = tid; i < n_floats; i += kNW * 64) fl[i] = src[i];
    }
    typedef __attribute__((address_space(3))) char lds_char;
    Ctx cx{smem, blob, tid, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_char*)smem),
           __builtin_amdgcn_readfirstlane(tid >> 6)};
    if constexpr (DMA == 2) {   // chunk 2 plays "fetched during tile -1": register set 1, stored at the end of tile 0
        const u32x4* g = reinterpret_cast<const u32x4*>(blob + (size_t)seq_frag_offset<S>(2) * kFragBytes);
#pragma unroll
        for (int k = 0; k < seq_frags<S>(2) / 4; ++k) rg.r[1][k] = g[k * kPieceThreads + tid];
    }
    // chunks 0 and 1 -> slots 0 and 1
    Stage<seq_frags<S>(0) / 4, kNW> s0;
    Stage<seq_frags<S>(1) / 4, kNW> s1;
    s0.load(reinterpret_cast<const u32x4*>(blob), tid);
    s1.load(reinterpret_cast<const u32x4*>(blob + (size_t)seq_frag_offset<S>(1) * kFragBytes), tid);
    s0.store(reinterpret_cast<u32x4*>(smem), tid);
    s1.store(reinterpret_cast<u32x4*>(smem + kSlotBytes), tid);
    if constexpr (DMA == 1) {   // fetch distance 3: chunk 2 must be resident before the first tile as well
        Stage<seq_frags<S>(2) / 4, kNW> s2;
        s2.load(reinterpret_cast<const u32x4*>(blob + (size_t)seq_frag_offset<S>(2) * kFragBytes), tid);
        s2.store(reinterpret_cast<u32x4*>(smem + 2 * kSlotBytes), tid);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPreA; ++i) pre.a[i] = *reinterpret_cast<const bf16x8*>(smem + lane * 16 + i * kFragBytes);
    bias_to_acc(fl, lane, acc0);
    return cx;
}

// Launch of a tile-loop kernel: min(tiles of `n_pts` points, max_blocks) workgroups of kNW waves, `lds` bytes of dynamic LDS.
template <typename Kern, typename... Args>
inline int launch_tiles(Kern kern, int lds, long long n_pts, int max_blocks, hipStream_t stream, Args... args) {
    const long long n_tiles = (n_pts + kTilePts - 1) / kTilePts;
    const int grid = (int)(n_tiles < max_blocks ? n_tiles : max_blocks);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kNW * 64), lds, stream, args...);
    return (int)hipGetLastError();
}

}  // namespace v6
}  // namespace nfx
