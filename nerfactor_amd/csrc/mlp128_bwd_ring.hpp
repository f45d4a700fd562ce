// mlp128_bwd_ring.hpp — the weight ring of the width-128 backward kernels: a tile's weights stream through kR slots of
// 8-KiB sub-chunks by LDS-DMA (global_load_lds_dwordx4, no VGPR staging), fetched kD sub-chunks ahead with counted
// s_waitcnt vmcnt, one barrier per sub-chunk.  mlp128_bwd_ring_kernel (mlp128_bwd.hip) streams the forward half of the
// train blob, 21 sub-chunks per tile, and keeps the dgrad half resident; mlp128_bwd_fused_kernel (mlp128_bwd_fused.hip)
// streams both halves, 23 or 35 sub-chunks.  gfx950 counts loads AND stores on vmcnt, in order: the counted waits are
// exact only where a kernel issues no store inside the window.
#pragma once
#include "lds_dma.hpp"
#include "mlp128_train_layout.hpp"
#include "mlp_engine.hpp"

namespace nfx {
namespace bwd {
namespace ring {

constexpr int kNW = 4;        // waves that share a ring: one 1-KiB piece of a 4-fragment sub-chunk each
constexpr int kR = 5, kD = kR - 1, kSlot = 8192;
constexpr int kFwdSub = 21;   // sub-chunks per tile: forward 0-20, dgrad through `out` 21-22, W3 23-26, W2 27-30, W1 31-34

// sub-chunk k of a tile of NS: fragments and first fragment in the train blob (P0 / P3 = fragments per layer-0 / layer-3
// chunk).  FIRST: the first sub-chunk ahead that may still be in flight at the barrier that ends sub-chunk k — 2 where the
// barrier has to guarantee k + 1 only; 3 where the first fragments of k + 2 are read while k + 1 multiplies
// (mlp128_bwd_fused.hip:sub_mma), so that k + 1 AND k + 2 have landed for every wave behind it.
template <int KSX, int NS, int FIRST>
struct Sub {
    using G = Geo<KSX>;
    static constexpr int kN = NS;
    static constexpr int frags(int k) {
        return k < 4 ? G::kP0 : k < 12 ? 8 : k < 20 ? ((k - 12) % 2 == 0 ? 8 : G::kP3 - 8) : 8;
    }
    static constexpr int off(int k) {
        return k < 4 ? k * G::kP0 : k < 8 ? 4 * G::kP0 + (k - 4) * 8 : k < 12 ? 4 * G::kP0 + 32 + (k - 8) * 8
             : k < 20 ? 4 * G::kP0 + 64 + ((k - 12) / 2) * G::kP3 + ((k - 12) % 2) * 8
             : k == 20 ? 4 * G::kP0 + 64 + 4 * G::kP3
             : G::kFwdFrags + (k - kFwdSub) * 8;   // the 112 dgrad fragments are contiguous: 14 sub-chunks of 8
    }
    static constexpr int pieces(int k) { return frags(k) / kNW; }   // 1-KiB pieces per wave: 1 | 2
    static constexpr int allow(int k) {   // pieces that may still be in flight at the barrier that ends sub-chunk k
        int n = 0;
        for (int j = FIRST; j <= kD; ++j) n += pieces((k + j) % NS);
        return n;
    }
};
static_assert(Sub<6, 35, 3>::off(kFwdSub) == Geo<6>::kFwdFrags && Sub<6, 35, 3>::off(34) + 8 == Geo<6>::kFwdFrags + Geo<6>::kBwdFrags, "blob");
static_assert(Sub<4, 35, 3>::off(kFwdSub) == Geo<4>::kFwdFrags && Sub<4, 35, 3>::off(34) + 8 == Geo<4>::kFwdFrags + Geo<4>::kBwdFrags, "blob");
static_assert(Sub<6, kFwdSub, 2>::off(kFwdSub - 1) + 8 == Geo<6>::kFwdFrags && Sub<4, kFwdSub, 2>::off(kFwdSub - 1) + 8 == Geo<4>::kFwdFrags,
              "the forward table ends where the dgrad fragments begin");

struct Ctx {
    char* smem;
    unsigned smem_lds;
    const char* blob;
    int lane, wave;   // wave: wave-uniform
    int cur;          // ring slot of the sub-chunk being consumed (wave-uniform)
};
// Before the first tile: the biases and sub-chunks 0 .. kD-1 of the first tile -> slots 0 .. kD-1; ends on the workgroup's barrier.
template <class S>
__device__ __forceinline__ void prologue(char* smem, float* bias_lds, const char* __restrict__ blob, int tid) {
    using G = typename S::G;
    const float* bsrc = reinterpret_cast<const float*>(blob + G::kWeightBytes);
    for (int i = tid; i < G::kBiasFloats; i += kNW * 64) bias_lds[i] = bsrc[i];
#pragma unroll
    for (int k = 0; k < kD; ++k) {
        const u32x4* src = reinterpret_cast<const u32x4*>(blob + (size_t)S::off(k) * 1024);
        u32x4* dst = reinterpret_cast<u32x4*>(smem + k * kSlot);
        for (int i = tid; i < S::frags(k) * 64; i += kNW * 64) dst[i] = src[i];
    }
    __syncthreads();
}
// start of sub-chunk K: fetch sub-chunk K + kD into the slot kD ahead (last read kR - kD = 1 sub-chunk ago: every wave
// has passed the barrier that ended it)
template <class S, int K>
__device__ __forceinline__ void begin(const Ctx& cx) {
    constexpr int F = (K + kD) % S::kN, n = S::pieces(F);
    unsigned long long base = reinterpret_cast<unsigned long long>(cx.blob);
    unsigned lds = cx.smem_lds;
    asm volatile("" : "+s"(base), "+s"(lds));   // per sub-chunk: keeps the addresses out of the loop preheader
    int slot = cx.cur + kD;
    slot = slot >= kR ? slot - kR : slot;
    const int piece0 = cx.wave * n;
    lds_dma_pieces<n>((unsigned)cx.lane * 16u, reinterpret_cast<const char*>(base) + (size_t)S::off(F) * 1024 + piece0 * 1024,
                      lds + (unsigned)slot * kSlot + (unsigned)piece0 * 1024u);
}
// end of sub-chunk K: the counted wait, the barrier, the next slot.  LGKM: the LDS reads that may still be in flight across
// the barrier — the fused kernel's carry fragments of the NEXT sub-chunk, issued last.  Everything older (this sub-chunk's own
// fragment reads: the compiler is free to sink their MFMAs below the barrier) has returned before the wave arrives, so no
// wave's DMA into this slot (begin<K + 1>) can overtake a read of it.  kAnyLgkm: a wait that names vmcnt alone (the
// stored-activation kernel, whose compiler-placed waits cover its reads).
constexpr int kAnyLgkm = -1;
template <class S, int K, int LGKM>
__device__ __forceinline__ void end(Ctx& cx) {
    if constexpr (LGKM == kAnyLgkm) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(S::allow(K)) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(%1)\n\ts_barrier" ::"n"(S::allow(K)), "n"(LGKM) : "memory");
    cx.cur = cx.cur + 1 == kR ? 0 : cx.cur + 1;
}

}  // namespace ring
}  // namespace bwd
}  // namespace nfx
