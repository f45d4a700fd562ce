// nerf_fold.hip — writes the RENDER blob (nerf_fold_layout.hpp) from a packed bf16 NeRF blob, on the device.
//
// The network's bottleneck layer is linear and feeds rgb_out[0] only, so the two collapse into one layer of rgb_out[0]'s
// shape: W' = Wb W0a (256 x 128), b0' = bb W0a + b0.  The render kernels then skip the bottleneck's 8 tiles (256 of 2368
// MFMAs per 64 points).  Everything else — the encoder, the sigma tile, the view rows of rgb_out[0], rgb_out[1] — is copied
// byte for byte, so the density is the unfolded kernels' density bit for bit.
//
// This runs on EVERY folded forward call (8.4 M multiply-adds and 1.1 MB against a launch of tens of milliseconds) and the
// result is not cached: during training the blobs are re-packed in place by device kernels, a cache keyed on the blob's
// address would go stale without anybody noticing.
//
// Arithmetic (tests/test_cpu_nerf_fold.py restates it in NumPy; the device blob equals that one bit for bit):
//   W'[k][c] = bf16_rne( sum_{m = 0..255, ascending} Wb[k][m] * W0a[m][c] )   fp32; the operands are the bf16 values
//              read back from the fragments, so every product is exact and the sum is a plain fp32 running sum from 0
//   b0'[c]   = ( sum_{m ascending} fl(bb[m] * W0a[m][c]) ) + b0[c]            fp32 multiply, then add (no fused form)
// Row permutation: a hidden layer's k-step s, lane half h, element j holds input feature F(s, h, j) = 16 s + (j & 3) +
// 8 (j >> 2) + 4 h (pack.hpp) whatever the layer, so the folded layer — which consumes enc[7]'s output like the
// bottleneck — keeps the bottleneck's K slots: fragment s, lane (h, n), element j of folded tile u is W'[F(s, h, j)][32 u + n],
// Wb[F(s, h, j)][m] sits in bottleneck chunk m >> 5, fragment s, lane (h, m & 31), element j, and W0a[m][c] in
// rgb_out[0] chunk c >> 5, fragment m >> 4, lane (hm, c & 31), element jm with F(m >> 4, hm, jm) = m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nerf_fold_layout.hpp"
#include "launchers.hpp"

namespace nfx {
namespace nfold {

constexpr int kThreads = 256;
constexpr int kFoldBlocks = 4 * 16 * 64 * 8 / kThreads;   // one thread per folded weight: 128 blocks
constexpr int kBiasBlock = kFoldBlocks;                    // one block for the 128 folded biases
constexpr int kCopyBlocks = 64;
constexpr int kBlocks = kFoldBlocks + 1 + kCopyBlocks;

__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {   // pack.cpp:f32_to_bf16_rne (finite sums only)
    uint32_t u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// W0a[m][32 u + n] as stored in the packed blob (element index into the bf16 view of the blob)
__device__ __forceinline__ int w0a_index(int u, int m, int n) {
    const int r = m & 15, jm = (r & 3) | ((r >> 3) << 2), hm = (r >> 2) & 1;
    return (nerf::chunk_frag_offset(73) + u * nerf::chunk_frags(73) + (m >> 4)) * 512 + (hm * 32 + n) * 8 + jm;
}

struct Seg {
    int src, dst, n;   // 16-byte units
};

// ctrl: null, or the 16-byte control block of a render workspace (nfx.h: nfx_nerf_render_workspace_bytes), cleared here so that
// the render launch behind this one on the stream finds its tile counter at 0 on every call, replays of a captured graph included.
__global__ __launch_bounds__(kThreads) void nerf_fold_kernel(const char* __restrict__ blob, char* __restrict__ out,
                                                             uint4* __restrict__ ctrl) {
    using namespace nerf;
    if (ctrl && blockIdx.x == kBiasBlock && threadIdx.x == kThreads - 1) *ctrl = make_uint4(0u, 0u, 0u, 0u);
    const uint16_t* w = reinterpret_cast<const uint16_t*>(blob);
    const float* fl = reinterpret_cast<const float*>(blob + kWeightBytes);
    const int b = blockIdx.x;
    if (b < kFoldBlocks) {
        const int t = b * kThreads + threadIdx.x;
        const int j = t & 7, lane = (t >> 3) & 63, s = (t >> 9) & 15, u = t >> 13;
        const int h = lane >> 5, n = lane & 31;
        const uint16_t* wb = w + (chunk_frag_offset(fold::kBottChunk) + s) * 512 + h * 32 * 8 + j;
        float acc = 0.0f;
#pragma unroll 8
        for (int m = 0; m < 256; ++m) {
            const float a = bf16_to_f32(wb[(m >> 5) * chunk_frags(fold::kBottChunk) * 512 + (m & 31) * 8]);
            acc = acc + a * bf16_to_f32(w[w0a_index(u, m, n)]);
        }
        uint16_t* o = reinterpret_cast<uint16_t*>(out);
        o[(fold::chunk_frag_offset(fold::kRgb0Chunk + u) + s) * 512 + lane * 8 + j] = f32_to_bf16_rne(acc);
    } else if (b == kBiasBlock) {
        const int c = threadIdx.x;
        if (c < 128) {
            float acc = 0.0f;
#pragma unroll 8
            for (int m = 0; m < 256; ++m) acc = acc + fl[kBiasBott + m] * bf16_to_f32(w[w0a_index(c >> 5, m, c & 31)]);
            reinterpret_cast<float*>(out + fold::kWeightBytes)[kBiasRgb0 + c] = acc + fl[kBiasRgb0 + c];
        }
    } else {
        // everything the fold leaves alone, in 16-byte units: the encoder, the sigma tile, fragments 16..23 of the four
        // rgb_out[0] chunks (view rows and padding), rgb_out[1], and the float section around the rgb_out[0] biases
        constexpr int F = 64, W = kWeightBytes / 16, WF = fold::kWeightBytes / 16;
        const Seg segs[9] = {
            {0, 0, chunk_frag_offset(64) * F},
            {chunk_frag_offset(72) * F, fold::chunk_frag_offset(fold::kSigmaChunk) * F, 16 * F},
            {(chunk_frag_offset(73) + 16) * F, (fold::chunk_frag_offset(65) + 16) * F, 8 * F},
            {(chunk_frag_offset(74) + 16) * F, (fold::chunk_frag_offset(66) + 16) * F, 8 * F},
            {(chunk_frag_offset(75) + 16) * F, (fold::chunk_frag_offset(67) + 16) * F, 8 * F},
            {(chunk_frag_offset(76) + 16) * F, (fold::chunk_frag_offset(68) + 16) * F, 8 * F},
            {chunk_frag_offset(77) * F, fold::chunk_frag_offset(fold::kRgb1Chunk) * F, 8 * F},
            {W, WF, kBiasRgb0 / 4},
            {W + kBiasRgb1 / 4, WF + kBiasRgb1 / 4, (kBiasFloats - kBiasRgb1) / 4},
        };
        const uint4* src = reinterpret_cast<const uint4*>(blob);
        uint4* dst = reinterpret_cast<uint4*>(out);
        const int t0 = (b - kBiasBlock - 1) * kThreads + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            for (int i = t0; i < segs[k].n; i += kCopyBlocks * kThreads) dst[segs[k].dst + i] = src[segs[k].src + i];
    }
}

static_assert(nerf::kBiasRgb0 % 4 == 0 && nerf::kBiasRgb1 % 4 == 0 && nerf::kBiasFloats % 4 == 0, "16-byte float segments");
static_assert(nerf::chunk_frags(73) == 24 && nerf::chunk_frags(64) == 16, "layout");

}  // namespace nfold
}  // namespace nfx

// blob: a packed bf16 NeRF blob (nerf::kBlobBytes); out: nerf::fold::kBlobBytes, 16-byte aligned, not overlapping blob;
// ctrl: null or 16 bytes, 16-byte aligned, that one thread clears.
extern "C" int nfx_launch_nerf_fold(const void* blob, void* out, void* ctrl, hipStream_t stream) {
    using namespace nfx::nfold;
    hipLaunchKernelGGL(nerf_fold_kernel, dim3(kBlocks), dim3(kThreads), 0, stream, (const char*)blob, (char*)out, (uint4*)ctrl);
    return (int)hipGetLastError();
}
