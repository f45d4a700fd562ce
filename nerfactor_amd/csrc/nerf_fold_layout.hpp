// nerf_fold_layout.hpp — layout of the RENDER blob: the bf16 NeRF blob (nerf_layout.hpp) with the linear bottleneck folded
// into rgb_out[0].  The bottleneck (256 -> 256) has no activation and feeds rgb_out[0] only, so
//   relu(W0a^T (Wb^T h + bb) + W0v^T pe_v + b0) = relu((Wb W0a)^T h + W0v^T pe_v + (bb W0a + b0))
// and its 8 tiles leave the render kernels.  The render blob is written on the device by nerf_fold.hip from a packed blob;
// no host packer produces it and the packed blob itself is unchanged.
//
// 70 chunks in consumption order (source chunk of the packed blob in brackets):
//   0..63   enc[0..7]                           [0..63]   copied
//   64      sigma_out (row 0 of its tile)       [72]      copied
//   65..68  folded rgb_out[0]: 256+32 -> 128    [73..76]  fragments 0..15 = bf16(Wb W0a), 16..23 (view rows, padding) copied
//   69      rgb_out[1]                          [77]      copied
// The float section keeps the packed blob's offsets (nerf::kBias*): the bottleneck's 256 biases are copied and never read,
// the 128 floats at kBiasRgb0 hold b0' = bb W0a + b0.
#pragma once
#include "nerf_layout.hpp"
namespace nfx {
namespace nerf {
namespace fold {
constexpr int kNChunks = 70;
constexpr int kSigmaChunk = 64, kRgb0Chunk = 65, kRgb1Chunk = 69;
constexpr int src_chunk(int k) { return k < 64 ? k : k + 8; }     // chunk of the packed blob behind render chunk k
constexpr int chunk_frags(int k) { return nerf::chunk_frags(src_chunk(k)); }
constexpr int chunk_frag_offset(int k) {
    int off = 0;
    for (int i = 0; i < k; ++i) off += chunk_frags(i);
    return off;
}
constexpr int kFrags = chunk_frag_offset(kNChunks);  // 1144
constexpr int kWeightBytes = kFrags * 1024;
using nerf::kBiasL0;
using nerf::kBiasBott;
using nerf::kBiasRgb0;
using nerf::kBiasRgb1;
using nerf::kBiasFloats;
using nerf::kNL0;
using nerf::kNLH;
using nerf::kNL5;
using nerf::kNLR0;
using nerf::kNLR1;
constexpr int kBlobBytes = kWeightBytes + kBiasFloats * 4;
constexpr int kBottChunk = 64;                       // first of the packed blob's 8 bottleneck chunks
static_assert(kFrags == nerf::kFrags - 8 * 16, "the bottleneck's 128 fragments leave the stream");
static_assert(kNChunks % 2 == 0, "tile K accumulates in accs[K & 1] in every pass");
}  // namespace fold
}  // namespace nerf
}  // namespace nfx
