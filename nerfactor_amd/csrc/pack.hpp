// pack.hpp — host-side weight packer (no GPU needed): Keras Dense kernels [in, out] fp32 ->
// MFMA A-operand fragments in the order the fused-MLP kernels consume them (see mlp_engine.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <vector>

namespace nfx {
namespace pack {

// One input segment of a layer = a run of B-operand k-steps.
//   kHidden: `n` features produced by a previous layer (n % 16 == 0), k-steps follow the C/D
//            lane map: slot (s,h,j) <-> feature hidden_feature(s, h, j).
//   kPosEnc: the 6L+3 features of an L-band positional encoding, slots as in mlp_engine.hpp
//            (half 0 = sines + x0,x1; half 1 = cosines + x2).
//   kRaw:    `n` k-steps of raw features placed by an explicit slot table: slot (s,h,j) reads row
//            row0 + raw_slots[(2s + h) * 8 + j] of the kernel, or nothing (zero) where the entry is -1.
enum SegKind { kHidden = 0, kPosEnc = 1, kRaw = 2 };
struct Seg {
    SegKind kind;
    int n;     // kHidden: feature count; kPosEnc: L; kRaw: number of k-steps
    int row0;  // first row of this segment in the Keras kernel
    const int* raw_slots;  // kRaw: [n][2][8] row offsets relative to row0, -1 = zero
};
// Output columns = concatenation of column blocks taken from (possibly different) kernels that
// share the same input rows (used to fuse [bottleneck | sigma_out]).
struct Src {
    const float* kernel;  // [rows, cols] row-major
    const float* bias;    // [cols]
    int cols;
};

// The C/D lane map of the 32x32x16 MFMA: the feature a previous layer leaves in B slot (k-step s, lane half h, element j).
// Two k-steps cover one 32-row output tile, so the 32 slots of a two-k-step input (the learned BRDF's) read 16 s + ... .
int hidden_feature(int s, int h, int j);
int seg_ksteps(const Seg& s);
// Source row for B slot (k-step s within the segment, lane half h, element j), or -1.
int seg_row(const Seg& seg, int s, int h, int j);

// Packs one layer: n_tiles chunks of `chunk_frags` 1-KiB fragments (zero padded), then returns
// the number of bytes written to wdst.  bias_dst gets n_tiles*32 floats.
size_t pack_layer_bf16(const std::vector<Seg>& segs, const std::vector<Src>& srcs, int n_tiles,
                       int chunk_frags, uint8_t* wdst, float* bias_dst);

uint16_t f32_to_bf16_rne(float f);

// The five layers of a width-128 network (mlp128_layout.hpp) at w, their biases at b[544]: tiles 4/4/4/4/1, chunks of
// p0/8/8/p3/8 fragments.  in0 feeds layer 0; layer 3 takes the 128 hidden features, then in3.  A null biases[l] packs zeros.
// Returns the bytes written to w.
size_t pack_m128_ladder(const std::vector<Seg>& in0, const std::vector<Seg>& in3, int p0, int p3, const float* const kernels[5],
                        const float* const biases[5], int out_dim, uint8_t* w, float* b);

// Backward operands, as Keras kernels for pack_layer_bf16 (biases: none, the caller gives a sink).
// W[row0 : row0 + n_rows, :cols]^T, [pad_cols, n_rows] with the rows from `cols` on zero: dX = W dZ as a Dense layer on dZ.
std::vector<float> transposed(const float* kernel, int row0, int n_rows, int cols, int pad_cols);
// The input gradient of a layer whose kernel [., width] reads segment `in`: [width, 16 * seg_ksteps(in)], column
// hidden_feature(s, h, j) = row seg_row(in, s, h, j) of the kernel — so the C/D lane map of the product's output tile IS the
// input's B slot layout (mlp_engine.hpp:posenc<L> for kPosEnc, the slot table for kRaw), and empty slots get zeros.
std::vector<float> input_grad_kernel(const float* kernel, const Seg& in, int width);

// The fp32-class blobs (NFX_PREC_FP32) hold every kernel twice: the fragments of hi = bf16(W), then of lo = bf16(W - hi).
// lo_kernels() gives the fp32 kernels W - hi, to be packed like the kernels themselves.
struct Shape {
    int rows, cols;   // a Keras Dense kernel [in, out]
};
// enc[0..7] (enc[5] takes the skip input), sigma_out, bottleneck, rgb[0] (+ the view encoding), rgb[1]
extern const Shape kNerfShapes[12];
struct LoKernels {
    std::vector<std::vector<float>> data;
    std::vector<const float*> ptr;   // ptr[i] = data[i].data(): what the packers take
};
LoKernels lo_kernels(const float* const* kernels, const Shape* shapes, int n);
// [hi fragments | lo fragments | floats] at blob: pack_half(kernels, fragments, floats) lays out one half of weight_bytes
// and its n_floats floats (biases, which are the same for both halves: the second pass writes them to a sink).  Returns the
// first non-zero result of pack_half, else 0.
typedef std::function<int(const float* const* kernels, uint8_t* fragments, float* floats)> PackHalf;
int pack_hi_lo(const float* const* kernels, const Shape* shapes, int n, size_t weight_bytes, int n_floats, uint8_t* blob,
               const PackHalf& pack_half);

}  // namespace pack
}  // namespace nfx
