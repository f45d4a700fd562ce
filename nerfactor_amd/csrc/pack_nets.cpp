// pack_nets.cpp — the host packers of the tuned networks' weight blobs (include/nfx.h: nfx_*_pack_*weights and their
// *_packed_bytes): NeRF (render, training, density gradient), the width-128 surface MLPs and the learned BRDF (inference,
// training).  Each lays out what its *_layout.hpp describes from the pieces of pack.hpp.  Pure host code, no GPU needed.
#include <string.h>

#include <vector>

#include "capi_common.hpp"
#include "mlp128_layout.hpp"
#include "nerf_geom_layout.hpp"
#include "nerf_layout.hpp"
#include "nerf_train_layout.hpp"
#include "pack.hpp"

using namespace nfx;
using namespace nfx::pack;

namespace {
const Seg kHid16{kHidden, 16, 0, nullptr}, kHid128{kHidden, 128, 0, nullptr}, kHid256{kHidden, 256, 0, nullptr};

// One backward product at w: the Dense layer with Keras kernel t [., cols] (no bias) on the gradient segments `in`, in
// cols / 32 chunks of chunk_frags fragments.  Returns the bytes written.
size_t pack_dgrad(const std::vector<Seg>& in, const std::vector<float>& t, int cols, int chunk_frags, uint8_t* w) {
    std::vector<float> sink(cols);
    return pack_layer_bf16(in, {{t.data(), nullptr, cols}}, cols / 32, chunk_frags, w, sink.data());
}

// bf16 fragments of the 12 layers into w (nerf::kWeightBytes), biases into b (nerf::kBiasFloats)
int pack_nerf_fragments(const float* const* kernels, const float* const* biases, uint8_t* w0, float* b) {
    uint8_t* w = w0;
    const Seg pe_xyz{kPosEnc, 10, 0, nullptr};
    // enc[0]: posenc(xyz) 63 -> 256
    w += pack_layer_bf16({pe_xyz}, {{kernels[0], biases[0], 256}}, 8, 8, w, b + nerf::kBiasL0);
    for (int l = 1; l <= 7; ++l) {
        float* bl = b + nerf::kBiasL0 + 256 * l;
        if (l == 5) {  // input = concat(y[256], posenc(xyz)[63])   (mlp.py:47-48)
            const Seg pe_skip{kPosEnc, 10, 256, nullptr};
            w += pack_layer_bf16({kHid256, pe_skip}, {{kernels[5], biases[5], 256}}, 8, 24, w, bl);
        } else {
            w += pack_layer_bf16({kHid256}, {{kernels[l], biases[l], 256}}, 8, 16, w, bl);
        }
    }
    // fused [bottleneck (256 cols) | sigma_out (1 col)] on the encoder output
    w += pack_layer_bf16({kHid256}, {{kernels[9], biases[9], 256}, {kernels[8], biases[8], 1}}, 9, 16, w,
                         b + nerf::kBiasBott);
    // rgb_out[0]: concat(bottleneck[256], posenc(view)[27]) -> 128
    const Seg pe_view{kPosEnc, 4, 256, nullptr};
    w += pack_layer_bf16({kHid256, pe_view}, {{kernels[10], biases[10], 128}}, 4, 24, w, b + nerf::kBiasRgb0);
    // rgb_out[1]: 128 -> 3
    w += pack_layer_bf16({kHid128}, {{kernels[11], biases[11], 3}}, 1, 8, w, b + nerf::kBiasRgb1);
    if (w != w0 + nerf::kWeightBytes) return nfx_fail(NFX_EINVAL, "nfx_nerf_pack_weights: internal layout mismatch");
    return NFX_OK;
}

// The bf16 fragments of nerf_geom_layout.hpp's chunk sequence at w0 and its kGeoFloats floats at fl.
int pack_geom_fragments(const float* const* kernels, const float* const* biases, uint8_t* w0, float* fl) {
    std::vector<uint8_t> fwd(nerf::kWeightBytes);
    std::vector<float> fb(nerf::kBiasFloats);
    if (int rc = pack_nerf_fragments(kernels, biases, fwd.data(), fb.data())) return rc;
    // forward: encoder chunks 0..63 and the sigma tile (chunk 72 = 9th tile of the fused [bottleneck | sigma_out])
    const size_t enc_bytes = (size_t)nerf::chunk_frag_offset(64) * 1024;
    memcpy(w0, fwd.data(), enc_bytes);
    memcpy(w0 + enc_bytes, fwd.data() + (size_t)nerf::chunk_frag_offset(72) * 1024, 16 * 1024);
    uint8_t* w = w0 + enc_bytes + 16 * 1024;
    auto dgrad = [&](int l) { w += pack_dgrad({kHid256}, transposed(kernels[l], 0, 256, 256, 256), 256, 16, w); };
    auto igrad = [&](int l, int row0) {   // onto the 64 slots of posenc<10>
        w += pack_dgrad({kHid256}, input_grad_kernel(kernels[l], Seg{kPosEnc, 10, row0, nullptr}, 256), 64, 16, w);
    };
    dgrad(7);
    dgrad(6);
    igrad(5, 256);
    for (int l = 5; l >= 1; --l) dgrad(l);
    igrad(0, 0);
    if (w != w0 + nerf::kGeoWeightBytes) return nfx_fail(NFX_EINVAL, "nfx_nerf_pack_geom_weights: layout mismatch");
    memcpy(fl, fb.data() + nerf::kBiasL0, 8 * 256 * 4);
    memcpy(fl + nerf::kGeoBiasSig, fb.data() + nerf::kBiasBott + 256, 32 * 4);
    // sigma_out kernel in fp32: the bf16 kernel rounds it to bf16 when it forms dZ7, as the forward's packed copy is;
    // the fp32-class kernel splits it into a hi / lo pair
    memcpy(fl + nerf::kGeoWSig, kernels[8], 256 * 4);
    return NFX_OK;
}

// Layer-0 and layer-3 input segments of a width-128 network (layer 3: behind its 128 hidden features) and the two chunk
// sizes.  folded: the inference blob of light visibility, whose posenc10(xyz) rows of both layers sit in the "pre" stream
// (mlp128_layout.hpp); the fp32-class and the training blobs hold the plain network.  slots: brdf_input_slots(z_dim).
struct M128Inputs {
    std::vector<Seg> in0, in3;
    int p0 = 4, p3 = 12;
};
M128Inputs m128_inputs(int in_kind, const int* slots, bool folded) {
    M128Inputs in;
    if (in_kind == NFX_IN_Z_RUSINK) {
        in.in0 = {Seg{kRaw, 2, 0, slots}};
        in.in3 = {Seg{kRaw, 2, 128, slots}};
        return in;
    }
    const bool ldir = in_kind == NFX_IN_XYZ_LDIR;
    if (!(ldir && folded)) {
        in.in0 = {Seg{kPosEnc, 10, 0, nullptr}};
        in.in3 = {Seg{kPosEnc, 10, 128, nullptr}};
    }
    if (ldir) {   // rows 63..89 = posenc4(ldir)
        in.in0.push_back(Seg{kPosEnc, 4, 63, nullptr});
        in.in3.push_back(Seg{kPosEnc, 4, 128 + 63, nullptr});
        if (!folded) in.p0 = 8, in.p3 = 16;
    }
    return in;
}

bool m128_train_kind(int k) { return k == NFX_IN_XYZ || k == NFX_IN_XYZ_LDIR; }
}  // namespace

extern "C" {
// ----------------------------------------------------------------------------------------------- NeRF
size_t nfx_nerf_packed_bytes(int prec) {
    if (prec == NFX_PREC_BF16) return nerf::kBlobBytes;
    if (prec == NFX_PREC_FP32) return (size_t)nerf::kBlobBytes + nerf::kWeightBytes;  // hi | lo | biases
    return 0;
}

int nfx_nerf_pack_weights(const float* const kernels[12], const float* const biases[12], int prec,
                          void* blob, size_t blob_bytes) {
    REQUIRE(kernels && biases && blob, "nfx_nerf_pack_weights: null argument");
    for (int i = 0; i < 12; ++i) REQUIRE(kernels[i] && biases[i], "nfx_nerf_pack_weights: layer %d null", i);
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_pack_weights: bad prec %d", prec);
    REQUIRE(blob_bytes >= nfx_nerf_packed_bytes(prec), "nfx_nerf_pack_weights: blob too small (%zu < %zu)",
            blob_bytes, nfx_nerf_packed_bytes(prec));
    uint8_t* w = static_cast<uint8_t*>(blob);
    if (prec == NFX_PREC_BF16) return pack_nerf_fragments(kernels, biases, w, reinterpret_cast<float*>(w + nerf::kWeightBytes));
    // NFX_PREC_FP32 (nerf_mlp_x3.hip): [fragments of hi = bf16(W) | fragments of lo = bf16(W - hi) | fp32 biases]
    return pack_hi_lo(kernels, kNerfShapes, 12, nerf::kWeightBytes, nerf::kBiasFloats, w,
                      [&](const float* const* k, uint8_t* frags, float* b) { return pack_nerf_fragments(k, biases, frags, b); });
}

size_t nfx_nerf_train_packed_bytes(int prec) { return prec == NFX_PREC_BF16 ? (size_t)nerf::kTrainBlobBytes : 0; }

int nfx_nerf_pack_train_weights(const float* const kernels[12], const float* const biases[12], int prec, void* blob,
                                size_t blob_bytes) {
    REQUIRE(kernels && biases && blob, "nfx_nerf_pack_train_weights: null argument");
    for (int i = 0; i < 12; ++i) REQUIRE(kernels[i] && biases[i], "nfx_nerf_pack_train_weights: layer %d null", i);
    if (prec != NFX_PREC_BF16) return nfx_fail(NFX_ENOSUP, "nfx_nerf_pack_train_weights: only bf16 is built");
    REQUIRE(blob_bytes >= (size_t)nerf::kTrainBlobBytes, "nfx_nerf_pack_train_weights: blob too small (%zu < %d)",
            blob_bytes, nerf::kTrainBlobBytes);
    uint8_t* w0 = static_cast<uint8_t*>(blob);
    // forward fragments + biases: the inference packer's layout, biases moved behind the dgrad fragments
    if (int rc = pack_nerf_fragments(kernels, biases, w0, reinterpret_cast<float*>(w0 + nerf::kTrainWeightBytes))) return rc;
    uint8_t* w = w0 + nerf::kWeightBytes;
    // D1: dR0[128] = Wrgb1[128, 3] dZrgb[3]
    w += pack_dgrad({kHid16}, transposed(kernels[11], 0, 128, 3, 16), 128, 4, w);
    // D2: dBott[256] = Wrgb0[:256, 128] dZr0[128]
    w += pack_dgrad({kHid128}, transposed(kernels[10], 0, 256, 128, 128), 256, 8, w);
    {   // D3: dA7[256] = Wbott[256, 256] dZbott[256] + Wsigma[256, 1] dZsigma  (input rows: 256 + 16 slots, sigma_out's first)
        std::vector<float> t = transposed(kernels[9], 0, 256, 256, 256 + 16);
        memcpy(t.data() + 256 * 256, kernels[8], 256 * 4);
        w += pack_dgrad({kHid256, Seg{kHidden, 16, 256, nullptr}}, t, 256, 20, w);
    }
    for (int l = 7; l >= 1; --l)  // dA_{l-1}[256] = W_l[:256, 256] dZ_l[256]   (enc[5]: the y rows of [y, posenc])
        w += pack_dgrad({kHid256}, transposed(kernels[l], 0, 256, 256, 256), 256, 16, w);
    if (w != w0 + nerf::kTrainWeightBytes) return nfx_fail(NFX_EINVAL, "nfx_nerf_pack_train_weights: layout mismatch");
    return NFX_OK;
}

size_t nfx_nerf_geom_packed_bytes(int prec) {
    if (prec == NFX_PREC_BF16) return (size_t)nerf::kGeoBlobBytes;
    if (prec == NFX_PREC_FP32) return 2 * (size_t)nerf::kGeoWeightBytes + nerf::kGeoFloats * sizeof(float);   // [hi | lo | floats]
    return 0;
}

int nfx_nerf_pack_geom_weights(const float* const kernels[12], const float* const biases[12], int prec, void* blob,
                               size_t blob_bytes) {
    REQUIRE(kernels && biases && blob, "nfx_nerf_pack_geom_weights: null argument");
    for (int i = 0; i < 12; ++i) REQUIRE(kernels[i] && biases[i], "nfx_nerf_pack_geom_weights: layer %d null", i);
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_pack_geom_weights: bad prec %d", prec);
    REQUIRE(blob_bytes >= nfx_nerf_geom_packed_bytes(prec), "nfx_nerf_pack_geom_weights: blob too small (%zu < %zu)",
            blob_bytes, nfx_nerf_geom_packed_bytes(prec));
    uint8_t* w0 = static_cast<uint8_t*>(blob);
    if (prec == NFX_PREC_BF16) return pack_geom_fragments(kernels, biases, w0, reinterpret_cast<float*>(w0 + nerf::kGeoWeightBytes));
    // NFX_PREC_FP32 (nerf_geom_x3.hip): the chunk sequence of hi = bf16(W), then of lo = bf16(W - hi), then the floats
    return pack_hi_lo(kernels, kNerfShapes, 12, nerf::kGeoWeightBytes, nerf::kGeoFloats, w0,
                      [&](const float* const* k, uint8_t* frags, float* fl) { return pack_geom_fragments(k, biases, frags, fl); });
}

// ------------------------------------------------------------------- width-128 surface MLPs, learned BRDF
size_t nfx_mlp128_packed_bytes(int in_kind, int z_dim, int out_dim, int prec) {
    using namespace nfx::m128;
    if (out_dim < 1 || out_dim > 8) return 0;
    if (prec == NFX_PREC_FP32) {   // mlp128_x3.hip: [hi fragments | lo fragments | biases]
        if (in_kind != NFX_IN_XYZ && in_kind != NFX_IN_XYZ_LDIR &&
            !(in_kind == NFX_IN_Z_RUSINK && z_dim >= 1 && z_dim <= kMaxZDim))
            return 0;
        return 2 * (size_t)nfx_mlp128_x3_weight_bytes(in_kind) + kMainBiasFloats * sizeof(float);
    }
    if (prec != NFX_PREC_BF16) return 0;
    if (in_kind == NFX_IN_XYZ) return kMainBytes;
    if (in_kind == NFX_IN_XYZ_LDIR) return (size_t)kPreBytes + kMainBytes;
    if (in_kind == NFX_IN_Z_RUSINK && z_dim >= 1 && z_dim <= kMaxZDim) return kMainBytes;
    return 0;
}

int nfx_mlp128_pack_weights(const float* const kernels[5], const float* const biases[5], int in_kind,
                            int z_dim, int out_dim, int prec, void* blob, size_t blob_bytes) {
    using namespace nfx::m128;
    REQUIRE(kernels && biases && blob, "nfx_mlp128_pack_weights: null argument");
    for (int i = 0; i < 5; ++i) REQUIRE(kernels[i] && biases[i], "nfx_mlp128_pack_weights: layer %d null", i);
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_mlp128_pack_weights: bad prec %d", prec);
    const size_t need = nfx_mlp128_packed_bytes(in_kind, z_dim, out_dim, prec);
    REQUIRE(need != 0, "nfx_mlp128_pack_weights: unsupported configuration (in_kind %d, z_dim %d, out_dim %d)",
            in_kind, z_dim, out_dim);
    REQUIRE(blob_bytes >= need, "nfx_mlp128_pack_weights: blob too small (%zu < %zu)", blob_bytes, need);
    int slots[32];
    brdf_input_slots(z_dim, slots);
    uint8_t* w = static_cast<uint8_t*>(blob);
    if (prec == NFX_PREC_FP32) {   // the plain five layers, the light-visibility input NOT folded
        const int in_dims = in_dims_of(in_kind, z_dim);
        const Shape shapes[5] = {{in_dims, 128}, {128, 128}, {128, 128}, {128 + in_dims, 128}, {128, out_dim}};
        const M128Inputs in = m128_inputs(in_kind, slots, false);
        const size_t wb = nfx_mlp128_x3_weight_bytes(in_kind);
        return pack_hi_lo(kernels, shapes, 5, wb, kMainBiasFloats, w, [&](const float* const* k, uint8_t* frags, float* b) {
            if (pack_m128_ladder(in.in0, in.in3, in.p0, in.p3, k, biases, out_dim, frags, b) != wb)
                return nfx_fail(NFX_EINVAL, "nfx_mlp128_pack_weights: layout mismatch (fp32)");
            return (int)NFX_OK;
        });
    }
    const float* main_biases[5] = {biases[0], biases[1], biases[2], biases[3], biases[4]};
    if (in_kind == NFX_IN_XYZ_LDIR) {   // the "pre" stream; b0 and b3 go with it, folded into the per-point pre-activation
        float* pb = reinterpret_cast<float*>(w + kPreWeightBytes);
        w += pack_layer_bf16({Seg{kPosEnc, 10, 0, nullptr}}, {{kernels[0], biases[0], 128}}, 4, 4, w, pb);
        w += pack_layer_bf16({Seg{kPosEnc, 10, 128, nullptr}}, {{kernels[3], biases[3], 128}}, 4, 4, w, pb + 128);
        w += kPreBiasFloats * 4;
        main_biases[0] = main_biases[3] = nullptr;
    }
    const M128Inputs in = m128_inputs(in_kind, slots, true);
    if (pack_m128_ladder(in.in0, in.in3, in.p0, in.p3, kernels, main_biases, out_dim, w, reinterpret_cast<float*>(w + kMainWeightBytes)) !=
        (size_t)kMainWeightBytes)
        return nfx_fail(NFX_EINVAL, "nfx_mlp128_pack_weights: layout mismatch");
    return NFX_OK;
}

size_t nfx_mlp128_train_packed_bytes(int in_kind) {
    return m128_train_kind(in_kind) ? (size_t)nfx_mlp128_train_blob_bytes(in_kind) : 0;
}

int nfx_mlp128_pack_train_weights(const float* const kernels[5], const float* const biases[5], int in_kind,
                                  int out_dim, int prec, void* blob, size_t blob_bytes) {
    REQUIRE(kernels && biases && blob, "nfx_mlp128_pack_train_weights: null argument");
    for (int i = 0; i < 5; ++i) REQUIRE(kernels[i] && biases[i], "nfx_mlp128_pack_train_weights: layer %d null", i);
    REQUIRE(m128_train_kind(in_kind), "nfx_mlp128_pack_train_weights: in_kind %d has no backward", in_kind);
    REQUIRE(out_dim >= 1 && out_dim <= 8, "nfx_mlp128_pack_train_weights: out_dim %d not in [1, 8]", out_dim);
    if (prec != NFX_PREC_BF16) return nfx_fail(NFX_ENOSUP, "nfx_mlp128_pack_train_weights: only bf16 is built");
    const size_t need = nfx_mlp128_train_packed_bytes(in_kind);
    REQUIRE(blob_bytes >= need, "nfx_mlp128_pack_train_weights: blob too small (%zu < %zu)", blob_bytes, need);
    uint8_t* w = static_cast<uint8_t*>(blob);
    float* b = reinterpret_cast<float*>(w + need - m128::kMainBiasFloats * 4);
    // ---- forward fragments (same dataflow as the inference kernels, un-folded input)
    const M128Inputs in = m128_inputs(in_kind, nullptr, false);
    w += pack_m128_ladder(in.in0, in.in3, in.p0, in.p3, kernels, biases, out_dim, w, b);
    // ---- dgrad fragments: layer l backward = a Dense whose Keras kernel is W_l^T ([out, in])
    // through the out layer: dH3[128] = Wo[128, out] dZo[out]; 16 padded gradient slots
    w += pack_dgrad({kHid16}, transposed(kernels[4], 0, 128, out_dim, 16), 128, 4, w);
    // through L3 (only the h2 rows, its first 128, carry a gradient that is needed), L2, L1
    for (int l = 3; l >= 1; --l) w += pack_dgrad({kHid128}, transposed(kernels[l], 0, 128, 128, 128), 128, 8, w);
    if (w != reinterpret_cast<uint8_t*>(b)) return nfx_fail(NFX_EINVAL, "nfx_mlp128_pack_train_weights: layout mismatch");
    return NFX_OK;
}

size_t nfx_brdf_train_packed_bytes(void) { return (size_t)nfx_brdf_train_blob_bytes(); }

int nfx_brdf_pack_train_weights(const float* const kernels[5], const float* const biases[5], int z_dim, int prec,
                                void* blob, size_t blob_bytes) {
    REQUIRE(kernels && biases && blob, "nfx_brdf_pack_train_weights: null argument");
    for (int i = 0; i < 5; ++i) REQUIRE(kernels[i] && biases[i], "nfx_brdf_pack_train_weights: layer %d null", i);
    REQUIRE(z_dim >= 1 && z_dim <= m128::kMaxZDim, "nfx_brdf_pack_train_weights: z_dim %d unsupported", z_dim);
    if (prec != NFX_PREC_BF16) return nfx_fail(NFX_ENOSUP, "nfx_brdf_pack_train_weights: only bf16 is built");
    const size_t need = nfx_brdf_train_packed_bytes();
    REQUIRE(blob_bytes >= need, "nfx_brdf_pack_train_weights: blob too small (%zu < %zu)", blob_bytes, need);
    int slots[32];
    m128::brdf_input_slots(z_dim, slots);
    uint8_t* w = static_cast<uint8_t*>(blob);
    float* b = reinterpret_cast<float*>(w + need - m128::kMainBiasFloats * 4);
    const M128Inputs in = m128_inputs(NFX_IN_Z_RUSINK, slots, false);
    w += pack_m128_ladder(in.in0, in.in3, in.p0, in.p3, kernels, biases, 1, w, b);
    // through the out layer; W3[128:, :] dZ3 -> the 32 input slots; the hidden-to-hidden dgrads; W0 dZ0 -> the input slots
    w += pack_dgrad({kHid16}, transposed(kernels[4], 0, 128, 1, 16), 128, 4, w);
    w += pack_dgrad({kHid128}, input_grad_kernel(kernels[3], in.in3[0], 128), 32, 8, w);
    for (int l = 3; l >= 1; --l) w += pack_dgrad({kHid128}, transposed(kernels[l], 0, 128, 128, 128), 128, 8, w);
    w += pack_dgrad({kHid128}, input_grad_kernel(kernels[0], in.in0[0], 128), 32, 8, w);
    if (w != reinterpret_cast<uint8_t*>(b)) return nfx_fail(NFX_EINVAL, "nfx_brdf_pack_train_weights: layout mismatch");
    return NFX_OK;
}
}  // extern "C"
