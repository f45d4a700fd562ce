// bwd_tile.hpp — the pieces of a backward tile that the training kernels share, written once:
//   * the masked dgrad epilogue and the register-staged dgrad layer (mlp128_bwd.hip, brdf_bwd.hip);
//   * the set-up of a width-128 row — its network input as B operand, the stores of that input, and dZ_out
//     (mlp128_bwd.hip: both kernels; mlp128_bwd_fused.hip stores nothing, uses dz_out and keeps its operand written out).
// The weight ring of the width-128 kernels is mlp128_bwd_ring.hpp; the NeRF backward's pieces serve one file and stay in it.
#pragma once
#include "feat_store.hpp"
#include "geom.hpp"
#include "mlp128_train_layout.hpp"
#include "mlp_engine.hpp"

namespace nfx {
namespace bwd {

// dH tile -> next dZ: the accumulators where the activation the features belong to (its two k-steps hlo / hhi, B layout) is
// positive, zero elsewhere
__device__ __forceinline__ void relu_gate(const f32x16& acc, const bf16x8& hlo, const bf16x8& hhi, bf16x8& olo, bf16x8& ohi) {
#pragma unroll
    for (int j = 0; j < 8; ++j) olo[j] = (__bf16)((float)hlo[j] > 0.f ? acc[j] : 0.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) ohi[j] = (__bf16)((float)hhi[j] > 0.f ? acc[8 + j] : 0.f);
}

// dgrad layer on the register-staged weight stream: dH^T = W dZ^T (4 tiles of 32 input features, KS k-steps of dZ),
// ReLU-masked by the activation `hact` the features belong to; result = next dZ (bf16, B layout).
template <int KS, int NL_SELF, int NL_NEXT, int NW, int KSA>
__device__ __forceinline__ void dgrad_layer(WStream& ws, int tid, const bf16x8 (&dz)[KSA][1],
                                            const bf16x8 (&hact)[8][1], bf16x8 (&dout)[8][1]) {
    static_for<0, 4>([&](auto T) {
        constexpr int t = decltype(T)::value;
        f32x16 acc[1];
        tile_init<KS, 0, (t == 3 ? NL_NEXT : NL_SELF), NW>(
            ws, tid, [&](f32x16(&a)[1]) { zero_init<1>(a); }, dz, dz, acc);
        relu_gate(acc[0], hact[2 * t][0], hact[2 * t + 1][0], dout[2 * t][0], dout[2 * t + 1][0]);
    });
}

// ---- a width-128 row.  IN_KIND 0: posenc10(xyz_scale*xyz) ; 1: [posenc10(xyz_scale*xyz), posenc4(normalize(lp - xd))]
// The row's network input as B operand `xin`, from the point, the light position `lp` and the point `xd` the direction is taken
// from (IN_KIND 0 reads neither).  pe / pl: the two encodings' own k-steps, for store_row_inputs.
template <int IN_KIND, int KSX>
__device__ __forceinline__ void row_operand(const float (&xyz)[3], float xyz_scale, const float (&lp)[3], const float (&xd)[3],
                                            int h, bf16x8 (&xin)[KSX][1], bf16x8 (&pe)[4][1], bf16x8 (&pl)[2][1]) {
    static_assert(KSX == (IN_KIND == 0 ? 4 : 6), "k-steps of the input");
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = xyz_scale * xyz[k];
    posenc<10, 1>(x, h, 0, pe);
#pragma unroll
    for (int s = 0; s < 4; ++s) xin[s][0] = pe[s][0];
    if constexpr (IN_KIND == 1) {
        float d[3];
        dir_to(lp, xd, d);
        posenc<4, 1>(d, h, 0, pl);
        xin[4][0] = pl[0][0];
        xin[5][0] = pl[1][0];
    }
}
// the stored network input: features 0..62 (+ 63..89), logical Embedder order, and the pads up to the k-step
template <int IN_KIND>
__device__ __forceinline__ void store_row_inputs(const FeatStore& fs, int h, const bf16x8 (&pe)[4][1], const bf16x8 (&pl)[2][1]) {
    store_posenc<10, 4>(fs, 0, h, pe);
    // pad feature 63 — only where nothing else owns the slot: with IN_KIND == 1 feature 63 is ldir.x, written by
    // store_posenc<4, 2>(fs, 63) below from the OTHER lane half; two stores of different lanes to one address
    // have no defined order
    if constexpr (IN_KIND == 0) { if (h == 1) st16(fs, 63, (__bf16)0.f); }
    if constexpr (IN_KIND == 1) {
        store_posenc<4, 2>(fs, 63, h, pl);
        if (h == 1) {  // pad features 90..95
#pragma unroll
            for (int e = 90; e < 96; ++e) st16(fs, e, (__bf16)0.f);
        }
    }
}
// dZ_out = dOut * post_scale * act'(logit) of one output of a row that has it (`on`), zero elsewhere.  Element by element:
// the three kernels keep their own loop over the lane's four outputs (the storing ones store in it), and as a whole k-step
// the function moves instructions of mlp128_bwd_fused_kernel.
__device__ __forceinline__ __bf16 dz_out(float dv, float logit, float post_scale, int out_act, bool on) {
    const float g = dv * post_scale * act_grad(logit, out_act);
    return (__bf16)(on ? g : 0.f);
}

}  // namespace bwd
}  // namespace nfx
