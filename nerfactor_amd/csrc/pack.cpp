// pack.cpp — see pack.hpp.  Pure host C++ (compiled into libnfx.so by hipcc, runs without a GPU).
#include "pack.hpp"

#include <string.h>

namespace nfx {
namespace pack {

uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

const Shape kNerfShapes[12] = {{63, 256},  {256, 256}, {256, 256}, {256, 256}, {256, 256}, {319, 256},
                               {256, 256}, {256, 256}, {256, 1},   {256, 256}, {283, 128}, {128, 3}};

LoKernels lo_kernels(const float* const* kernels, const Shape* shapes, int n) {
    LoKernels lo;
    lo.data.resize(n);
    lo.ptr.resize(n);
    for (int i = 0; i < n; ++i) {
        const size_t cnt = (size_t)shapes[i].rows * shapes[i].cols;
        lo.data[i].resize(cnt);
        for (size_t k = 0; k < cnt; ++k) {
            const uint32_t bits = (uint32_t)f32_to_bf16_rne(kernels[i][k]) << 16;
            float hi;
            memcpy(&hi, &bits, 4);
            lo.data[i][k] = kernels[i][k] - hi;
        }
        lo.ptr[i] = lo.data[i].data();
    }
    return lo;
}

int pack_hi_lo(const float* const* kernels, const Shape* shapes, int n, size_t weight_bytes, int n_floats, uint8_t* blob,
               const PackHalf& pack_half) {
    const LoKernels lo = lo_kernels(kernels, shapes, n);
    std::vector<float> sink(n_floats);
    if (int rc = pack_half(kernels, blob, reinterpret_cast<float*>(blob + 2 * weight_bytes))) return rc;
    return pack_half(lo.ptr.data(), blob + weight_bytes, sink.data());
}

int hidden_feature(int s, int h, int j) { return 32 * (s >> 1) + 16 * (s & 1) + (j & 3) + 8 * (j >> 2) + 4 * h; }

int seg_ksteps(const Seg& s) {
    switch (s.kind) {
        case kHidden: return s.n / 16;
        case kPosEnc: return (3 * s.n + 2 + 7) / 8;
        default: return s.n;
    }
}

int seg_row(const Seg& seg, int s, int h, int j) {
    if (seg.kind == kHidden) return seg.row0 + hidden_feature(s, h, j);
    if (seg.kind == kPosEnc) {
        const int L = seg.n, q = 8 * s + j;
        int e;
        if (q < 3 * L) e = 3 + 6 * (q / 3) + (q % 3) + (h ? 3 : 0);  // embedder.py:38-47 order
        else if (q == 3 * L) e = h ? 2 : 0;
        else if (q == 3 * L + 1) e = h ? -1 : 1;
        else e = -1;
        return e < 0 ? -1 : seg.row0 + e;
    }
    const int r = seg.raw_slots[(s * 2 + h) * 8 + j];
    return r < 0 ? -1 : seg.row0 + r;
}

size_t pack_layer_bf16(const std::vector<Seg>& segs, const std::vector<Src>& srcs, int n_tiles,
                       int chunk_frags, uint8_t* wdst, float* bias_dst) {
    int n_out = 0;
    for (const Src& s : srcs) n_out += s.cols;
    uint16_t* w = reinterpret_cast<uint16_t*>(wdst);
    const size_t chunk_elems = (size_t)chunk_frags * 512;  // 1 KiB = 512 bf16
    memset(wdst, 0, (size_t)n_tiles * chunk_elems * 2);
    for (int t = 0; t < n_tiles; ++t) {
        uint16_t* chunk = w + (size_t)t * chunk_elems;
        int frag = 0;
        for (const Seg& seg : segs) {
            const int ks = seg_ksteps(seg);
            for (int s = 0; s < ks; ++s, ++frag) {
                for (int lane = 0; lane < 64; ++lane) {
                    const int h = lane >> 5, n = lane & 31;
                    const int col = 32 * t + n;
                    if (col >= n_out) continue;
                    // locate the column block
                    int c = col;
                    const Src* src = nullptr;
                    for (const Src& sb : srcs) {
                        if (c < sb.cols) { src = &sb; break; }
                        c -= sb.cols;
                    }
                    for (int j = 0; j < 8; ++j) {
                        const int row = seg_row(seg, s, h, j);
                        if (row < 0) continue;
                        chunk[(size_t)frag * 512 + lane * 8 + j] =
                            f32_to_bf16_rne(src->kernel[(size_t)row * src->cols + c]);
                    }
                }
            }
        }
        for (int n = 0; n < 32; ++n) {
            const int col = 32 * t + n;
            float b = 0.f;
            if (col < n_out) {
                int c = col;
                for (const Src& sb : srcs) {
                    if (c < sb.cols) { b = sb.bias ? sb.bias[c] : 0.f; break; }
                    c -= sb.cols;
                }
            }
            bias_dst[32 * t + n] = b;
        }
    }
    return (size_t)n_tiles * chunk_elems * 2;
}

size_t pack_m128_ladder(const std::vector<Seg>& in0, const std::vector<Seg>& in3, int p0, int p3, const float* const kernels[5],
                        const float* const biases[5], int out_dim, uint8_t* w, float* b) {
    const uint8_t* w0 = w;
    const Seg hid{kHidden, 128, 0, nullptr};
    std::vector<Seg> hid_in3{hid};
    hid_in3.insert(hid_in3.end(), in3.begin(), in3.end());
    w += pack_layer_bf16(in0, {{kernels[0], biases[0], 128}}, 4, p0, w, b);
    w += pack_layer_bf16({hid}, {{kernels[1], biases[1], 128}}, 4, 8, w, b + 128);
    w += pack_layer_bf16({hid}, {{kernels[2], biases[2], 128}}, 4, 8, w, b + 256);
    w += pack_layer_bf16(hid_in3, {{kernels[3], biases[3], 128}}, 4, p3, w, b + 384);
    w += pack_layer_bf16({hid}, {{kernels[4], biases[4], out_dim}}, 1, 8, w, b + 512);
    return w - w0;
}

std::vector<float> transposed(const float* kernel, int row0, int n_rows, int cols, int pad_cols) {
    std::vector<float> t((size_t)pad_cols * n_rows, 0.f);
    for (int r = 0; r < n_rows; ++r)
        for (int c = 0; c < cols; ++c) t[(size_t)c * n_rows + r] = kernel[(size_t)(row0 + r) * cols + c];
    return t;
}

std::vector<float> input_grad_kernel(const float* kernel, const Seg& in, int width) {
    const int ks = seg_ksteps(in), n = 16 * ks;
    std::vector<float> t((size_t)width * n, 0.f);
    for (int s = 0; s < ks; ++s)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 8; ++j) {
                const int row = seg_row(in, s, h, j);
                if (row < 0) continue;
                const int f = hidden_feature(s, h, j);
                for (int k = 0; k < width; ++k) t[(size_t)k * n + f] = kernel[(size_t)row * width + k];
            }
    return t;
}

}  // namespace pack
}  // namespace nfx
