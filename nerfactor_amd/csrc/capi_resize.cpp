// capi_resize.cpp — C-ABI entry points of the antialiased resize (include/nfx.h, resize.hip): the host-only table of one
// axis and the checked launch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "capi_common.hpp"
#include "resize.hpp"

namespace {
// fp64, every operation rounded on its own (the build has no contraction): include/nfx.h states this order
inline double tap_weight(int x, double centre, double support) {
    const double w = 1. - fabs(((double)x + 0.5) - centre) / support;
    return w > 0. ? w : 0.;
}
}  // namespace

extern "C" {
int nfx_resize_axis_table(int n_in, int n_out, int32_t* first, int32_t* count, float* weights, int max_taps) {
    REQUIRE(n_in >= 1 && n_in <= NFX_RESIZE_MAX_SIDE && n_out >= 1 && n_out <= NFX_RESIZE_MAX_SIDE,
            "nfx_resize_axis_table: n_in = %d, n_out = %d (1 .. %d each)", n_in, n_out, NFX_RESIZE_MAX_SIDE);
    const bool fill = first || count || weights;
    REQUIRE(!fill || (first && count && weights), "nfx_resize_axis_table: first, count and weights are all given or all null");
    REQUIRE(!fill || max_taps >= 1, "nfx_resize_axis_table: max_taps = %d (at least 1)", max_taps);
    const double scale = (double)n_in / (double)n_out, support = scale > 1. ? scale : 1.;
    int largest = 0;
    for (int i = 0; i < n_out; ++i) {
        const double centre = ((double)i + 0.5) * scale;
        // every tap lies within `support` of the centre: scan two positions further on either side
        int lo = (int)floor(centre - support) - 2, hi = (int)ceil(centre + support) + 2;
        if (lo < 0) lo = 0;
        if (hi > n_in - 1) hi = n_in - 1;
        while (lo <= hi && !(tap_weight(lo, centre, support) > 0.)) ++lo;
        int n = 0;
        double sum = 0.;
        while (lo + n <= hi && tap_weight(lo + n, centre, support) > 0.) {
            const double w = tap_weight(lo + n, centre, support);
            sum = n ? sum + w : w;
            ++n;
        }
        REQUIRE(n >= 1, "nfx_resize_axis_table: output %d of %d -> %d has no tap", i, n_in, n_out);
        if (n > largest) largest = n;
        if (!fill) continue;
        REQUIRE(n <= max_taps, "nfx_resize_axis_table: output %d of %d -> %d has %d taps, max_taps = %d", i, n_in, n_out, n, max_taps);
        first[i] = lo;
        count[i] = n;
        for (int k = 0; k < max_taps; ++k)
            weights[(size_t)i * max_taps + k] = k < n ? (float)(tap_weight(lo + k, centre, support) / sum) : 0.f;
    }
    return largest;
}

int nfx_resize_antialias(const void* in, int in_type, int64_t batch, int h, int w, int c, float in_scale, const int32_t* first_y,
                         const int32_t* count_y, const float* weights_y, int taps_y, const int32_t* first_x, const int32_t* count_x,
                         const float* weights_x, int taps_x, void* out, int out_uint8, int oh, int ow, void* stream) {
    REQUIRE(in_type == NFX_RESIZE_U8 || in_type == NFX_RESIZE_U16 || in_type == NFX_RESIZE_F32,
            "nfx_resize_antialias: in_type = %d (0: uint8, 1: uint16, 2: float32)", in_type);
    REQUIRE(batch >= 1 && batch <= 65535, "nfx_resize_antialias: batch = %lld images (1 .. 65535)", (long long)batch);
    REQUIRE(h >= 1 && w >= 1 && oh >= 1 && ow >= 1 && h <= NFX_RESIZE_MAX_SIDE && w <= NFX_RESIZE_MAX_SIDE &&
                oh <= NFX_RESIZE_MAX_SIDE && ow <= NFX_RESIZE_MAX_SIDE,
            "nfx_resize_antialias: %d x %d -> %d x %d pixels (1 .. %d each)", h, w, oh, ow, NFX_RESIZE_MAX_SIDE);
    REQUIRE((long long)h <= 16ll * oh && (long long)w <= 16ll * ow,
            "nfx_resize_antialias: %d x %d -> %d x %d shrinks an axis by more than 16 (more than %d taps)", h, w, oh, ow,
            NFX_RESIZE_MAX_TAPS);
    REQUIRE(c >= 1 && c <= NFX_RESIZE_MAX_CHANNELS, "nfx_resize_antialias: c = %d channels (1 .. %d)", c, NFX_RESIZE_MAX_CHANNELS);
    REQUIRE(taps_y >= 1 && taps_y <= NFX_RESIZE_MAX_TAPS && taps_x >= 1 && taps_x <= NFX_RESIZE_MAX_TAPS,
            "nfx_resize_antialias: taps_y = %d, taps_x = %d (1 .. %d)", taps_y, taps_x, NFX_RESIZE_MAX_TAPS);
    REQUIRE(in && out && first_y && count_y && weights_y && first_x && count_x && weights_x, "nfx_resize_antialias: null pointer");
    if (!ALIGNED(in, (size_t)nfx::rsz::elem_bytes(in_type)) || !ALIGNED(out, out_uint8 ? 1 : 4) || !ALIGNED(first_y, 4) ||
        !ALIGNED(count_y, 4) || !ALIGNED(weights_y, 4) || !ALIGNED(first_x, 4) || !ALIGNED(count_x, 4) || !ALIGNED(weights_x, 4))
        return nfx_fail(NFX_EALIGN, "nfx_resize_antialias: images must be aligned to their element, the tables to 4 bytes");
    const nfx::rsz::Plan p = nfx::rsz::plan(in_type, h, w, c, oh, ow, taps_y, taps_x);
    REQUIRE(p.ty >= 1 && p.lds_bytes <= nfx::rsz::kLdsBytes, "nfx_resize_antialias: no tile of %d x %d -> %d x %d x %d fits", h, w, oh, ow, c);
    REQUIRE(p.tiles_y * p.tiles_x <= 2147483647ll, "nfx_resize_antialias: %lld x %lld tiles of %d x %d pixels per image (at most 2^31 - 1)",
            p.tiles_y, p.tiles_x, p.ty, p.tx);
    return nfx_hip_result(nfx_launch_resize_antialias(in, in_type, (int)batch, h, w, c, in_scale, first_y, count_y, weights_y, taps_y,
                                                      first_x, count_x, weights_x, taps_x, out, out_uint8, oh, ow, (hipStream_t)stream),
                          "resize_antialias");
}
}
