// capi_metrics.cpp — C-ABI entry points of the image metrics (include/nfx.h, image_metrics.hip).
#include <hip/hip_runtime.h>
#include <math.h>

#include "capi_common.hpp"
#include "image_metrics.hpp"

namespace {
bool shape_ok(int64_t batch, int h, int w, int c) {
    return batch >= 1 && h >= nfx::imet::kWin && w >= nfx::imet::kWin && (c == 1 || c == 3) &&
           (long long)h * w <= NFX_IMAGE_METRICS_MAX_PIXELS && batch <= 65535;
}
int scored_channels(int c, int luma) { return (luma && c == 3) ? 1 : c; }
}  // namespace

extern "C" {
size_t nfx_image_metrics_workspace_bytes(int64_t batch, int h, int w, int c, int luma) {
    using namespace nfx::imet;
    if (!shape_ok(batch, h, w, c) || batch * scored_channels(c, luma) > 65535) return 0;
    return (size_t)batch * scored_channels(c, luma) * tiles_of(h, kTileY) * tiles_of(w, kTileX) * 4 * sizeof(int64_t);
}

int nfx_image_metrics(const void* a, const void* b, int is_float, int64_t batch, int h, int w, int c, double max_val, int luma,
                      const uint8_t* mask, double* ssim_map, const double* host_weights, int64_t* totals, void* workspace,
                      size_t workspace_bytes, void* stream) {
    REQUIRE(h >= 11 && w >= 11, "nfx_image_metrics: images of %d x %d pixels, the 11 x 11 window needs at least 11 x 11", h, w);
    REQUIRE(c == 1 || c == 3, "nfx_image_metrics: c = %d channels (1 or 3)", c);
    REQUIRE((long long)h * w <= NFX_IMAGE_METRICS_MAX_PIXELS, "nfx_image_metrics: %d x %d = %lld pixels per image, at most %lld",
            h, w, (long long)h * w, (long long)NFX_IMAGE_METRICS_MAX_PIXELS);
    const int cp = scored_channels(c, luma);
    REQUIRE(batch >= 1 && batch * cp <= 65535, "nfx_image_metrics: batch = %lld images of %d scored channels (1 <= batch, batch * channels <= 65535)",
            (long long)batch, cp);
    REQUIRE(max_val > 0. && isfinite(max_val), "nfx_image_metrics: max_val = %g (positive and finite)", max_val);
    REQUIRE(is_float == 0 || is_float == 1, "nfx_image_metrics: is_float = %d (0: uint8, 1: float32)", is_float);
    REQUIRE(a && b && host_weights && totals && workspace, "nfx_image_metrics: null pointer");
    const size_t need = nfx_image_metrics_workspace_bytes(batch, h, w, c, luma);
    REQUIRE(workspace_bytes >= need, "nfx_image_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const size_t elem = is_float ? 4 : 1;
    if (!ALIGNED(a, elem) || !ALIGNED(b, elem) || !ALIGNED(ssim_map, 8) || !ALIGNED(totals, 8) || !ALIGNED(workspace, 8))
        return nfx_fail(NFX_EALIGN, "nfx_image_metrics: images must be aligned to their element, ssim_map, totals and workspace to 8 bytes");
    return nfx_hip_result(nfx_launch_image_metrics(a, b, is_float, (int)batch, h, w, c, cp, max_val, mask, ssim_map, host_weights,
                                                   (long long*)totals, (long long*)workspace, (hipStream_t)stream),
                          "image_metrics");
}
}
