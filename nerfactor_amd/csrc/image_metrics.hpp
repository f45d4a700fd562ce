// image_metrics.hpp — what image_metrics.hip and its C-ABI entry (capi_metrics.cpp) both need: the window, the tile of
// window positions one block scores (include/nfx.h's NFX_IMAGE_METRICS_TILE_*), and the number of tiles along an axis.
#pragma once
#include "../../include/nfx.h"

namespace nfx {
namespace imet {

constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kTileY = NFX_IMAGE_METRICS_TILE_Y, kTileX = NFX_IMAGE_METRICS_TILE_X;

// tiles that cover the n - 10 window positions along an axis of n pixels (n >= 11)
inline int tiles_of(int n, int tile) { return (n - kHalo + tile - 1) / tile; }

}  // namespace imet
}  // namespace nfx
