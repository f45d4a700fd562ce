// resize.hpp — what resize.hip and its C-ABI entry (capi_resize.cpp) both need: the launch plan of one antialiased resize
// (the output tile, the channel chunk and the LDS image of one workgroup), a function of the shapes and the input type only.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/nfx.h"

namespace nfx {
namespace rsz {

constexpr int kThreads = 256;
constexpr size_t kLdsBytes = 64 * 1024;       // two workgroups per CU

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int elem_bytes(int in_type) { return in_type == NFX_RESIZE_U8 ? 1 : in_type == NFX_RESIZE_U16 ? 2 : 4; }

// The taps of t consecutive outputs span fewer than (t - 1) scale + 2 support + 1 input positions (include/nfx.h: a tap's
// centre lies strictly within `support` of the output's); one more for the rounding of the fp64 weights at the two ends.
inline int footprint_cap(int n_in, int n_out, int t) {
    const double scale = (double)n_in / (double)n_out, support = scale > 1. ? scale : 1.;
    const double span = floor((double)(t - 1) * scale + 2. * support) + 2.;
    return span < (double)n_in ? (int)span : n_in;
}

struct Plan {
    int ty, tx, cc;            // output rows and columns of a tile, channels of a chunk
    int fr_cap, fc_cap;        // rows and columns of the largest input footprint of a tile
    int mid_pitch, in_pitch;   // elements per footprint row of the horizontal pass's result (float) and of the staged input
    size_t off_wy, off_wx, off_meta, off_in, lds_bytes;
    long long tiles_y, tiles_x;
    int chunks;
};

inline void layout(Plan& p, int h, int w, int c, int oh, int ow, int taps_y, int taps_x, int esize) {
    p.fr_cap = footprint_cap(h, oh, p.ty);
    p.fc_cap = footprint_cap(w, ow, p.tx);
    p.mid_pitch = round_up(p.tx * p.cc, 4);
    p.in_pitch = round_up(p.fc_cap * p.cc, 16 / esize);
    p.off_wy = (size_t)p.fr_cap * p.mid_pitch * sizeof(float);
    p.off_wx = p.off_wy + (size_t)p.ty * taps_y * sizeof(float);
    p.off_meta = p.off_wx + (size_t)p.tx * taps_x * sizeof(float);
    p.off_in = (p.off_meta + (size_t)3 * (p.ty + p.tx) * sizeof(int) + 15) / 16 * 16;
    p.lds_bytes = p.off_in + (size_t)p.fr_cap * p.in_pitch * esize;
    p.tiles_y = (oh + p.ty - 1) / p.ty;
    p.tiles_x = (ow + p.tx - 1) / p.tx;
    p.chunks = (c + p.cc - 1) / p.cc;
}

// Among the tiles whose LDS image fits: the fewest input elements staged per output value (the halo a tile re-reads), then
// the larger channel chunk (longer contiguous runs), then the larger tile.  The smallest candidate (1 x 1 x 4) always fits.
inline Plan plan(int in_type, int h, int w, int c, int oh, int ow, int taps_y, int taps_x) {
    const int esize = elem_bytes(in_type);
    Plan best{};
    double best_cost = -1.;
    const int ccs[5] = {c <= 64 ? c : 64, 32, 16, 8, 4};
    for (int ci = 0; ci < 5; ++ci) {
        const int cc = ccs[ci];
        if (ci > 0 && cc >= ccs[0]) continue;
        for (int ty = 32; ty >= 1; ty >>= 1)
            for (int tx = 64; tx >= 1; tx >>= 1) {
                Plan p{};
                p.ty = ty < oh ? ty : oh;
                p.tx = tx < ow ? tx : ow;
                p.cc = cc;
                layout(p, h, w, c, oh, ow, taps_y, taps_x, esize);
                if (p.lds_bytes > kLdsBytes) continue;
                double cost = (double)p.fr_cap * p.fc_cap / ((double)p.ty * p.tx);
                if ((long long)p.ty * p.tx * p.cc < kThreads) cost *= 2.;      // a tile with less than one value per thread
                if (cc < c && cc * esize < 128) cost *= 128. / (cc * esize);   // a chunk's contiguous run is cc elements
                if (best_cost < 0. || cost < best_cost) {
                    best = p;
                    best_cost = cost;
                }
            }
    }
    return best;
}

}  // namespace rsz
}  // namespace nfx
