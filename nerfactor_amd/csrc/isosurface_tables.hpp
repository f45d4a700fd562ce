// isosurface_tables.hpp — the tables of marching tetrahedra on the Kuhn split (isosurface.hip), built at
// compile time from the rule of include/nfx.h so that the host entry point (nfx_isosurface_tables) and the kernels read the
// same bytes.  Integer arithmetic only: corners are 0 / 1 vectors, edge midpoints are kept doubled.
#pragma once
#include <stdint.h>

namespace nfx {
namespace iso {

struct Tables {
    int8_t corner[6][4][3];      // corner n of tet t as an offset from the cell's lattice point
    int8_t edge[6][4][4][4];     // [t][a][b], a < b: edge class, then the owner's offset (corner a); -1 elsewhere
    int8_t tri[6][16][2][3][2];  // [t][inside mask][triangle][vertex] = the corner pair (a < b) of its edge; -1 = unused
    uint8_t ntri[6][16];
    uint8_t code[6][16][6];      // the same vertices for the kernel: owner's corner id (4 dx + 2 dy + dz) | class << 3
    uint8_t cid[6][4];           // corner id of corner n of tet t
};

constexpr Tables make_tables() {
    Tables T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int class_of[8] = {-1, 2, 1, 5, 0, 4, 3, 6};   // by 4 dx + 2 dy + dz of the edge's direction
    for (int t = 0; t < 6; ++t) {
        for (int n = 0; n < 4; ++n)
            for (int k = 0; k < 3; ++k) T.corner[t][n][k] = 0;
        T.corner[t][1][perm[t][0]] = 1;
        T.corner[t][2][perm[t][0]] = 1;
        T.corner[t][2][perm[t][1]] = 1;
        for (int k = 0; k < 3; ++k) T.corner[t][3][k] = 1;
        for (int n = 0; n < 4; ++n) T.cid[t][n] = (uint8_t)(4 * T.corner[t][n][0] + 2 * T.corner[t][n][1] + T.corner[t][n][2]);
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                for (int k = 0; k < 4; ++k) T.edge[t][a][b][k] = -1;
                if (a < b) {
                    T.edge[t][a][b][0] = (int8_t)class_of[T.cid[t][b] - T.cid[t][a]];
                    for (int k = 0; k < 3; ++k) T.edge[t][a][b][1 + k] = T.corner[t][a][k];
                }
            }
        for (int m = 0; m < 16; ++m) {
            for (int r = 0; r < 2; ++r)
                for (int v = 0; v < 3; ++v) T.tri[t][m][r][v][0] = T.tri[t][m][r][v][1] = -1;
            for (int v = 0; v < 6; ++v) T.code[t][m][v] = 0;
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
            for (int n = 0; n < 4; ++n) {
                if ((m >> n) & 1)
                    in[n_in++] = n;
                else
                    out[n_out++] = n;
            }
            int pair[2][3][2] = {};
            int n_tri = 0;
            if (n_in == 1 || n_in == 3) {
                const int lone = n_in == 1 ? in[0] : out[0];
                const int* rest = n_in == 1 ? out : in;
                n_tri = 1;
                for (int v = 0; v < 3; ++v) {
                    pair[0][v][0] = lone;
                    pair[0][v][1] = rest[v];
                }
            } else if (n_in == 2) {
                const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                n_tri = 2;
                for (int r = 0; r < 2; ++r)
                    for (int v = 0; v < 3; ++v) {
                        pair[r][v][0] = q[pick[r][v]][0];
                        pair[r][v][1] = q[pick[r][v]][1];
                    }
            }
            T.ntri[t][m] = (uint8_t)n_tri;
            // from the inside corners' centroid to the outside corners', times n_in n_out
            int dir[3] = {0, 0, 0};
            for (int k = 0; k < 3; ++k) {
                for (int n = 0; n < n_out; ++n) dir[k] += n_in * T.corner[t][out[n]][k];
                for (int n = 0; n < n_in; ++n) dir[k] -= n_out * T.corner[t][in[n]][k];
            }
            for (int r = 0; r < n_tri; ++r) {
                int p[3][3] = {};   // doubled midpoints
                for (int v = 0; v < 3; ++v)
                    for (int k = 0; k < 3; ++k) p[v][k] = T.corner[t][pair[r][v][0]][k] + T.corner[t][pair[r][v][1]][k];
                int u[3] = {}, w[3] = {};
                for (int k = 0; k < 3; ++k) {
                    u[k] = p[1][k] - p[0][k];
                    w[k] = p[2][k] - p[0][k];
                }
                const int dot = (u[1] * w[2] - u[2] * w[1]) * dir[0] + (u[2] * w[0] - u[0] * w[2]) * dir[1] +
                                (u[0] * w[1] - u[1] * w[0]) * dir[2];
                if (dot < 0)
                    for (int e = 0; e < 2; ++e) {
                        const int s = pair[r][1][e];
                        pair[r][1][e] = pair[r][2][e];
                        pair[r][2][e] = s;
                    }
                for (int v = 0; v < 3; ++v) {
                    const int a = pair[r][v][0] < pair[r][v][1] ? pair[r][v][0] : pair[r][v][1];
                    const int b = pair[r][v][0] < pair[r][v][1] ? pair[r][v][1] : pair[r][v][0];
                    T.tri[t][m][r][v][0] = (int8_t)a;
                    T.tri[t][m][r][v][1] = (int8_t)b;
                    T.code[t][m][r * 3 + v] = (uint8_t)(T.cid[t][a] | (T.edge[t][a][b][0] << 3));
                }
            }
        }
    }
    return T;
}

}  // namespace iso
}  // namespace nfx
