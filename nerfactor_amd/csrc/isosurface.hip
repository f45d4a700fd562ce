// isosurface.hip — marching tetrahedra on a scalar lattice (the rules are include/nfx.h's): the
// iso-surface of field[nx, ny, nz] (z fastest) as indexed triangles, every vertex once.
//
// One thread per lattice point p = (a ny + b) nz + c, z along the lanes: the point owns the vertices of its up to 7 edges
// (classes 0..6, to p + (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)) and the triangles of the cell whose lowest
// corner it is.  Both passes load the same 8 corners; neighbouring lanes share their cache lines.
//
//   count: per point the 7-bit crossing mask and the cell's triangle count (one byte each, kept in the workspace), summed per
//          1024 points; rowsel's one-workgroup scan over the block sums (vertices, then triangles: the totals land in words
//          0 and 1); then every point's own exclusive offsets = its block's offset + the points before it inside the block.
//   emit:  vertex (p, class) is row voff[p] + popcount(mask[p] below class); a triangle names the vertex of an edge by its
//          owner's offset and mask, read from the workspace.  Nothing but plain stores: the output is a function of the inputs.
//
// The block sums are int32 like the rest of rowsel: a sum that passes 2^31 shows as a negative offset (a block adds at most
// 12 288), which sets word 2 of the workspace; emit also bounds every store by the counts it was given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "isosurface_tables.hpp"
#include "launchers.hpp"
#include "rowsel.hpp"

namespace nfx {
namespace iso {

constexpr Tables kTab = make_tables();
constexpr int kBlockPts = rowsel::kBlockRows;
constexpr int kMaxBlocks = 256 * 8;   // 8 workgroups of 256 threads per CU; the rest of the lattice is strided over

// workspace (int32 words): [nv, nf, overflow, pad][vertex block sums, padded to 4][triangle block sums, padded to 4]
// [voff: n, padded to 4][toff: n, padded to 4], then bytes [mask: n, padded to 4][tcnt: n, padded to 4]
struct Layout {
    long long nb, nbp, np;
    __host__ __device__ explicit Layout(long long n) : nb((n + kBlockPts - 1) / kBlockPts), nbp((nb + 3) / 4 * 4), np((n + 3) / 4 * 4) {}
    __host__ __device__ long long words() const { return 4 + 2 * nbp + 2 * np + 2 * (np / 4); }
    template <class T> __host__ __device__ T* vblk(T* ws) const { return ws + 4; }
    template <class T> __host__ __device__ T* tblk(T* ws) const { return ws + 4 + nbp; }
    template <class T> __host__ __device__ T* voff(T* ws) const { return ws + 4 + 2 * nbp; }
    template <class T> __host__ __device__ T* toff(T* ws) const { return ws + 4 + 2 * nbp + np; }
    __host__ __device__ uint8_t* mask(int* ws) const { return reinterpret_cast<uint8_t*>(ws + 4 + 2 * nbp + 2 * np); }
    __host__ __device__ const uint8_t* mask(const int* ws) const { return reinterpret_cast<const uint8_t*>(ws + 4 + 2 * nbp + 2 * np); }
    __host__ __device__ uint8_t* tcnt(int* ws) const { return mask(ws) + np; }
};

struct Lattice {
    const float* field;
    int nx, ny, nz;
    unsigned n;
    float iso;
};

// corner id 4 dx + 2 dy + dz of the far end of an edge of class 0..6
__device__ __forceinline__ constexpr int corner_of_class(int cl) {
    constexpr int c[7] = {4, 2, 1, 6, 5, 3, 7};
    return c[cl];
}

struct Corners {
    float f[8];        // by corner id; 0 where the corner does not exist
    unsigned exist;    // bit per corner id
    unsigned in;       // exists and field > iso
    int a, b, c;
};

__device__ __forceinline__ Corners load_corners(const Lattice& L, unsigned p) {
    Corners k;
    k.c = (int)(p % (unsigned)L.nz);
    const unsigned row = p / (unsigned)L.nz;
    k.b = (int)(row % (unsigned)L.ny);
    k.a = (int)(row / (unsigned)L.ny);
    const bool ex = k.a + 1 < L.nx, ey = k.b + 1 < L.ny, ez = k.c + 1 < L.nz;
    const unsigned sx = (unsigned)L.ny * (unsigned)L.nz, sy = (unsigned)L.nz;
    k.exist = 0;
    k.in = 0;
#pragma unroll
    for (int id = 0; id < 8; ++id) {
        const bool e = (!(id & 4) || ex) && (!(id & 2) || ey) && (!(id & 1) || ez);
        const float v = e ? L.field[p + ((id & 4) ? sx : 0u) + ((id & 2) ? sy : 0u) + (unsigned)(id & 1)] : 0.f;
        k.f[id] = v;
        k.exist |= (unsigned)e << id;
        k.in |= (unsigned)(e && v > L.iso) << id;
    }
    return k;
}

// bit `class` set: the owned edge of that class exists and its ends differ in inside-ness
__device__ __forceinline__ unsigned crossing_mask(const Corners& k) {
    const unsigned differ = k.exist & (k.in ^ ((k.in & 1u) ? 0xffu : 0u));
    unsigned m = 0;
#pragma unroll
    for (int cl = 0; cl < 7; ++cl) m |= ((differ >> corner_of_class(cl)) & 1u) << cl;
    return m;
}

// the 4-bit inside mask of tet t (bit n = corner c_n)
__device__ __forceinline__ unsigned tet_mask(unsigned in, int t) {
    unsigned m = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) m |= ((in >> kTab.cid[t][n]) & 1u) << n;
    return m;
}

__device__ __forceinline__ int triangles_of(unsigned m4) {
    const int pc = __popc(m4);
    return pc == 2 ? 2 : (pc & 1);
}

__device__ __forceinline__ int cell_triangles(const Corners& k) {
    if (!((k.exist >> 7) & 1u)) return 0;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) n += triangles_of(tet_mask(k.in, t));
    return n;
}

// vertices in the low half, triangles in the high half: a block of 1024 points has at most 7168 and 12 288
__global__ __launch_bounds__(256) void count_kernel(Lattice L, int* __restrict__ ws) {
    __shared__ int s[4];
    const Layout lay(L.n);
    int* vblk = lay.vblk(ws);
    int* tblk = lay.tblk(ws);
    uint8_t* mask = lay.mask(ws);
    uint8_t* tcnt = lay.tcnt(ws);
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) ws[2] = ws[3] = 0;
    for (long long blk = blockIdx.x; blk < lay.nb; blk += gridDim.x) {
        int sum = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = blk * kBlockPts + r * 256 + tid;
            if (p < (long long)L.n) {
                const Corners k = load_corners(L, (unsigned)p);
                const unsigned m = crossing_mask(k);
                const int t = cell_triangles(k);
                mask[p] = (uint8_t)m;
                tcnt[p] = (uint8_t)t;
                sum += __popc(m) | (t << 16);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if ((tid & 63) == 0) s[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) {
            const int total = (s[0] + s[1]) + (s[2] + s[3]);
            vblk[blk] = total & 0xffff;
            tblk[blk] = total >> 16;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void offsets_kernel(unsigned n, int* __restrict__ ws) {
    __shared__ int s[16];
    const Layout lay(n);
    const int* vblk = lay.vblk(ws);
    const int* tblk = lay.tblk(ws);
    int* voff = lay.voff(ws);
    int* toff = lay.toff(ws);
    const uint8_t* mask = lay.mask(ws);
    const uint8_t* tcnt = lay.tcnt(ws);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0 && (ws[0] < 0 || ws[1] < 0)) ws[2] = 1;
    for (long long blk = blockIdx.x; blk < lay.nb; blk += gridDim.x) {
        int own[4], incl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = blk * kBlockPts + r * 256 + tid;
            own[r] = p < (long long)n ? (__popc((unsigned)mask[p]) | ((int)tcnt[p] << 16)) : 0;
            int x = own[r];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            incl[r] = x;
            if (lane == 63) s[r * 4 + wave] = x;
        }
        __syncthreads();
        const int bv = vblk[blk], bt = tblk[blk];
        if (tid == 0 && (bv < 0 || bt < 0)) ws[2] = 1;
        int before = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k == wave) {
                    const long long p = blk * kBlockPts + r * 256 + tid;
                    if (p < (long long)n) {
                        const int e = before + incl[r] - own[r];
                        voff[p] = bv + (e & 0xffff);
                        toff[p] = bt + (e >> 16);
                    }
                }
                before += s[r * 4 + k];
            }
        }
        __syncthreads();
    }
}

struct Frame {
    float origin[3], spacing[3];
};

__global__ __launch_bounds__(256) void emit_kernel(Lattice L, Frame fr, const int* __restrict__ ws, unsigned nv, unsigned nf,
                                                   float* __restrict__ vertices, int* __restrict__ faces) {
    const Layout lay(L.n);
    const int* voff = lay.voff(ws);
    const int* toff = lay.toff(ws);
    const uint8_t* mask = lay.mask(ws);
    const unsigned sx = (unsigned)L.ny * (unsigned)L.nz, sy = (unsigned)L.nz;
    for (long long pp = (long long)blockIdx.x * 256 + threadIdx.x; pp < (long long)L.n; pp += (long long)gridDim.x * 256) {
        const unsigned p = (unsigned)pp;
        const Corners k = load_corners(L, p);
        const unsigned m = crossing_mask(k);
        if (m) {
            const int idx[3] = {k.a, k.b, k.c};
            float lo[3], hi[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = fr.origin[d] + (float)idx[d] * fr.spacing[d];
                hi[d] = fr.origin[d] + (float)(idx[d] + 1) * fr.spacing[d];
            }
            unsigned row = (unsigned)voff[p];
#pragma unroll
            for (int cl = 0; cl < 7; ++cl) {
                if ((m >> cl) & 1u) {
                    const int id = corner_of_class(cl);
                    const float t = (L.iso - k.f[0]) / (k.f[id] - k.f[0]);
                    if (row < nv) {
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            const float q = ((id >> (2 - d)) & 1) ? hi[d] : lo[d];
                            vertices[(size_t)row * 3 + d] = lo[d] + t * (q - lo[d]);
                        }
                    }
                    ++row;
                }
            }
        }
        if (((k.exist >> 7) & 1u) && k.in != 0u && k.in != 0xffu) {   // a cell with corners on both sides: the others have no triangle
            unsigned tri = (unsigned)toff[p];
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const unsigned m4 = tet_mask(k.in, t);
                const int nt = triangles_of(m4);
                for (int r = 0; r < nt; ++r) {
                    if (tri < nf) {
#pragma unroll
                        for (int v = 0; v < 3; ++v) {
                            const unsigned code = kTab.code[t][m4][r * 3 + v];
                            const unsigned q = p + ((code & 4u) ? sx : 0u) + ((code & 2u) ? sy : 0u) + (code & 1u);
                            const unsigned below = (1u << (code >> 3)) - 1u;
                            faces[(size_t)tri * 3 + v] = voff[q] + __popc((unsigned)mask[q] & below);
                        }
                    }
                    ++tri;
                }
            }
        }
    }
}

inline unsigned grid_for(long long work_items, int per_block) {
    const long long nb = (work_items + per_block - 1) / per_block;
    return (unsigned)(nb < kMaxBlocks ? nb : kMaxBlocks);
}

}  // namespace iso
}  // namespace nfx

extern "C" size_t nfx_isosurface_ws_bytes(long long n_pts) {
    return n_pts <= 0 ? 0 : (size_t)nfx::iso::Layout(n_pts).words() * sizeof(int);
}

extern "C" void nfx_isosurface_host_tables(int8_t* tri, int8_t* edge) {
    constexpr nfx::iso::Tables T = nfx::iso::make_tables();
    const int8_t* t = &T.tri[0][0][0][0][0];
    for (size_t i = 0; i < sizeof T.tri; ++i) tri[i] = t[i];
    const int8_t* e = &T.edge[0][0][0][0];
    for (size_t i = 0; i < sizeof T.edge; ++i) edge[i] = e[i];
}

extern "C" int nfx_launch_isosurface_count(const float* field, int nx, int ny, int nz, float iso, void* ws, hipStream_t st) {
    using namespace nfx::iso;
    const long long n = (long long)nx * ny * nz;
    const Lattice L{field, nx, ny, nz, (unsigned)n, iso};
    const Layout lay(n);
    int* w = static_cast<int*>(ws);
    const dim3 grid(grid_for(n, kBlockPts));
    hipLaunchKernelGGL(count_kernel, grid, dim3(256), 0, st, L, w);
    if (int rc = nfx::rowsel::launch_scan(lay.vblk(w), (int)lay.nb, w + 0, st)) return rc;
    if (int rc = nfx::rowsel::launch_scan(lay.tblk(w), (int)lay.nb, w + 1, st)) return rc;
    hipLaunchKernelGGL(offsets_kernel, grid, dim3(256), 0, st, (unsigned)n, w);
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_isosurface_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin, const float* spacing,
                                          const void* ws, int nv, int nf, float* vertices, int* faces, hipStream_t st) {
    using namespace nfx::iso;
    const long long n = (long long)nx * ny * nz;
    const Lattice L{field, nx, ny, nz, (unsigned)n, iso};
    Frame fr;
    for (int k = 0; k < 3; ++k) {
        fr.origin[k] = origin[k];
        fr.spacing[k] = spacing[k];
    }
    hipLaunchKernelGGL(emit_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, L, fr, static_cast<const int*>(ws), (unsigned)nv, (unsigned)nf,
                       vertices, faces);
    return (int)hipGetLastError();
}
