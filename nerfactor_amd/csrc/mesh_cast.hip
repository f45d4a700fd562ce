// mesh_cast.hip — rays against a triangle mesh (reference: data_gen/dtu_mvs/surf_from_mvs.py, which casts camera rays and one
// shadow ray per (surface point, light) with trimesh on Embree).  The tree is mesh_bvh.hpp's blob.
//
// Traversal.  Stackless: node <- index + 1 into an inner node whose box is hit, node <- skip otherwise and after a leaf.
// Links only point forward, the loop also counts its steps against n_nodes, and every link and triangle range read from
// the blob is clamped to the header's counts, so a damaged blob ends and stays inside the blob.  No per-lane array is
// indexed at run time (that would be scratch memory): the axes of the shear are picked with selects.
//
// Ray / triangle (Woop, Benthin, Wald 2013), all fp32, no fused multiply-add (-ffp-contract=off), IEEE division:
//   kz = the axis of the largest |d| (the lower axis on a tie), kx = kz + 1, ky = kx + 1 (mod 3), swapped when d[kz] < 0
//   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
//   A = v0 - o, B = v1 - o, C = v2 - o
//   Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz]      (B, C alike)
//   U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax
//   if U, V or W is exactly 0: all three again with the four products and the difference in fp64, rounded to fp32
//   miss if one of them is < 0 and one is > 0;  det = (U + V) + W, miss if det == 0
//   T = (U * (Sz * A[kz]) + V * (Sz * B[kz])) + W * (Sz * C[kz]);  t = T / det;  hit iff t > 0
// Both faces count.  The closest hit is the smallest t, the smaller ORIGINAL index at equal t — a function of the
// triangle set, not of the tree or the order of the walk.
//
// Ray / box.  With D = the largest |corner - o| over the box's two corners and three axes, the slabs are the box grown by
// s = 2^-18 D on every side: a = ((lo - o) - s) / d, b = ((hi - o) + s) / d per axis (as products with 1 / d; fminf / fmaxf
// drop the NaN of 0 * inf), enter = max(min(a, b), 0), leave = min(max(a, b)); the box is visited iff enter <= leave and,
// for the closest hit, enter <= the best t so far.  The triangle test works on vertices moved by at most a few 2^-24 D
// across the ray (the rounding of v - o and of the shear) and its t is a convex combination of the vertices' Sz * (v - o)[kz],
// so an accepted hit lies inside the box grown by a few 2^-24 D: s is 64 roundings wide and covers that and the slab
// arithmetic's own rounding.
//
// nfx_mesh_lvis.  One wave per (64 rows, 64 lights) tile, lane = row: the 64 shadow rays of a step go to the same light
// and are nearly parallel.  A lane keeps its 64 results as one bit each; the tile is written light-major per row, one row per
// step, 64 consecutive floats per store.  No LDS, no workspace, no atomics.
#include "launchers.hpp"
#include "mesh_bvh.hpp"

namespace nfx {
namespace mesh {

constexpr float kInf = __builtin_inff();
constexpr float kSlack = 1.0f / 262144.0f;   // 2^-18

__device__ __forceinline__ float pick(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < kInf && fabsf(y) < kInf && fabsf(z) < kInf; }

struct Ray {
    float ox, oy, oz;
    float ix, iy, iz;   // 1 / d per axis
    float sx, sy, sz;
    int kx, ky, kz;
    bool ok;            // finite origin and direction, direction not zero

    __device__ __forceinline__ Ray(float ox_, float oy_, float oz_, float dx, float dy, float dz) : ox(ox_), oy(oy_), oz(oz_) {
        ok = finite3(ox, oy, oz) && finite3(dx, dy, dz) && (dx != 0.0f || dy != 0.0f || dz != 0.0f);
        kz = 0;
        float m = fabsf(dx);
        if (fabsf(dy) > m) kz = 1, m = fabsf(dy);
        if (fabsf(dz) > m) kz = 2;
        kx = kz == 2 ? 0 : kz + 1;
        ky = kx == 2 ? 0 : kx + 1;
        const float dzk = pick(kz, dx, dy, dz);
        if (dzk < 0.0f) {
            const int t = kx;
            kx = ky;
            ky = t;
        }
        sx = pick(kx, dx, dy, dz) / dzk;
        sy = pick(ky, dx, dy, dz) / dzk;
        sz = 1.0f / dzk;
        ix = 1.0f / dx;
        iy = 1.0f / dy;
        iz = 1.0f / dz;
    }

    // t of the hit with the triangle, or a value that is not > 0
    __device__ __forceinline__ float hit(const float4& p0, const float4& p1, const float4& p2) const {
        const float a0 = p0.x - ox, a1 = p0.y - oy, a2 = p0.z - oz;
        const float b0 = p1.x - ox, b1 = p1.y - oy, b2 = p1.z - oz;
        const float c0 = p2.x - ox, c1 = p2.y - oy, c2 = p2.z - oz;
        const float az = pick(kz, a0, a1, a2), bz = pick(kz, b0, b1, b2), cz = pick(kz, c0, c1, c2);
        const float ax = pick(kx, a0, a1, a2) - sx * az, ay = pick(ky, a0, a1, a2) - sy * az;
        const float bx = pick(kx, b0, b1, b2) - sx * bz, by = pick(ky, b0, b1, b2) - sy * bz;
        const float cx = pick(kx, c0, c1, c2) - sx * cz, cy = pick(ky, c0, c1, c2) - sy * cz;
        float u = cx * by - cy * bx, v = ax * cy - ay * cx, w = bx * ay - by * ax;
        if (u == 0.0f || v == 0.0f || w == 0.0f) {
            u = (float)((double)cx * (double)by - (double)cy * (double)bx);
            v = (float)((double)ax * (double)cy - (double)ay * (double)cx);
            w = (float)((double)bx * (double)ay - (double)by * (double)ax);
        }
        if ((u < 0.0f || v < 0.0f || w < 0.0f) && (u > 0.0f || v > 0.0f || w > 0.0f)) return -1.0f;
        const float det = (u + v) + w;
        if (det == 0.0f) return -1.0f;
        const float tt = (u * (sz * az) + v * (sz * bz)) + w * (sz * cz);
        return tt / det;
    }

    // does the ray cross the grown box, and where it enters it
    __device__ __forceinline__ bool enter(const float4& n0, const float4& n1, float& tn) const {
        const float lx = n0.x - ox, ly = n0.y - oy, lz = n0.z - oz, hx = n1.x - ox, hy = n1.y - oy, hz = n1.z - oz;
        const float dmax = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
        const float s = kSlack * dmax;
        const float xa = (lx - s) * ix, xb = (hx + s) * ix, ya = (ly - s) * iy, yb = (hy + s) * iy, za = (lz - s) * iz, zb = (hz + s) * iz;
        tn = fmaxf(fmaxf(fminf(xa, xb), fminf(ya, yb)), fmaxf(fminf(za, zb), 0.0f));
        const float tf = fminf(fminf(fmaxf(xa, xb), fmaxf(ya, yb)), fmaxf(za, zb));
        return tn <= tf;
    }
};

struct Tree {
    const float4* nodes;   // two per node
    const float4* tris;    // three per triangle
    int n_nodes, n_tris;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ANY = false: the closest hit (t, original index; +inf, -1 for none).  ANY = true: returns at the first accepted triangle.
template <bool ANY>
__device__ __forceinline__ bool walk(const Tree& tr, const Ray& r, float& best_t, int& best_tri) {
    best_t = kInf;
    best_tri = -1;
    if (!r.ok) return false;
    int node = 0;
    for (int step = 0; step < tr.n_nodes && node < tr.n_nodes; ++step) {
        const float4 n0 = tr.nodes[2 * (long long)node], n1 = tr.nodes[2 * (long long)node + 1];
        const int skip = clampi(__float_as_int(n0.w), node + 1, tr.n_nodes);
        const int first = __float_as_int(n1.w);
        float tn;
        if (!(r.enter(n0, n1, tn) && tn <= best_t)) {          // missed, or farther than the best hit (a hit at the same t may have the smaller index)
            node = skip;
            continue;
        }
        if (first < 0) {
            node = node + 1;
            continue;
        }
        const int end = clampi(subtree_first(__float_as_int(tr.nodes[2 * (long long)skip + 1].w)), 0, tr.n_tris);
        for (int i = clampi(first, 0, tr.n_tris); i < end; ++i) {
            const float4 p0 = tr.tris[3 * (long long)i], p1 = tr.tris[3 * (long long)i + 1], p2 = tr.tris[3 * (long long)i + 2];
            const float t = r.hit(p0, p1, p2);
            if (t > 0.0f) {
                if (ANY) return true;
                const int orig = __float_as_int(p0.w);
                if (t < best_t || (t == best_t && orig < best_tri)) {
                    best_t = t;
                    best_tri = orig;
                }
            }
        }
        node = skip;
    }
    return best_tri >= 0;
}

__global__ __launch_bounds__(256) void mesh_cast_kernel(Tree tr, const float* __restrict__ rayo, const float* __restrict__ rayd, long long n,
                                                        float* __restrict__ out_t, int* __restrict__ out_tri) {
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) {
        const Ray r(rayo[i * 3], rayo[i * 3 + 1], rayo[i * 3 + 2], rayd[i * 3], rayd[i * 3 + 1], rayd[i * 3 + 2]);
        float t;
        int tri;
        walk<false>(tr, r, t, tri);
        out_t[i] = t;
        out_tri[i] = tri;
    }
}

struct LvisArgs {
    Tree tr;
    const float* xyz;      // [n,3]
    const float* normal;   // [n,3]
    const float* alpha;    // [n]
    long long n;
    const float* lxyz;     // [L,3]
    int n_lights;
    float eps;
    float* lvis;           // [n,L]
};

__global__ __launch_bounds__(256) void mesh_lvis_kernel(LvisArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * 4;
    const long long row_tiles = (a.n + 63) / 64;
    const int light_tiles = (a.n_lights + 63) / 64;
    for (long long task = wave; task < row_tiles * light_tiles; task += nwaves) {
        const long long row0 = task / light_tiles * 64;
        const int l0 = (int)(task % light_tiles) * 64;
        const long long row = row0 + lane;
        const bool in = row < a.n;
        const long long rc = in ? row : 0;
        const float al = in ? a.alpha[rc] : 0.0f;
        const float px = a.xyz[rc * 3], py = a.xyz[rc * 3 + 1], pz = a.xyz[rc * 3 + 2];
        const float nx = a.normal[rc * 3], ny = a.normal[rc * 3 + 1], nz = a.normal[rc * 3 + 2];
        unsigned long long vis = 0ull;
        const int nl = a.n_lights - l0 < 64 ? a.n_lights - l0 : 64;
        for (int li = 0; li < nl; ++li) {
            const float qx = a.lxyz[(l0 + li) * 3], qy = a.lxyz[(l0 + li) * 3 + 1], qz = a.lxyz[(l0 + li) * 3 + 2];
            const float ex = qx - px, ey = qy - py, ez = qz - pz;
            const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float dx = ex / len, dy = ey / len, dz = ez / len;
            const float cosv = (nx * dx + ny * dy) + nz * dz;
            if (al != 0.0f && cosv > 0.0f) {
                const Ray r(px + a.eps * dx, py + a.eps * dy, pz + a.eps * dz, dx, dy, dz);
                float t;
                int tri;
                if (!walk<true>(a.tr, r, t, tri)) vis |= 1ull << li;
            }
        }
        // row by row: the 64 lanes store the 64 lights of one row
        const int rows = a.n - row0 < 64 ? (int)(a.n - row0) : 64;
        const unsigned vlo = (unsigned)vis, vhi = (unsigned)(vis >> 32);
        for (int rr = 0; rr < rows; ++rr) {
            const unsigned mlo = __shfl(vlo, rr, 64), mhi = __shfl(vhi, rr, 64);
            const float ar = __shfl(al, rr, 64);
            const unsigned long long m = ((unsigned long long)mhi << 32) | mlo;
            if (lane < nl) a.lvis[(row0 + rr) * a.n_lights + l0 + lane] = ((m >> lane) & 1ull) ? ar : 0.0f;
        }
    }
}

__host__ Tree tree_of(const void* blob, int n_nodes, int n_tris) {
    const char* p = (const char*)blob + sizeof(Header);
    return Tree{(const float4*)p, (const float4*)(p + (size_t)(n_nodes + 1) * sizeof(Node)), n_nodes, n_tris};
}

}  // namespace mesh
}  // namespace nfx

extern "C" int nfx_launch_mesh_cast(const void* blob, int n_nodes, int n_tris, const float* rayo, const float* rayd, long long n, float* t,
                                    int* tri, hipStream_t st) {
    using namespace nfx;
    if (n <= 0) return 0;
    const long long want = (n + 255) / 256;
    const int grid = (int)(want < 65536 ? want : 65536);
    hipLaunchKernelGGL(mesh::mesh_cast_kernel, dim3(grid), dim3(256), 0, st, mesh::tree_of(blob, n_nodes, n_tris), rayo, rayd, n, t, tri);
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_mesh_lvis(const void* blob, int n_nodes, int n_tris, const float* xyz, const float* normal, const float* alpha,
                                    long long n, const float* lxyz, int n_lights, float eps, float* lvis, hipStream_t st) {
    using namespace nfx;
    if (n <= 0 || n_lights <= 0) return 0;
    mesh::LvisArgs a{mesh::tree_of(blob, n_nodes, n_tris), xyz, normal, alpha, n, lxyz, n_lights, eps, lvis};
    const long long want = ((n + 63) / 64 * ((n_lights + 63) / 64) + 3) / 4;
    const int grid = (int)(want < 65536 ? want : 65536);
    hipLaunchKernelGGL(mesh::mesh_lvis_kernel, dim3(grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
