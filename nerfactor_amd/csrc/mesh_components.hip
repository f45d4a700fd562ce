// mesh_components.hip — connected components of an indexed triangle mesh (the rules are
// include/nfx.h's): label[v] = the smallest vertex index of v's component, a lock-free union-find in the label array itself.
//
//   init:    parent[v] = v; word 0 of the workspace (the count of skipped faces) = 0.
//   hook:    one thread per face; a face with an index outside [0, nv) adds one to word 0 and touches nothing else; the
//            others unite (a, b) and (b, c): find both roots with path halving, compare-and-swap the LARGER root under the
//            smaller, and start again from the two roots when the swap fails (somebody else hooked that root: progress).
//   flatten: parent[v] = root(v), halving on the way.
//
// Invariants: parent[x] <= x always, parent[x] < x once x is hooked, and a hooked vertex is never a root again — so every
// walk ends, whatever mix of old and new parents it reads, and the root of a tree is its smallest member.  When the hook
// launch has ended every face's vertices share a tree, so the trees are the components and the roots their minima, in any
// arrival order: the labels are a function of the face set.  Word 0 is an integer sum, which has no order either.
//
// Every parent word can be written by another workgroup, on another XCD with its own L2, during the same launch: all of its
// reads and writes are relaxed atomic operations at agent scope on the global address space — never a plain load, which
// may be served from a stale line.  Relaxed is enough, a parent publishes nothing but itself.  No wave waits for a store of
// another: the only loop that repeats on somebody else's action is the compare-and-swap retry.  No float, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"

namespace nfx {
namespace cc {

constexpr int kMaxBlocks = 256 * 8;   // 8 workgroups of 256 threads per CU; the rest is strided over

typedef __attribute__((address_space(1))) int gint;

__device__ __forceinline__ int load_parent(int* parent, int x) {
    return __hip_atomic_load((gint*)(parent + x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// an ancestor of x, never above the one already there
__device__ __forceinline__ void lower_parent(int* parent, int x, int ancestor) {
    __hip_atomic_fetch_min((gint*)(parent + x), ancestor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a vertex that was the root of x's tree at some moment of the call; halves the path it walks
__device__ __forceinline__ int find_root(int* parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        const int g = load_parent(parent, p);
        if (g == p) return p;
        lower_parent(parent, x, g);
        x = g;
    }
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
    while (a != b) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;      // the swap decides whether hi is still a root, not the load before it
        if (__hip_atomic_compare_exchange_strong((gint*)(parent + hi), &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = hi;
        b = lo;
    }
}

__global__ __launch_bounds__(256) void init_kernel(int* __restrict__ parent, unsigned nv, int* __restrict__ skipped) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *skipped = 0;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < (long long)nv; v += (long long)gridDim.x * 256) parent[v] = (int)v;
}

__global__ __launch_bounds__(256) void hook_kernel(const int* __restrict__ faces, unsigned nf, unsigned nv, int* parent, int* skipped) {
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < (long long)nf; f += (long long)gridDim.x * 256) {
        const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        if ((unsigned)a >= nv || (unsigned)b >= nv || (unsigned)c >= nv) {   // checked before any index addresses memory
            __hip_atomic_fetch_add((gint*)skipped, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        unite(parent, a, b);
        unite(parent, b, c);
    }
}

__global__ __launch_bounds__(256) void flatten_kernel(int* parent, unsigned nv) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < (long long)nv; v += (long long)gridDim.x * 256) {
        const int r = find_root(parent, (int)v);    // no hook runs now: the root of v's tree
        if (r != (int)v) lower_parent(parent, (int)v, r);
    }
}

inline unsigned grid_for(long long items) {
    const long long nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < kMaxBlocks ? nb : kMaxBlocks);
}

}  // namespace cc
}  // namespace nfx

extern "C" int nfx_launch_mesh_components(const int* faces, long long nf, long long nv, int* label, int* skipped, hipStream_t st) {
    using namespace nfx::cc;
    hipLaunchKernelGGL(init_kernel, dim3(grid_for(nv)), dim3(256), 0, st, label, (unsigned)nv, skipped);
    if (nf > 0) hipLaunchKernelGGL(hook_kernel, dim3(grid_for(nf)), dim3(256), 0, st, faces, (unsigned)nf, (unsigned)nv, label, skipped);
    if (nf > 0 && nv > 0) hipLaunchKernelGGL(flatten_kernel, dim3(grid_for(nv)), dim3(256), 0, st, label, (unsigned)nv);
    return (int)hipGetLastError();
}
