// mesh_bvh.cpp — host-only builder of the mesh BVH blob (layout and invariants: mesh_bvh.hpp).  Plain C++, no HIP.
//
// Split rule: object median.  Every range longer than max_leaf is cut at its middle element in the order of the centroids
// along the longest axis of the range's centroid box (std::nth_element; ties: the original index), so the shape of the
// tree — and the size of the blob — depends on (n_tris, max_leaf) only, and two builds of the same mesh give the same
// bytes.  (A median cut of one global Morton order was tried first: 133 nodes per camera ray on the 1.3 M-triangle bench
// mesh against 95 for this rule.)  Boxes are the exact fp32 min / max of their vertices moved one ulp outward; the
// ray-dependent padding is the slab test's (mesh_cast.hip).
#include "mesh_bvh.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace nfx {
namespace mesh {

int64_t node_count(int64_t n, int64_t max_leaf) {
    if (n <= max_leaf) return 1;
    const int64_t half = n / 2;
    // the two halves differ by at most one: at most two distinct sizes per level, no exponential recursion
    if (half == n - half) return 1 + 2 * node_count(half, max_leaf);
    return 1 + node_count(half, max_leaf) + node_count(n - half, max_leaf);
}

size_t blob_bytes(int64_t n_tris, int64_t max_leaf) {
    if (n_tris < 1 || max_leaf < 1 || n_tris > (int64_t)1 << 28) return 0;
    return sizeof(Header) + (size_t)(node_count(n_tris, max_leaf) + 1) * sizeof(Node) + (size_t)n_tris * sizeof(Tri);
}

namespace {

int fail(char* err, size_t err_len, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    if (err && err_len) snprintf(err, err_len, fmt, a, b, c);
    return 1;
}

struct Item {
    float c[3];     // centroid (it only orders: the geometry is never made from it)
    int32_t idx;    // index in the caller's face array
};

// reorders items[a, b) so that every range the tree will cut is cut at its object median
void order_range(Item* items, int32_t a, int32_t b, int32_t max_leaf) {
    if (b - a <= max_leaf) return;
    float lo[3] = {items[a].c[0], items[a].c[1], items[a].c[2]}, hi[3] = {lo[0], lo[1], lo[2]};
    for (int32_t i = a + 1; i < b; ++i)
        for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], items[i].c[k]), hi[k] = std::max(hi[k], items[i].c[k]);
    int axis = 0;
    if (hi[1] - lo[1] > hi[axis] - lo[axis]) axis = 1;
    if (hi[2] - lo[2] > hi[axis] - lo[axis]) axis = 2;
    const int32_t mid = a + (b - a) / 2;
    std::nth_element(items + a, items + mid, items + b, [axis](const Item& x, const Item& y) {
        return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.idx < y.idx);
    });
    order_range(items, a, mid, max_leaf);
    order_range(items, mid, b, max_leaf);
}

struct Builder {
    Node* nodes;
    const Tri* tris;
    int32_t max_leaf;
    int32_t n_nodes = 0;

    // emits the subtree over the reordered triangles [a, b); returns its node index
    int32_t emit(int32_t a, int32_t b) {
        const int32_t me = n_nodes++;
        Node& nd = nodes[me];
        if (b - a <= max_leaf) {
            const float inf = std::numeric_limits<float>::infinity();
            for (int k = 0; k < 3; ++k) nd.lo[k] = inf, nd.hi[k] = -inf;
            for (int32_t i = a; i < b; ++i) {
                const float* vs[3] = {tris[i].v0, tris[i].v1, tris[i].v2};
                for (const float* v : vs)
                    for (int k = 0; k < 3; ++k) nd.lo[k] = std::min(nd.lo[k], v[k]), nd.hi[k] = std::max(nd.hi[k], v[k]);
            }
            for (int k = 0; k < 3; ++k) nd.lo[k] = std::nextafterf(nd.lo[k], -inf), nd.hi[k] = std::nextafterf(nd.hi[k], inf);
            nd.first = a;
        } else {
            const int32_t mid = a + (b - a) / 2;
            const int32_t l = emit(a, mid), r = emit(mid, b);
            for (int k = 0; k < 3; ++k) {
                nodes[me].lo[k] = std::min(nodes[l].lo[k], nodes[r].lo[k]);
                nodes[me].hi[k] = std::max(nodes[l].hi[k], nodes[r].hi[k]);
            }
            nodes[me].first = -a - 1;
        }
        nodes[me].skip = n_nodes;
        return me;
    }
};

}  // namespace

int check_header(const Header* h, size_t bytes, char* err, size_t err_len) {
    if (!h) return fail(err, err_len, "mesh BVH: null header");
    if (h->magic != kMagic || h->version != kVersion)
        return fail(err, err_len, "mesh BVH: not a blob of nfx_mesh_bvh_build (magic %llx, version %lld)", h->magic, h->version);
    if (h->n_tris < 1 || h->max_leaf < 1 || blob_bytes(h->n_tris, h->max_leaf) == 0 || h->n_nodes != node_count(h->n_tris, h->max_leaf))
        return fail(err, err_len, "mesh BVH: inconsistent header (%lld nodes, %lld triangles, max_leaf %lld)", h->n_nodes, h->n_tris,
                    h->max_leaf);
    if (bytes != blob_bytes(h->n_tris, h->max_leaf))
        return fail(err, err_len, "mesh BVH: the blob is %lld bytes, its header describes %lld", (long long)bytes,
                    (long long)blob_bytes(h->n_tris, h->max_leaf));
    return 0;
}

int build(const float* vertices, int64_t nv, const int32_t* faces, int64_t nf, int max_leaf, void* blob, size_t bytes, char* err,
          size_t err_len) {
    if (!vertices || !faces || !blob) return fail(err, err_len, "mesh BVH: null pointer");
    if (nv < 1 || nv > std::numeric_limits<int32_t>::max()) return fail(err, err_len, "mesh BVH: %lld vertices", nv);
    const size_t need = blob_bytes(nf, max_leaf);
    if (need == 0) return fail(err, err_len, "mesh BVH: %lld triangles with max_leaf %lld cannot be built", nf, max_leaf);
    if (bytes < need) return fail(err, err_len, "mesh BVH: the buffer holds %lld bytes, %lld are needed", (long long)bytes, (long long)need);
    for (int64_t i = 0; i < nv * 3; ++i)
        if (!std::isfinite(vertices[i])) return fail(err, err_len, "mesh BVH: vertex %lld has a non-finite coordinate", i / 3);
    for (int64_t i = 0; i < nf * 3; ++i)
        if (faces[i] < 0 || faces[i] >= nv)
            return fail(err, err_len, "mesh BVH: face %lld names vertex %lld of %lld", i / 3, faces[i], nv);

    std::vector<Item> items((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) {
        for (int k = 0; k < 3; ++k)
            items[(size_t)f].c[k] = (float)(((double)vertices[(int64_t)faces[f * 3] * 3 + k] + (double)vertices[(int64_t)faces[f * 3 + 1] * 3 + k] +
                                             (double)vertices[(int64_t)faces[f * 3 + 2] * 3 + k]) / 3.0);
        items[(size_t)f].idx = (int32_t)f;
    }
    const int32_t leaf = (int32_t)std::min<int64_t>(max_leaf, nf);
    order_range(items.data(), 0, (int32_t)nf, leaf);

    std::memset(blob, 0, need);
    Header* h = (Header*)blob;
    Node* nodes = (Node*)((char*)blob + sizeof(Header));
    const int64_t n_nodes = node_count(nf, max_leaf);
    Tri* tris = (Tri*)((char*)nodes + (size_t)(n_nodes + 1) * sizeof(Node));
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t f = items[(size_t)i].idx;
        float* dst[3] = {tris[i].v0, tris[i].v1, tris[i].v2};
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) dst[c][k] = vertices[(int64_t)faces[f * 3 + c] * 3 + k];
        tris[i].orig = (int32_t)f;
    }
    Builder b{nodes, tris, leaf};
    b.emit(0, (int32_t)nf);
    if (b.n_nodes != n_nodes) return fail(err, err_len, "mesh BVH: built %lld nodes, counted %lld", b.n_nodes, n_nodes);
    Node& end = nodes[n_nodes];   // the sentinel: where the last subtree's triangles end
    end.skip = (int32_t)n_nodes;
    end.first = (int32_t)nf;
    h->magic = kMagic;
    h->version = kVersion;
    h->n_nodes = (int32_t)n_nodes;
    h->n_tris = (int32_t)nf;
    h->max_leaf = leaf;
    return 0;
}

}  // namespace mesh
}  // namespace nfx
