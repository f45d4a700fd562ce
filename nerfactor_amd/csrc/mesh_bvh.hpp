// mesh_bvh.hpp — the blob of a triangle mesh's bounding-volume hierarchy: its layout (read by mesh_cast.hip, written by
// mesh_bvh.cpp) and the host-only builder.  No HIP in this header: mesh_bvh.cpp also builds as plain C++.
//
//   [Header 32 B] [Node 32 B] x (n_nodes + 1) [Tri 48 B] x n_tris          (every part 16-byte aligned in an aligned blob)
//
// Nodes are in depth-first order: the first child of an inner node is index + 1, its second child is the first child's
// skip link.  `skip` is the node to go to when the box is missed or the subtree is done (n_nodes = the end); it is always
// greater than the node's own index, so a walk that follows child / skip links only moves forward.  `first` is the first
// reordered triangle of the node's subtree — stored as is in a leaf and as -first - 1 in an inner node — and the subtree
// ends where the subtree of node[skip] begins; node[n_nodes] is a sentinel with first = n_tris for that reason.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nfx {
namespace mesh {

constexpr uint32_t kMagic = 0x4856424eu;   // "NBVH"
constexpr uint32_t kVersion = 1;

struct Header {
    uint32_t magic, version;
    int32_t n_nodes, n_tris, max_leaf;
    int32_t reserved[3];
};
struct Node {
    float lo[3];
    int32_t skip;
    float hi[3];
    int32_t first;
};
struct Tri {
    float v0[3];
    int32_t orig;      // index of the triangle in the caller's face array
    float v1[3];
    int32_t pad1;
    float v2[3];
    int32_t pad2;
};
static_assert(sizeof(Header) == 32 && sizeof(Node) == 32 && sizeof(Tri) == 48, "blob layout");

constexpr int32_t subtree_first(int32_t first) { return first < 0 ? -first - 1 : first; }

// number of nodes of the tree over n triangles (a function of n and max_leaf only: the split is by count)
int64_t node_count(int64_t n_tris, int64_t max_leaf);
// bytes of the blob; 0 for n_tris < 1, max_leaf < 1 or a mesh beyond the int32 limits of the layout
size_t blob_bytes(int64_t n_tris, int64_t max_leaf);
// Writes the blob.  Returns 0, or a non-zero code with a message in err (err_len bytes) for non-finite vertices, face
// indices outside [0, nv), sizes out of range or a buffer that is too small.  Deterministic: same input, same bytes.
int build(const float* vertices, int64_t nv, const int32_t* faces, int64_t nf, int max_leaf, void* blob, size_t bytes, char* err,
          size_t err_len);
// 0 when `h` is a header this builder writes and `bytes` the size of its blob; else non-zero with a message
int check_header(const Header* h, size_t bytes, char* err, size_t err_len);

}  // namespace mesh
}  // namespace nfx
