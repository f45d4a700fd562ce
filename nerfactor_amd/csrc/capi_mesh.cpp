// capi_mesh.cpp — C-ABI entry points of the mesh BVH builder (mesh_bvh.cpp, host only) and the ray casts (mesh_cast.hip).
#include <hip/hip_runtime.h>

#include "capi_common.hpp"
#include "mesh_bvh.hpp"

namespace {
// the counts of a header that matches the blob's size, or a recorded failure
int checked_counts(const char* who, const void* blob, size_t blob_bytes, const void* host_header, int* n_nodes, int* n_tris) {
    REQUIRE(blob && host_header, "%s: null blob or header", who);
    if (!ALIGNED(blob, 16)) return nfx_fail(NFX_EALIGN, "%s: the blob must be 16-byte aligned", who);
    char msg[200];
    const nfx::mesh::Header* h = (const nfx::mesh::Header*)host_header;
    if (nfx::mesh::check_header(h, blob_bytes, msg, sizeof msg)) return nfx_fail(NFX_EINVAL, "%s: %s", who, msg);
    *n_nodes = h->n_nodes;
    *n_tris = h->n_tris;
    return NFX_OK;
}
}  // namespace

extern "C" {
size_t nfx_mesh_bvh_bytes(int64_t nf, int max_leaf) { return nfx::mesh::blob_bytes(nf, max_leaf); }

int nfx_mesh_bvh_build(const float* vertices, int64_t nv, const int32_t* faces, int64_t nf, int max_leaf, void* blob, size_t blob_bytes) {
    char msg[200];
    if (nfx::mesh::build(vertices, nv, faces, nf, max_leaf, blob, blob_bytes, msg, sizeof msg))
        return nfx_fail(NFX_EINVAL, "nfx_mesh_bvh_build: %s", msg);
    return NFX_OK;
}

int nfx_mesh_cast(const void* blob, size_t blob_bytes, const void* host_header, const float* rayo, const float* rayd, int64_t n, float* t,
                  int* tri, void* stream) {
    REQUIRE(n >= 0, "nfx_mesh_cast: n (%lld) < 0", (long long)n);
    int n_nodes, n_tris;
    if (int rc = checked_counts("nfx_mesh_cast", blob, blob_bytes, host_header, &n_nodes, &n_tris)) return rc;
    if (n == 0) return NFX_OK;
    REQUIRE(rayo && rayd && t && tri, "nfx_mesh_cast: null pointer");
    return nfx_hip_result(nfx_launch_mesh_cast(blob, n_nodes, n_tris, rayo, rayd, n, t, tri, (hipStream_t)stream), "mesh_cast");
}

int nfx_mesh_lvis(const void* blob, size_t blob_bytes, const void* host_header, const float* xyz, const float* normal, const float* alpha,
                  int64_t n, const float* lxyz, int n_lights, float eps, float* lvis, void* stream) {
    REQUIRE(n >= 0, "nfx_mesh_lvis: n (%lld) < 0", (long long)n);
    REQUIRE(n_lights >= 1, "nfx_mesh_lvis: n_lights (%d) < 1", n_lights);
    int n_nodes, n_tris;
    if (int rc = checked_counts("nfx_mesh_lvis", blob, blob_bytes, host_header, &n_nodes, &n_tris)) return rc;
    if (n == 0) return NFX_OK;
    REQUIRE(xyz && normal && alpha && lxyz && lvis, "nfx_mesh_lvis: null pointer");
    return nfx_hip_result(nfx_launch_mesh_lvis(blob, n_nodes, n_tris, xyz, normal, alpha, n, lxyz, n_lights, eps, lvis, (hipStream_t)stream),
                          "mesh_lvis");
}
}
