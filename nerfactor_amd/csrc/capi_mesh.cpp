// capi_mesh.cpp — C-ABI entry points of the mesh BVH builder (mesh_bvh.cpp, host only), the ray casts (mesh_cast.hip), the
// iso-surface extraction (isosurface.hip) and the component labelling (mesh_components.hip).
#include <hip/hip_runtime.h>
#include <math.h>

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

// the lattice's point count, or a recorded failure
int checked_lattice(const char* who, int nx, int ny, int nz, long long* n) {
    REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: a %d x %d x %d lattice (at least 2 points per axis)", who, nx, ny, nz);
    *n = (long long)nx * ny * nz;
    REQUIRE(*n < NFX_ISOSURFACE_MAX_POINTS, "%s: %d x %d x %d = %lld lattice points (fewer than 2^31)", who, nx, ny, nz, *n);
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

int nfx_isosurface_tables(int8_t* tri_table, int8_t* edge_table) {
    REQUIRE(tri_table && edge_table, "nfx_isosurface_tables: null pointer");
    nfx_isosurface_host_tables(tri_table, edge_table);
    return NFX_OK;
}

size_t nfx_isosurface_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2 || (long long)nx * ny * nz >= NFX_ISOSURFACE_MAX_POINTS) return 0;
    return nfx_isosurface_ws_bytes((long long)nx * ny * nz);
}

int nfx_isosurface_count(const float* field, int nx, int ny, int nz, float iso, void* workspace, size_t workspace_bytes, void* stream) {
    long long n;
    if (int rc = checked_lattice("nfx_isosurface_count", nx, ny, nz, &n)) return rc;
    REQUIRE(!isnan(iso), "nfx_isosurface_count: iso is NaN");
    REQUIRE(field && workspace, "nfx_isosurface_count: null pointer");
    REQUIRE(workspace_bytes >= nfx_isosurface_ws_bytes(n), "nfx_isosurface_count: workspace of %zu bytes, %zu needed", workspace_bytes,
            nfx_isosurface_ws_bytes(n));
    if (!ALIGNED(workspace, 16)) return nfx_fail(NFX_EALIGN, "nfx_isosurface_count: workspace must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_isosurface_count(field, nx, ny, nz, iso, workspace, (hipStream_t)stream), "isosurface_count");
}

int nfx_isosurface_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin, const float* spacing,
                        const void* workspace, size_t workspace_bytes, int64_t nv, int64_t nf, float* vertices, int32_t* faces, void* stream) {
    long long n;
    if (int rc = checked_lattice("nfx_isosurface_emit", nx, ny, nz, &n)) return rc;
    REQUIRE(!isnan(iso), "nfx_isosurface_emit: iso is NaN");
    REQUIRE(origin && spacing, "nfx_isosurface_emit: null origin or spacing");
    for (int k = 0; k < 3; ++k) {
        REQUIRE(isfinite(origin[k]), "nfx_isosurface_emit: origin[%d] = %g is not finite", k, origin[k]);
        REQUIRE(isfinite(spacing[k]) && spacing[k] > 0.f, "nfx_isosurface_emit: spacing[%d] = %g (finite, > 0)", k, spacing[k]);
    }
    REQUIRE(nv >= 0 && nv < (1ll << 31), "nfx_isosurface_emit: nv = %lld vertices (0 .. 2^31 - 1)", (long long)nv);
    REQUIRE(nf >= 0 && 3 * nf < (1ll << 31), "nfx_isosurface_emit: nf = %lld triangles, 3 nf = %lld (below 2^31)", (long long)nf,
            (long long)(3 * nf));
    REQUIRE(field && workspace, "nfx_isosurface_emit: null pointer");
    REQUIRE(workspace_bytes >= nfx_isosurface_ws_bytes(n), "nfx_isosurface_emit: workspace of %zu bytes, %zu needed", workspace_bytes,
            nfx_isosurface_ws_bytes(n));
    if (!ALIGNED(workspace, 16)) return nfx_fail(NFX_EALIGN, "nfx_isosurface_emit: workspace must be 16-byte aligned");
    if (nv == 0 && nf == 0) return NFX_OK;
    REQUIRE((nv == 0 || vertices) && (nf == 0 || faces), "nfx_isosurface_emit: null output");
    return nfx_hip_result(nfx_launch_isosurface_emit(field, nx, ny, nz, iso, origin, spacing, workspace, (int)nv, (int)nf, vertices, faces,
                                                     (hipStream_t)stream),
                          "isosurface_emit");
}

size_t nfx_mesh_components_workspace_bytes(int64_t nv, int64_t nf) {
    if (nv < 0 || nv >= (1ll << 31) || nf < 0 || 3 * nf >= (1ll << 31)) return 0;
    return 16;   // word 0: the faces skipped; padded to the alignment
}

int nfx_mesh_components(const int32_t* faces, int64_t nf, int64_t nv, int32_t* label, void* workspace, size_t workspace_bytes, void* stream) {
    REQUIRE(nv >= 0 && nv < (1ll << 31), "nfx_mesh_components: nv = %lld vertices (0 .. 2^31 - 1)", (long long)nv);
    REQUIRE(nf >= 0 && nf < (1ll << 31) && 3 * nf < (1ll << 31), "nfx_mesh_components: nf = %lld triangles, 3 nf = %lld (below 2^31)",
            (long long)nf, (long long)(3 * nf));
    REQUIRE(workspace, "nfx_mesh_components: null workspace");
    REQUIRE(workspace_bytes >= nfx_mesh_components_workspace_bytes(nv, nf), "nfx_mesh_components: workspace of %zu bytes, %zu needed",
            workspace_bytes, nfx_mesh_components_workspace_bytes(nv, nf));
    REQUIRE((nf == 0 || faces) && (nv == 0 || label), "nfx_mesh_components: null pointer");
    if (!ALIGNED(faces, 16) || !ALIGNED(label, 16) || !ALIGNED(workspace, 16))
        return nfx_fail(NFX_EALIGN, "nfx_mesh_components: faces, label and workspace must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_mesh_components(faces, nf, nv, label, (int*)workspace, (hipStream_t)stream), "mesh_components");
}
}
