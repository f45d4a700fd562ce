// capi_geom.cpp — C-ABI entry points of the geometry-extraction kernels (include/nfx.h): density only, and density
// with its spatial gradient (geometry_from_nerf.py:249-350).  Their blob (nfx_nerf_pack_geom_weights) is laid out in
// pack_nets.cpp.
#include <hip/hip_runtime.h>
#include <math.h>

#include "capi_common.hpp"
#include "nerf_points.hpp"

extern "C" {
// The three point descriptions of nerf_points.hpp.  A listed launch has n_pts = the list's capacity, every sample.
static nfx::geo::Points every_sample(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples) {
    return {rayo, rayd, z, (long long)n_rays * n_samples, n_samples, nullptr, nullptr, 1, 0};
}
static nfx::geo::Points listed(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                               const int* list, const int* count, int list_stride) {
    return {rayo, rayd, z, (long long)n_rays * n_samples, n_samples, list, count, list_stride, 0};
}
static nfx::geo::Points last_samples(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples) {
    return {rayo, rayd, z, (long long)n_rays, n_samples, nullptr, nullptr, 4, 1};
}

// bf16 density of every sample: the render kernel's dataflow over the GEOM blob (nerf_sigma_v6.hip, round 6; default) or the
// round-2 kernel (option sigma_variant = 0) — the same MFMAs on the same operands, bit-identical
static int launch_sigma_bf16(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples,
                             const void* blob, float* sigma, hipStream_t st) {
    const int blocks = nfx_option_int("nerf_blocks", 256);
    if (nfx_option_int("sigma_variant", 1) != 0)
        return nfx_launch_nerf_sigma_v6(rayo, rayd, z, n_pts, n_samples, blob, sigma, blocks, st);
    return nfx_launch_nerf_sigma_geo(rayo, rayd, z, n_pts, n_samples, blob, sigma, blocks, st);
}

int nfx_nerf_sigma_fwd(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                       const void* blob, int prec, float* sigma, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_fwd: bad shape");
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_sigma_fwd: bad prec %d", prec);
    if (n_rays == 0) return NFX_OK;
    REQUIRE(rayo && rayd && z && blob && sigma, "nfx_nerf_sigma_fwd: null pointer");
    if (!ALIGNED(blob, 16)) return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_fwd: blob must be 16-byte aligned");
    if (prec == NFX_PREC_FP32) {
        const nfx::geo::Points pts = every_sample(rayo, rayd, z, n_rays, n_samples);
        return nfx_hip_result(nfx_launch_nerf_sigma_x3(&pts, blob, sigma, nfx_option_int("nerf_blocks", 256), (hipStream_t)stream),
                              "nerf_sigma_fwd(fp32)");
    }
    return nfx_hip_result(launch_sigma_bf16(rayo, rayd, z, (long long)n_rays * n_samples, n_samples, blob, sigma,
                                            (hipStream_t)stream),
                          "nerf_sigma_fwd");
}

int nfx_nerf_refine_select(const float* rgbs, const float* z, const float* rayd, int64_t n_rays, int n_samples,
                           float t_min, float a_lo, float a_hi, float sigma_margin, int dilate, int* list, int* count,
                           void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1 && n_samples <= 512, "nfx_nerf_refine_select: bad shape (1 <= S <= 512, got %d)", n_samples);
    REQUIRE(n_rays * (int64_t)n_samples < (int64_t)1 << 31, "nfx_nerf_refine_select: %lld samples do not fit int32 indices",
            (long long)(n_rays * n_samples));
    REQUIRE(dilate >= 0 && dilate <= 8, "nfx_nerf_refine_select: dilate = %d (0 .. 8)", dilate);
    REQUIRE(count, "nfx_nerf_refine_select: null count");
    if (n_rays > 0) REQUIRE(rgbs && z && rayd && list, "nfx_nerf_refine_select: null pointer");
    if (n_rays > 0 && !ALIGNED(rgbs, 16)) return nfx_fail(NFX_EALIGN, "nfx_nerf_refine_select: rgbs must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_refine_select(rgbs, z, rayd, (long long)n_rays, n_samples, t_min, a_lo, a_hi, sigma_margin, dilate,
                                                   list, count, (hipStream_t)stream), "nerf_refine_select");
}

int nfx_nerf_sigma_refine(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                          const void* blob, const int* list, const int* count, float* rgbs, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_refine: bad shape");
    if (n_rays == 0) return NFX_OK;
    REQUIRE(rayo && rayd && z && blob && list && count && rgbs, "nfx_nerf_sigma_refine: null pointer");
    if (!ALIGNED(blob, 16)) return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_refine: blob must be 16-byte aligned");
    const nfx::geo::Points pts = listed(rayo, rayd, z, n_rays, n_samples, list, count, 4);
    return nfx_hip_result(nfx_launch_nerf_sigma_x3(&pts, blob, rgbs, nfx_option_int("nerf_blocks", 256), (hipStream_t)stream),
                          "nerf_sigma_refine");
}

int nfx_nerf_sigma_refine_last(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                               const void* blob, float* rgbs, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_refine_last: bad shape");
    if (n_rays == 0) return NFX_OK;
    REQUIRE(rayo && rayd && z && blob && rgbs, "nfx_nerf_sigma_refine_last: null pointer");
    if (!ALIGNED(blob, 16)) return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_refine_last: blob must be 16-byte aligned");
    const nfx::geo::Points pts = last_samples(rayo, rayd, z, n_rays, n_samples);
    return nfx_hip_result(nfx_launch_nerf_sigma_x3(&pts, blob, rgbs, nfx_option_int("nerf_blocks", 256), (hipStream_t)stream),
                          "nerf_sigma_refine_last");
}

int nfx_nerf_sigma_grad(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                        const void* geom_blob, int prec, float* normal_sigma, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_grad: bad shape");
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_sigma_grad: bad prec %d", prec);
    if (n_rays == 0) return NFX_OK;
    REQUIRE(rayo && rayd && z && geom_blob && normal_sigma, "nfx_nerf_sigma_grad: null pointer");
    if (!ALIGNED(geom_blob, 16) || !ALIGNED(normal_sigma, 16))
        return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_grad: blob and output must be 16-byte aligned");
    const nfx::geo::Points pts = every_sample(rayo, rayd, z, n_rays, n_samples);
    const int blocks = nfx_option_int("nerf_blocks", 256);
    return nfx_hip_result((prec == NFX_PREC_FP32 ? nfx_launch_nerf_sigma_grad_x3 : nfx_launch_nerf_sigma_grad)(
                              &pts, geom_blob, normal_sigma, blocks, (hipStream_t)stream),
                          prec == NFX_PREC_FP32 ? "nerf_sigma_grad(fp32)" : "nerf_sigma_grad");
}

// the density of every sample [n_pts floats, padded to 16 bytes], then the row list (rowsel.hpp)
static size_t sigma_grad_sigma_bytes(long long n_pts) { return ((size_t)n_pts * 4 + 15) / 16 * 16; }
size_t nfx_nerf_sigma_grad_workspace_bytes(int64_t n_rays, int n_samples) {
    if (n_rays <= 0 || n_samples <= 0) return 0;
    const long long n_pts = (long long)n_rays * n_samples;
    return sigma_grad_sigma_bytes(n_pts) + nfx_nerf_bwd_list_bytes(n_pts);
}

int nfx_nerf_sigma_grad_rows(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                             const void* geom_blob, int prec, float* normal_sigma, void* workspace,
                             size_t workspace_bytes, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_grad_rows: bad shape");
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_sigma_grad_rows: bad prec %d", prec);
    if (n_rays == 0) return NFX_OK;
    REQUIRE(rayo && rayd && z && geom_blob && normal_sigma && workspace, "nfx_nerf_sigma_grad_rows: null pointer");
    const long long n_pts = (long long)n_rays * n_samples;
    REQUIRE(n_pts < (1ll << 31), "nfx_nerf_sigma_grad_rows: %lld samples do not fit int32 indices", n_pts);
    REQUIRE(workspace_bytes >= nfx_nerf_sigma_grad_workspace_bytes(n_rays, n_samples), "nfx_nerf_sigma_grad_rows: workspace too small");
    if (!ALIGNED(geom_blob, 16) || !ALIGNED(normal_sigma, 16) || !ALIGNED(workspace, 16))
        return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_grad_rows: blob, output and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = nfx_option_int("nerf_blocks", 256);
    float* sigma = static_cast<float*>(workspace);
    void* list_ws = static_cast<char*>(workspace) + sigma_grad_sigma_bytes(n_pts);
    const int* count = static_cast<const int*>(list_ws);
    const int* list = reinterpret_cast<const int*>(static_cast<char*>(list_ws) + nfx_nerf_bwd_list_bytes(n_pts)) - (n_pts + 3) / 4 * 4;
    // 1. the density of every sample (the forward-only kernel: bit-identical to the gradient kernel's own density)
    const nfx::geo::Points all = every_sample(rayo, rayd, z, n_rays, n_samples);
    int rc = nfx_hip_result(prec == NFX_PREC_FP32 ? nfx_launch_nerf_sigma_x3(&all, geom_blob, sigma, blocks, st)
                                                  : launch_sigma_bf16(rayo, rayd, z, n_pts, n_samples, geom_blob, sigma, st),
                            "nerf_sigma_grad_rows(density)");
    if (rc) return rc;
    // 2. the samples with a density, ascending; every other sample's output row is final after this pass
    rc = nfx_hip_result(nfx_launch_select_density(sigma, n_pts, normal_sigma, list_ws, st), "nerf_sigma_grad_rows(select)");
    if (rc) return rc;
    // 3. forward + reverse sweep over the listed samples only
    const nfx::geo::Points pts = listed(rayo, rayd, z, n_rays, n_samples, list, count, 4);
    return nfx_hip_result((prec == NFX_PREC_FP32 ? nfx_launch_nerf_sigma_grad_x3 : nfx_launch_nerf_sigma_grad)(
                              &pts, geom_blob, normal_sigma, blocks, st),
                          "nerf_sigma_grad_rows(gradient)");
}

// ---------------------------------------------------------------- occupancy grid (occgrid.hip)
int nfx_nerf_sigma_fwd_list(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                            const void* blob, int prec, const int* list, const int* count, float* sigma, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_nerf_sigma_fwd_list: bad shape");
    REQUIRE(prec == NFX_PREC_BF16 || prec == NFX_PREC_FP32, "nfx_nerf_sigma_fwd_list: bad prec %d", prec);
    if (n_rays == 0) return NFX_OK;
    const long long n_pts = (long long)n_rays * n_samples;
    REQUIRE(n_pts < (1ll << 31), "nfx_nerf_sigma_fwd_list: %lld samples do not fit int32 indices", n_pts);
    REQUIRE(rayo && rayd && z && blob && list && count && sigma, "nfx_nerf_sigma_fwd_list: null pointer");
    if (!ALIGNED(blob, 16)) return nfx_fail(NFX_EALIGN, "nfx_nerf_sigma_fwd_list: blob must be 16-byte aligned");
    const int blocks = nfx_option_int("nerf_blocks", 256);
    hipStream_t st = (hipStream_t)stream;
    if (prec == NFX_PREC_FP32) {
        const nfx::geo::Points pts = listed(rayo, rayd, z, n_rays, n_samples, list, count, 1);
        return nfx_hip_result(nfx_launch_nerf_sigma_x3(&pts, blob, sigma, blocks, st), "nerf_sigma_fwd_list");
    }
    return nfx_hip_result(nfx_launch_nerf_sigma_v6_list(rayo, rayd, z, n_pts, n_samples, blob, sigma, list, count, blocks, st),
                          "nerf_sigma_fwd_list");
}

size_t nfx_occgrid_workspace_bytes(int64_t n_rays, int n_samples) {
    if (n_rays <= 0 || n_samples <= 0) return 0;
    return nfx_occgrid_list_bytes((long long)n_rays * n_samples);
}

static bool valid_box(const float* b) {
    for (int k = 0; k < 3; ++k)
        if (!(b[2 * k] < b[2 * k + 1]) || !isfinite(b[2 * k]) || !isfinite(b[2 * k + 1])) return false;
    return true;
}

int nfx_occgrid_select(const float* rayo, const float* rayd, const float* z, int64_t n_rays, int n_samples,
                       const uint32_t* bits, int res, const float* box, const float* bbox, float* sigma, void* workspace,
                       size_t workspace_bytes, void* stream) {
    REQUIRE(n_rays >= 0 && n_samples >= 1, "nfx_occgrid_select: bad shape");
    REQUIRE(res >= 1 && res <= NFX_OCCGRID_MAX_RES, "nfx_occgrid_select: res = %d (1 .. %d)", res, NFX_OCCGRID_MAX_RES);
    REQUIRE(box && valid_box(box), "nfx_occgrid_select: box must be finite with min < max on every axis");
    if (n_rays == 0) return NFX_OK;
    const long long n_pts = (long long)n_rays * n_samples;
    REQUIRE(n_pts < (1ll << 31), "nfx_occgrid_select: %lld samples do not fit int32 indices", n_pts);
    REQUIRE(rayo && rayd && z && bits && sigma && workspace, "nfx_occgrid_select: null pointer");
    REQUIRE(workspace_bytes >= nfx_occgrid_workspace_bytes(n_rays, n_samples), "nfx_occgrid_select: workspace too small");
    if (!ALIGNED(workspace, 16)) return nfx_fail(NFX_EALIGN, "nfx_occgrid_select: workspace must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_occgrid_select(rayo, rayd, z, n_pts / n_samples, n_samples, bits, res, box, bbox, sigma,
                                                    workspace, (hipStream_t)stream),
                          "occgrid_select");
}

int nfx_occgrid_bake(const float* probe_sigma, int res, int probes, float margin, int dilate, uint32_t* bits,
                     uint32_t* workspace, void* stream) {
    REQUIRE(res >= 1 && res <= NFX_OCCGRID_MAX_RES, "nfx_occgrid_bake: res = %d (1 .. %d)", res, NFX_OCCGRID_MAX_RES);
    REQUIRE(probes >= 1 && probes <= 16, "nfx_occgrid_bake: probes = %d (1 .. 16 per axis)", probes);
    const long long m = (long long)res * probes;
    REQUIRE(m * m * m <= NFX_OCCGRID_MAX_PROBES, "nfx_occgrid_bake: (res probes)^3 = %lld probes (at most %lld)", m * m * m,
            (long long)NFX_OCCGRID_MAX_PROBES);
    REQUIRE(dilate >= 0 && dilate <= 16, "nfx_occgrid_bake: dilate = %d (0 .. 16)", dilate);
    REQUIRE(isfinite(margin), "nfx_occgrid_bake: margin must be finite");
    REQUIRE(probe_sigma && bits && workspace, "nfx_occgrid_bake: null pointer");
    return nfx_hip_result(nfx_launch_occgrid_bake(probe_sigma, res, probes, margin, dilate, bits, workspace,
                                                  (hipStream_t)stream),
                          "occgrid_bake");
}
}  // extern "C"
