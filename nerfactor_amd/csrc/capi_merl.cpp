// capi_merl.cpp — C-ABI entry points of the measured-BRDF lookup and sphere render (include/nfx.h, merl.hip).
#include <hip/hip_runtime.h>

#include "capi_common.hpp"

extern "C" {
int nfx_merl_query(const void* table4, const float* rusink, int64_t n, float* rgb, int* idx, void* stream) {
    REQUIRE(n >= 0, "nfx_merl_query: n (%lld) < 0", (long long)n);
    if (n == 0) return NFX_OK;
    REQUIRE(table4 && rusink && rgb, "nfx_merl_query: null pointer");
    if (!ALIGNED(table4, 16)) return nfx_fail(NFX_EALIGN, "nfx_merl_query: the table must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_merl_query(table4, rusink, n, rgb, idx, (hipStream_t)stream), "merl_query");
}

int nfx_merl_sphere_fwd(const float* xyz, const float* normal, int64_t n, const float* cam3, const void* table4,
                        const float* lxyz, const float* lweight, int n_lights, float* rgb, int* idx, void* stream) {
    REQUIRE(n >= 0, "nfx_merl_sphere_fwd: n (%lld) < 0", (long long)n);
    REQUIRE(n_lights > 0 && n_lights % 32 == 0 && n_lights <= 1024,
            "nfx_merl_sphere_fwd: n_lights (%d) must be a multiple of 32 in [32, 1024]", n_lights);
    if (n == 0) return NFX_OK;
    REQUIRE(xyz && normal && cam3 && table4 && lxyz && lweight && rgb, "nfx_merl_sphere_fwd: null pointer");
    if (!ALIGNED(table4, 16)) return nfx_fail(NFX_EALIGN, "nfx_merl_sphere_fwd: the table must be 16-byte aligned");
    return nfx_hip_result(nfx_launch_merl_sphere(xyz, normal, n, cam3, table4, lxyz, lweight, n_lights, rgb, idx, (hipStream_t)stream),
                          "merl_sphere_fwd");
}
}
