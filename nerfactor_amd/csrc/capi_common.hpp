// capi_common.hpp — what the C-ABI translation units (capi*.cpp) share: error reporting (defined in capi.cpp), the
// argument checks, and through launchers.hpp every launcher they dispatch to.
#pragma once
#include "launchers.hpp"

int nfx_fail(int code, const char* fmt, ...);   // records the message for nfx_last_error, returns code
int nfx_hip_result(int e, const char* what);    // NFX_OK, or NFX_EHIP with HIP's error string recorded

#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) return nfx_fail(NFX_EINVAL, __VA_ARGS__); \
    } while (0)
#define ALIGNED(p, a) ((((uintptr_t)(p)) & ((a)-1)) == 0)

// input features of a width-128 network: posenc10(xyz) | + posenc4(light direction) | z + posenc2(rusink); -1 = no such kind
inline int in_dims_of(int in_kind, int z_dim) {
    return in_kind == NFX_IN_XYZ ? 63 : in_kind == NFX_IN_XYZ_LDIR ? 90 : in_kind == NFX_IN_Z_RUSINK ? z_dim + 15 : -1;
}
// the kinds with a training blob and a backward of their own (the learned BRDF has its own entry points)
inline bool m128_has_backward(int in_kind) { return in_kind == NFX_IN_XYZ || in_kind == NFX_IN_XYZ_LDIR; }
