// brdf_row.hpp — one (point, light) row of the learned BRDF (nerfactor.py:413-458): from the point, the light, the
// camera and the normal to the 16 B-operand values of lane half h in the slot order of brdf_input_slots()
// (mlp128_layout.hpp):
//   k-step 0: h=0: sin(r0) sin(r1) sin(r2) sin(2r0) sin(2r1) sin(2r2) r0 r1      r = (phi_d, theta_h, theta_d)
//             h=1: cos(r0) ...                         cos(2r2)       r2 z0
//   k-step 1: z_i (i >= 1) at h = (i-1)&1, j = (i-1)>>1; zero elsewhere
// Two geometries in front of the slots: the reference's op sequence (brdf_row_rusink) and the closed form
// (brdf_point_frame + brdf_row_angles).  Every kernel that evaluates the prior on rows fills its operand here.
#pragma once
#include "geom.hpp"

namespace nfx {

// ---- reference order: front-lit decision (nerfactor.py:429-432) and rus = (phi_d, theta_h, theta_d)
__device__ __forceinline__ bool brdf_row_rusink(const float (&x)[3], const float (&lp)[3], const float (&cm)[3],
                                                const float (&nr)[3], float (&rus)[3]) {
    float ldir[3], vdir[3], rot[9], ll[3], vl[3];
    dir_to(lp, x, ldir);          // shape.py:128-131
    dir_to(cm, x, vdir);          // shape.py:137-140
    world2local(nr, rot);         // util/geom.py:119-149
    mat3_apply(rot, ldir, ll);    // nerfactor.py:418-419
    mat3_apply(rot, vdir, vl);
    dir2rusink(ll, vl, rus);      // util/geom.py:152-192 with a = light, b = view
    return ll[2] > 0.0f;
}

// ---- the slots.  k-step 1 (the latent code's z_1 ..) on its own: the closed-form callers fill k-step 0 themselves
__device__ __forceinline__ void brdf_fill_z(const float* zp, int z_dim, int h, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = 1 + 2 * j + h;  // z index held by (half h, element j) of k-step 1
        v[8 + j] = i < z_dim ? zp[i] : 0.0f;
    }
}
// SMALL: v_sin / v_cos on the angles <= pi of two bands (sin_shifted_small); else the full-range sin_shifted
template <bool SMALL = true>
__device__ __forceinline__ void brdf_fill_slots(const float (&rus)[3], const float* zp, int z_dim, int h, float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const float arg = rus[q % 3] * (float)(1 << (q / 3));
        v[q] = SMALL ? sin_shifted_small(arg, h) : sin_shifted(arg, h);
    }
    v[6] = h ? rus[2] : rus[0];
    v[7] = h ? zp[0] : rus[1];
    brdf_fill_z(zp, z_dim, h, v);
}
// 16 floats -> the two bf16 k-steps of column tile c
template <int CT>
__device__ __forceinline__ void brdf_cast_slots(const float (&v)[16], bf16x8 (&pl)[2][CT], int c) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) pl[s][c][j] = (__bf16)v[8 * s + j];
    }
}

// ---- closed form: Rusinkiewicz angles without the two Rodrigues rotations' sin / cos and without the half-vector
// azimuth (cos phi_h = h_x / s, sin phi_h = h_y / s, sin theta_h = s = |h_xy|), polynomial acos / atan2, v_rsq_f32
// (1 ulp) instead of the IEEE sqrt + divide sequences, and the two-band encoding of the three angles from double-angle
// identities instead of 6 v_sin / v_cos
__device__ __forceinline__ float acos_poly(float x) {   // Abramowitz-Stegun 4.4.46, |err| <= 2e-8 + fp32 rounding
    const float ax = fabsf(x);
    float p = -0.0012624911f;
    p = fmaf(p, ax, 0.0066700901f);
    p = fmaf(p, ax, -0.0170881256f);
    p = fmaf(p, ax, 0.0308918810f);
    p = fmaf(p, ax, -0.0501743046f);
    p = fmaf(p, ax, 0.0889789874f);
    p = fmaf(p, ax, -0.2145988016f);
    p = fmaf(p, ax, 1.5707963050f);
    const float r = sqrtf(1.0f - ax) * p;
    return x < 0.0f ? 3.14159265358979323846f - r : r;
}
__device__ __forceinline__ float atan2_poly(float y, float x) {   // Cephes atanf polynomial, |err| <= 3e-7
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float t = mx > 0.0f ? mn * __builtin_amdgcn_rcpf(mx) : 0.0f;
    const bool big = t > 0.4142135623730950f;
    const float t2 = big ? (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f) : t;
    const float zz = t2 * t2;
    float q = fmaf(8.05374449538e-2f, zz, -1.38776856032e-1f);
    q = fmaf(q, zz, 1.99777106478e-1f);
    q = fmaf(q, zz, -3.33329491539e-1f);
    float r = fmaf(q * zz, t2, t2) + (big ? 0.78539816339744830962f : 0.0f);
    r = ay > ax ? 1.57079632679489661923f - r : r;
    r = x < 0.0f ? 3.14159265358979323846f - r : r;
    return y < 0.0f ? -r : r;
}
__device__ __forceinline__ void nrm_rsq(float (&v)[3]) {
    const float inv = __builtin_amdgcn_rsqf(fmaxf(dot3(v, v), 1e-6f));
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}
// The per-POINT half of the row geometry: local frame [t; b; n] of the normal and the view direction in it (a queue
// fill computes it once per point); brdf_row_angles is what is left per (point, light) row.
__device__ __forceinline__ void brdf_point_frame(const float (&x)[3], const float (&cm)[3], const float (&nr)[3],
                                                 float (&rot)[9], float (&vl)[3]) {
    float vdir[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vdir[k] = cm[k] - x[k];
    nrm_rsq(vdir);
    float n[3] = {nr[0], nr[1], nr[2]}, t[3], b[3];
    nrm_rsq(n);
    const float zax[3] = {0.0f + 1e-6f, 0.0f + 1e-6f, 1.0f + 1e-6f};   // geom.py:128
    cross3(n, zax, t);
    nrm_rsq(t);
    cross3(n, t, b);
    nrm_rsq(b);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rot[k] = t[k];
        rot[3 + k] = b[k];
        rot[6 + k] = n[k];
    }
    mat3_apply(rot, vdir, vl);
    nrm_rsq(vl);                  // dir2rusink re-normalises its inputs (geom.py:158-159)
}
// The row with the values of BOTH lane halves: S[q] is what the half-0 lane puts into slot q of k-step 0 (sines, phi_d,
// theta_h), C[q] what the half-1 lane does (cosines, theta_d; slot 7 of half 1 is z_0, filled by the caller).
__device__ __forceinline__ void brdf_row_angles(const float (&x)[3], const float (&lp)[3], const float (&rot)[9],
                                                const float (&vl)[3], float (&S)[8], float (&C)[8]) {
    auto nrm = [](float (&v)[3]) { nrm_rsq(v); };
    float ldir[3], ll[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ldir[k] = lp[k] - x[k];
    nrm(ldir);
    mat3_apply(rot, ldir, ll);
    nrm(ll);
    float hv[3] = {(ll[0] + vl[0]) * 0.5f, (ll[1] + vl[1]) * 0.5f, (ll[2] + vl[2]) * 0.5f};
    nrm(hv);
    const float cth = fminf(fmaxf(hv[2], -1.0f), 1.0f);
    const float sxy = sqrtf(hv[0] * hv[0] + hv[1] * hv[1]);           // sin(theta_h) >= 0
    const float inv = sxy > 0.0f ? __builtin_amdgcn_rcpf(sxy) : 0.0f;
    const float cph = sxy > 0.0f ? hv[0] * inv : 1.0f, sph = hv[1] * inv;   // atan2(0, 0) = 0
    // diff = R_y(-theta_h) R_z(-phi_h) b with b = view (geom.py:183)
    const float t0 = vl[0] * cph + vl[1] * sph, t1 = vl[1] * cph - vl[0] * sph;
    const float d0 = t0 * cth - vl[2] * sxy, d1 = t1, d2 = vl[2] * cth + t0 * sxy;
    const float ctd = fminf(fmaxf(d2, -1.0f), 1.0f);
    const float rxy = sqrtf(d0 * d0 + d1 * d1);                       // sin(theta_d) >= 0
    const float theta_h = acos_poly(cth), theta_d = acos_poly(ctd);
    const float pi = 3.14159265358979323846f;
    float phi_d = atan2_poly(d1, d0);
    phi_d = phi_d - floorf(phi_d / pi) * pi;                          // tf.math.floormod(x, pi)
    const float rinv = rxy > 0.0f ? __builtin_amdgcn_rcpf(rxy) : 0.0f;
    const bool flip = d1 < 0.0f || (d1 == 0.0f && d0 < 0.0f);        // + pi: both signs change
    const float cpd0 = rxy > 0.0f ? d0 * rinv : 1.0f, spd0 = d1 * rinv;
    const float cpd = flip ? -cpd0 : cpd0, spd = flip ? -spd0 : spd0;
    // band 0: (phi_d, theta_h, theta_d), band 1: the doubled angles
    S[0] = spd; S[1] = sxy; S[2] = rxy;
    S[3] = 2.0f * spd * cpd; S[4] = 2.0f * sxy * cth; S[5] = 2.0f * rxy * ctd;
    S[6] = phi_d; S[7] = theta_h;
    C[0] = cpd; C[1] = cth; C[2] = ctd;
    C[3] = cpd * cpd - spd * spd; C[4] = cth * cth - sxy * sxy; C[5] = ctd * ctd - rxy * rxy;
    C[6] = theta_d; C[7] = 0.0f;
}

// The 16 values of one row, lane half h.  GEO = 0: the reference's op sequence.  GEO = 1: the closed form.
template <int GEO>
__device__ __forceinline__ void brdf_row_inputs(const float (&x)[3], const float (&lp)[3], const float (&cm)[3],
                                                const float (&nr)[3], const float* zp, int z_dim, int h,
                                                float (&v)[16]) {
    if constexpr (GEO == 0) {
        float rus[3];
        brdf_row_rusink(x, lp, cm, nr, rus);
        brdf_fill_slots(rus, zp, z_dim, h, v);
    } else {
        float rot[9], vl[3], S[8], C[8];
        brdf_point_frame(x, cm, nr, rot, vl);
        brdf_row_angles(x, lp, rot, vl, S, C);
#pragma unroll
        for (int q = 0; q < 7; ++q) v[q] = h ? C[q] : S[q];
        v[7] = h ? zp[0] : S[7];
        brdf_fill_z(zp, z_dim, h, v);
    }
}

}  // namespace nfx
