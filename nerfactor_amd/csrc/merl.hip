// merl.hip — measured MERL BRDFs on the GPU (reference: brdf/merl/merl.py:MERL.query, a SciPy k-d tree over the valid
// entries of the 180 x 90 x 90 table, and data_gen/merl/make_dataset.py's render of it on a sphere).
//
// Table.  float4[180 * 90 * 90] in cube order (phi_d, theta_h, theta_d): rgb plus one pad float; an INVALID entry (below the
// horizon, or a hole of the measurement) holds -1 in all four lanes, a valid one is > 0 in x, y and z.
//
// Lookup.  The answer is the valid entry nearest to the query in Euclidean distance over raw (phi_d, theta_h, theta_d)
// radians.  The grid is a product grid (grid_phi / grid_th / grid_td below: brdf.merl.merl_to_rusink in fp32), so the
// per-axis nearest cell is the nearest entry overall: rint on the two linear axes, the inverted square on theta_h, each
// then settled against its neighbours by the true angular distance through the same fp32 grid function (ties: the smaller
// index).  When that cell is invalid the search stays EXACT: the lanes of the wave that need it are taken one by one
// (ballot), the 64 lanes scan the shell of radius r = 1, 2, ... of the box around the cell together (6 faces, 24 r^2 + 2
// cells, clipped to the cube), keep (squared distance, flat index) minima and reduce them with a fixed butterfly; the
// search stops when the nearest coordinate outside the box on any axis is farther than the best entry found, or when the
// box covers the cube — so it terminates for any table, and finds the entry of any table that has one.  The result of a
// query depends on the query and the table only, not on its lane or on the other queries of the launch.
//
// nfx_merl_sphere_fwd.  One wave per sphere sample walks the lights in tiles of 64, ascending; a tile without a lit
// front-facing light (ballot) is dropped; a row is  table[idx] * lweight[l] * (local l.z), a tile is summed by a fixed
// butterfly, a sample accumulates three fp32 sums and stores them once.  No atomics, no workspace, no LDS.  The angles are
// atan2 of a sine and a cosine: theta_h = atan2(|h_xy|, h_z) and theta_d = atan2(|l - v| / 2, |l + v| / 2) — near the
// highlight the theta_h cells are microns wide and acos of a cosine close to 1 keeps half the digits.
#include "geom.hpp"
#include "launchers.hpp"

namespace nfx {
namespace merl {

constexpr int kNP = 180, kNH = 90, kND = 90;
constexpr float kPi = 3.14159265358979323846f, kHalfPi = 1.57079632679489661923f;
constexpr float kInf = __builtin_inff();

__device__ __forceinline__ float grid_phi(int i) { return (float)i / (float)(kNP - 1) * kPi; }
__device__ __forceinline__ float grid_th(int j) {
    const float t = ((float)j + 0.105f) / (float)kNH;
    return t * t * kHalfPi;
}
__device__ __forceinline__ float grid_td(int k) { return (float)k / (float)(kND - 1) * kHalfPi; }
__device__ __forceinline__ int flat_of(int i, int j, int k) { return (i * kNH + j) * kND + k; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the index of [0, n) whose grid coordinate is nearest to q, from a first guess; ties go to the smaller index
template <class G>
__device__ __forceinline__ int settle(float q, int guess, int n, G grid) {
    int c = clampi(guess, 0, n - 1);
    const int lo = c > 0 ? c - 1 : c, hi = c < n - 1 ? c + 1 : c;
    const float dl = fabsf(q - grid(lo)), dc = fabsf(q - grid(c)), dh = fabsf(q - grid(hi));
    if (dh < dc && dh < dl) return hi;
    return dl <= dc ? lo : c;
}

__device__ __forceinline__ float dist2(const float (&q)[3], int i, int j, int k) {
    const float a = q[0] - grid_phi(i), b = q[1] - grid_th(j), c = q[2] - grid_td(k);
    return a * a + b * b + c * c;
}

// (d, idx) <- the smaller of the two pairs, by distance and then by index
__device__ __forceinline__ void take_min(float& d, int& idx, float od, int oidx) {
    if (od < d || (od == d && oidx < idx)) {
        d = od;
        idx = oidx;
    }
}

// The exact search around the invalid cell (ci, cj, ck) for the query q; every argument is wave-uniform and all 64
// lanes are active.  Returns the flat index of the nearest valid entry (ties: the smaller index), -1 for a table without one.
__device__ __forceinline__ int search_shells(const float4* __restrict__ tbl, float q0, float q1, float q2, int ci, int cj, int ck) {
    const int lane = threadIdx.x & 63;
    const float q[3] = {q0, q1, q2};
    float best = kInf;
    int bidx = 0x7fffffff;
    for (int r = 1; r < kNP; ++r) {
        for (int f = 0; f < 6; ++f) {
            const int ax = f >> 1, sgn = (f & 1) ? r : -r;
            // fixed coordinate of the face; its two free axes in ascending order, the earlier axes one cell short
            const int fix = (ax == 0 ? ci : ax == 1 ? cj : ck) + sgn;
            const int nfix = ax == 0 ? kNP : (ax == 1 ? kNH : kND);
            if (fix < 0 || fix >= nfix) continue;
            const float gfix = ax == 0 ? grid_phi(fix) : (ax == 1 ? grid_th(fix) : grid_td(fix));
            const float gap = (ax == 0 ? q0 : (ax == 1 ? q1 : q2)) - gfix;
            if (gap * gap > best) continue;                       // no entry of this face can beat or tie the best
            const int cu = ax == 0 ? cj : ci, nu = ax == 0 ? kNH : kNP, ru = ax == 0 ? r : r - 1;
            const int cv = ax == 2 ? cj : ck, nv = ax == 2 ? kNH : kND, rv = ax == 2 ? r - 1 : r;
            const int u0 = clampi(cu - ru, 0, nu - 1), u1 = clampi(cu + ru, 0, nu - 1);
            const int v0 = clampi(cv - rv, 0, nv - 1), v1 = clampi(cv + rv, 0, nv - 1);
            const int wv = v1 - v0 + 1, count = (u1 - u0 + 1) * wv;
            for (int e0 = 0; e0 < count; e0 += 256) {
                int fl[4];
                float x[4], d[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {                   // four gathers in flight
                    const int e = e0 + s * 64 + lane;
                    const bool in = e < count;
                    const int ec = in ? e : 0;
                    const int u = u0 + ec / wv, v = v0 + ec % wv;
                    const int i = ax == 0 ? fix : u, j = ax == 0 ? u : (ax == 1 ? fix : v), k = ax == 2 ? fix : v;
                    fl[s] = flat_of(i, j, k);
                    x[s] = in ? tbl[fl[s]].x : -1.0f;
                    d[s] = dist2(q, i, j, k);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (x[s] > 0.0f) take_min(best, bidx, d[s], fl[s]);
            }
            // the face's minimum to every lane, so that the next face's pruning is wave-uniform
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bidx, o, 64);
                take_min(best, bidx, od, oi);
            }
        }
        // the nearest coordinate outside the box, per axis and side; none when the box reaches the cube's end
        float out = kInf;
        if (ci - r - 1 >= 0) out = fminf(out, fabsf(q[0] - grid_phi(ci - r - 1)));
        if (ci + r + 1 < kNP) out = fminf(out, fabsf(q[0] - grid_phi(ci + r + 1)));
        if (cj - r - 1 >= 0) out = fminf(out, fabsf(q[1] - grid_th(cj - r - 1)));
        if (cj + r + 1 < kNH) out = fminf(out, fabsf(q[1] - grid_th(cj + r + 1)));
        if (ck - r - 1 >= 0) out = fminf(out, fabsf(q[2] - grid_td(ck - r - 1)));
        if (ck + r + 1 < kND) out = fminf(out, fabsf(q[2] - grid_td(ck + r + 1)));
        if (out == kInf) break;                                     // the box is the cube
        if (best < out * out * 0.99999f) break;                     // an entry outside is strictly farther
    }
    return best < kInf ? bidx : -1;
}

// idx of the query of every lane with `active` set (others: -1).  Convergent: call it with all 64 lanes of the wave.
// `t` receives the entry (NaN in all lanes where idx is -1).
__device__ __forceinline__ int lookup(const float4* __restrict__ tbl, const float (&q)[3], bool active, float4& t) {
    const bool finite = active && fabsf(q[0]) < kInf && fabsf(q[1]) < kInf && fabsf(q[2]) < kInf;   // false for NaN too
    const float qc[3] = {finite ? q[0] : 0.0f, finite ? q[1] : 0.0f, finite ? q[2] : 0.0f};
    const float ti = fminf(fmaxf(rintf(qc[0] / kPi * (float)(kNP - 1)), 0.0f), (float)(kNP - 1));
    const float tj = fminf(fmaxf(floorf(sqrtf(fmaxf(qc[1], 0.0f) / kHalfPi) * (float)kNH - 0.105f), 0.0f), (float)(kNH - 1));
    const float tk = fminf(fmaxf(rintf(qc[2] / kHalfPi * (float)(kND - 1)), 0.0f), (float)(kND - 1));
    const int ci = settle(qc[0], (int)ti, kNP, [](int i) { return grid_phi(i); });
    const int cj = settle(qc[1], (int)tj, kNH, [](int j) { return grid_th(j); });
    const int ck = settle(qc[2], (int)tk, kND, [](int k) { return grid_td(k); });
    const float nan = __builtin_nanf("");
    t = float4{nan, nan, nan, nan};
    int idx = -1;
    bool need = false;
    if (finite) {
        idx = flat_of(ci, cj, ck);
        t = tbl[idx];
        need = !(t.x > 0.0f);
    }
    unsigned long long todo = __ballot(need);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int found = search_shells(tbl, __shfl(qc[0], src, 64), __shfl(qc[1], src, 64), __shfl(qc[2], src, 64),
                                        __shfl(ci, src, 64), __shfl(cj, src, 64), __shfl(ck, src, 64));
        if (lane == src) {
            idx = found;
            t = found >= 0 ? tbl[found] : float4{nan, nan, nan, nan};
        }
    }
    return idx;
}

__global__ __launch_bounds__(256) void merl_query_kernel(const float4* __restrict__ tbl, const float* __restrict__ rusink, long long n,
                                                         float* __restrict__ rgb, int* __restrict__ out_idx) {
    const long long nthreads = (long long)gridDim.x * blockDim.x;
    // whole waves stay in the loop: the slow path of the lookup is wave-cooperative
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += nthreads) {
        const long long r = base + threadIdx.x;
        const bool active = r < n;
        const long long rc = active ? r : 0;
        const float q[3] = {rusink[rc * 3], rusink[rc * 3 + 1], rusink[rc * 3 + 2]};
        float4 t;
        const int idx = lookup(tbl, q, active, t);
        if (active) {
            rgb[r * 3] = t.x;
            rgb[r * 3 + 1] = t.y;
            rgb[r * 3 + 2] = t.z;
            if (out_idx) out_idx[r] = idx;
        }
    }
}

struct SphereArgs {
    const float* xyz;      // [n,3] sphere samples
    const float* normal;   // [n,3]
    long long n;
    float cam[3];
    const float4* tbl;
    const float* lxyz;     // [L,3]
    const float* lweight;  // [L,3] light * area
    int n_lights;
    float* rgb;            // [n,3]
    int* idx;              // [n,L] or null
};

__device__ __forceinline__ void unit3(float (&v)[3]) {
    const float len = sqrtf(dot3(v, v));
    const float inv = len > 0.0f ? 1.0f / len : 0.0f;
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}

// Rusinkiewicz angles of brdf.merl.dir2rusink for unit local directions (light ll, view vl)
__device__ __forceinline__ void rusink_of(const float (&ll)[3], const float (&vl)[3], float (&q)[3]) {
    float s[3] = {ll[0] + vl[0], ll[1] + vl[1], ll[2] + vl[2]}, m[3] = {ll[0] - vl[0], ll[1] - vl[1], ll[2] - vl[2]};
    const float ctd = 0.5f * sqrtf(dot3(s, s)), std_ = 0.5f * sqrtf(dot3(m, m));   // |l + v| = 2 cos theta_d, |l - v| = 2 sin theta_d
    float hv[3] = {s[0], s[1], s[2]};
    unit3(hv);
    const float sxy = sqrtf(hv[0] * hv[0] + hv[1] * hv[1]), cth = hv[2];
    const float inv = sxy > 0.0f ? 1.0f / sxy : 0.0f;
    const float cph = sxy > 0.0f ? hv[0] * inv : 1.0f, sph = hv[1] * inv;
    // the light turned by -phi_h about z and by -theta_h about y
    const float t0 = ll[0] * cph + ll[1] * sph, t1 = ll[1] * cph - ll[0] * sph;
    const float d0 = t0 * cth - ll[2] * sxy, d1 = t1;
    float phi_d = atan2f(d1, d0);
    if (phi_d < 0.0f) phi_d += kPi;          // np.mod(., pi)
    if (phi_d >= kPi) phi_d -= kPi;
    q[0] = phi_d;
    q[1] = atan2f(sxy, cth);
    q[2] = atan2f(std_, ctd);
}

__global__ __launch_bounds__(256) void merl_sphere_kernel(SphereArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long nw = (long long)gridDim.x * 4;
    for (long long is = (long long)blockIdx.x * 4 + wave; is < a.n; is += nw) {
        float x[3], nr[3], rot[9], vdir[3], vl[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = a.xyz[is * 3 + k];
            nr[k] = a.normal[is * 3 + k];
        }
        world2local(nr, rot);
        dir_to(a.cam, x, vdir);
        mat3_apply(rot, vdir, vl);
        unit3(vl);
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int l0 = 0; l0 < a.n_lights; l0 += 64) {
            const int l = l0 + lane;
            const bool valid = l < a.n_lights;
            const int lc = valid ? l : 0;
            const float lp[3] = {a.lxyz[lc * 3], a.lxyz[lc * 3 + 1], a.lxyz[lc * 3 + 2]};
            const float w[3] = {a.lweight[lc * 3], a.lweight[lc * 3 + 1], a.lweight[lc * 3 + 2]};
            float ldir[3], ll[3];
            dir_to(lp, x, ldir);
            mat3_apply(rot, ldir, ll);
            const float lz = ll[2];
            const bool fr = valid && lz > 0.0f && (w[0] != 0.0f || w[1] != 0.0f || w[2] != 0.0f);
            if (__ballot(fr) == 0ull) {
                if (a.idx && valid) a.idx[is * a.n_lights + l] = -1;
                continue;
            }
            unit3(ll);
            float q[3];
            rusink_of(ll, vl, q);
            float4 t;
            const int idx = lookup(a.tbl, q, fr, t);
            float term[3] = {0.0f, 0.0f, 0.0f};
            if (fr && idx >= 0) {
                term[0] = t.x * w[0] * lz;
                term[1] = t.y * w[1] * lz;
                term[2] = t.z * w[2] * lz;
            }
            if (a.idx && valid) a.idx[is * a.n_lights + l] = idx;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = term[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                sum[k] += v;
            }
        }
        if (lane == 0) {
            a.rgb[is * 3] = sum[0];
            a.rgb[is * 3 + 1] = sum[1];
            a.rgb[is * 3 + 2] = sum[2];
        }
    }
}

}  // namespace merl
}  // namespace nfx

extern "C" int nfx_launch_merl_query(const void* table4, const float* rusink, long long n, float* rgb, int* idx, hipStream_t st) {
    using namespace nfx;
    if (n <= 0) return 0;
    const long long want = (n + 255) / 256;
    const int grid = (int)(want < 65536 ? want : 65536);
    hipLaunchKernelGGL(merl::merl_query_kernel, dim3(grid), dim3(256), 0, st, (const float4*)table4, rusink, n, rgb, idx);
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_merl_sphere(const float* xyz, const float* normal, long long n, const float* cam3, const void* table4,
                                      const float* lxyz, const float* lweight, int n_lights, float* rgb, int* idx, hipStream_t st) {
    using namespace nfx;
    if (n <= 0) return 0;
    merl::SphereArgs a{xyz, normal, n, {cam3[0], cam3[1], cam3[2]}, (const float4*)table4, lxyz, lweight, n_lights, rgb, idx};
    const long long want = (n + 3) / 4;
    const int grid = (int)(want < 65536 ? want : 65536);
    hipLaunchKernelGGL(merl::merl_sphere_kernel, dim3(grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
