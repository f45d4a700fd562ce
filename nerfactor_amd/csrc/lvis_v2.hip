// lvis_v2.hip — the two (point, light)-row MLPs of NeRFactor, light visibility (shape.py:213-237) and the learned-BRDF
// specular term (nerfactor.py:413-458), with the whole network RESIDENT in LDS.
// The width-128 net is 136 fragments = 136 KiB (+ 2 KiB of biases): it fits the 160 KiB of a CU, so unlike the NeRF
// kernels there is no weight stream, no staging and — after the one-time load — no barrier at all.  One wave per
// SIMD, CT column tiles of 32 (point, light) rows per wave: one A fragment read from LDS feeds CT MFMAs (CT = 4:
// a quarter of the LDS traffic of the 8 x 32 kernel in mlp128.hip), the epilogue of tile i-1 (accvgpr_read +
// v_cvt_pk_bf16_f32 + v_pk_max_i16 per pair) is issued in the shadow of tile i's MFMAs, the per-point
// pre-activations of layers 0 and 3 (lvis_pre_kernel) are fetched into the free accumulator set one tile ahead.
// MODE 0 = light visibility, MODE 1 = learned BRDF (same chunk geometry: 2 input k-steps, skip into layer 3; biases
// instead of per-point pre-activations, softplus on front-lit rows).  Same blobs and arithmetic as lvis_kernel /
// brdf_spec_kernel of mlp128.hip: bit-identical outputs.
// The resident network — its size and fragment offsets, the tile and the 17-tile ladder — is mlp128_resident.hpp; the
// learned-BRDF row in front of it (both geometries, the input slots, the bf16 cast) is brdf_row.hpp.  This file is the two
// kernels' dataflow around them.  (The one-time copy loop and brdf_compact_kernel's bf16 cast stay written out here: as
// inlined functions they change the instruction text of the default kernels, profiles/brdf_row/code_objects.txt.)
#include "brdf_row.hpp"
#include "mlp128_resident.hpp"
#include "launchers.hpp"

namespace nfx {
namespace lv2 {

using namespace res128;

constexpr int kNW = 4;
// MODE 0 additionally parks the per-point pre-activation rows of the wave's column tiles (CT x 1 KiB per wave), copied
// one point tile ahead: the layer-0 / layer-3 accumulators then start from LDS like a bias, not from a global load
constexpr int kLds = kLdsNet + kNW * 4 * 1024;

struct Args {
    const float* xyz;      // [n,3] points (lvis: the points the directions are taken from)
    const float* lxyz;     // [L,3]
    const float* pre;      // MODE 0: [n,256] per-point pre-activations
    const float* cam;      // MODE 1: [n,3]
    const float* normal;   // MODE 1: [n,3]
    const float* z;        // MODE 1: [n,z_dim]
    int z_dim;
    long long n;
    int n_lights;
    const char* blob;
    float* out;            // [n,L]
    // MODE 0, round 6 (both optional): row of point i in the caller's FULL [n_all, L] buffer (the tf.scatter_nd of
    // shape.py:171-176 done by the store itself: the compact [n, L] tensor is never written and never re-read), and the
    // tf.debugging.check_numerics flag: 1 is OR-ed into it when a visibility is NaN
    const int* out_row;
    int* nan_flag;
};

// NW = 4: one wave per SIMD with up to 512 registers (CT = 3 | 4).  NW = 8 (CT = 2): two waves per SIMD with 256
// registers each share the LDS copy of the network — a wave's stalls (epilogue bursts, the slow first tile of a
// layer, encoder VALU at the start of a point tile) are covered by its partner's MFMAs; an A fragment feeds 2 MFMAs,
// 64 B/clk of LDS reads per CU at full MFMA rate, a quarter of the ds_read_b128 peak.
// ROWS (MODE 0, round 6): the stores go to the rows Args::out_row names and NaNs raise Args::nan_flag.  A separate instantiation:
// the plain kernel keeps the exact code that 5e11 rows of soak have seen (255 registers, no scratch).
template <int CT, int MODE, int NW, bool ROWS = false>
__global__ __launch_bounds__(NW * 64, NW / 4) void resident128_kernel(Args a) {
    constexpr int kNW = NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace m128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
    {   // the whole network, once
        const u32x4* src = reinterpret_cast<const u32x4*>(a.blob);
        u32x4* dst = reinterpret_cast<u32x4*>(smem);
        for (int i = tid; i < kLdsNet / 16; i += kNW * 64) dst[i] = src[i];
        __syncthreads();
    }
    const char* wlds = smem;
    const float* bias_lds = reinterpret_cast<const float*>(smem + kMainWeightBytes);
    constexpr int kTileRows = kNW * CT * 32;
    const int n_lights = a.n_lights;
    const long long n_rows = a.n * n_lights;
    const long long n_tiles = (n_rows + kTileRows - 1) / kTileRows;
    float* pre_rows = reinterpret_cast<float*>(smem + kLdsNet) + wave * CT * 256;   // this wave's [CT][256] floats
    // point of column tile c in point tile t (clamped), and the copy of its pre row: one 16-byte piece per lane
    auto div_l = [&](long long v) -> long long { return v / n_lights; };
    auto mod_l = [&](long long v) -> int { return (int)(v % n_lights); };
    auto point_of = [&](long long t, int c) {
        const long long m = t * kTileRows + (wave * CT + c) * 32;
        return div_l(m < n_rows ? m : 0);
    };
    u32x4 stage[CT];
    auto fetch_rows = [&](long long t) {
        if constexpr (MODE == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                stage[c] = *reinterpret_cast<const u32x4*>(a.pre + point_of(t, c) * 256 + lane * 4);
        }
    };
    auto park_rows = [&]() {
        if constexpr (MODE == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) *reinterpret_cast<u32x4*>(pre_rows + c * 256 + lane * 4) = stage[c];
        }
    };
    fetch_rows(blockIdx.x);
    park_rows();
    // point position and light position of this lane's row in column tile c of point tile t, fetched one point tile
    // ahead: the first touch of a point's xyz is an HBM miss (~2-3 k cycles) that the first MFMA of the tile waited for
    float xq[CT][3], lq[CT][3];
    // ROWS: where column tile c of the NEXT point tile stores — out_row[point] * L + first light — as two wave-uniform words
    // (readfirstlane: SGPRs; the point index is computed here anyway, a division at the store would cost the registers the
    // kernel does not have)
    unsigned obq_lo[CT], obq_hi[CT];
    auto fetch_inputs = [&](long long t) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const long long m = t * kTileRows + (wave * CT + c) * 32;
            const long long mc = m < n_rows ? m : 0;
            const long long pt = div_l(mc);
            const int l0 = mod_l(mc);
            const int l = l0 + p;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xq[c][k] = a.xyz[pt * 3 + k];
                lq[c][k] = a.lxyz[l * 3 + k];
            }
            if constexpr (ROWS) {
                // everything scalar: the point index is wave-uniform, so its row comes by s_load (no vector-memory wait in
                // front of the prefetch — a readfirstlane of a vector LOAD made every tile wait for the loads it had just issued)
                const unsigned long long ptu = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)pt >> 32)) << 32) |
                                               __builtin_amdgcn_readfirstlane((unsigned)pt);
                const long long ob = (long long)a.out_row[ptu] * n_lights + __builtin_amdgcn_readfirstlane(l0);
                obq_lo[c] = (unsigned)ob;
                obq_hi[c] = (unsigned)((unsigned long long)ob >> 32);
            }
        }
    };
    fetch_inputs(blockIdx.x);
    unsigned long long bad = 0ull;      // lanes that saw a NaN: a ballot, wave-uniform — SGPRs, not one more VGPR (the kernel sits at 255)
    for (long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        bf16x8 pl[2][CT];
        const float* pre_pt[CT];
        const long long tnext = tl + gridDim.x < n_tiles ? tl + gridDim.x : tl;
        fetch_rows(tnext);   // next point tile's rows: in flight during this whole tile, parked after the last layer-3 initialiser
        long long m0[CT];
        bool front[CT];
        float xc[CT][3], lc[CT][3];
        unsigned ob_lo[CT], ob_hi[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xc[c][k] = xq[c][k];
                lc[c][k] = lq[c][k];
            }
            if constexpr (ROWS) {
                ob_lo[c] = obq_lo[c];
                ob_hi[c] = obq_hi[c];
            }
        }
        fetch_inputs(tnext);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            m0[c] = tl * kTileRows + (wave * CT + c) * 32;   // 32 consecutive lights of one point (n_lights % 32 == 0)
            const long long mc = m0[c] < n_rows ? m0[c] : 0;
            const long long pt = div_l(mc);
            float x[3], lp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[k] = xc[c][k];
                lp[k] = lc[c][k];
            }
            if constexpr (MODE == 0) {
                float d[3], sq = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    d[k] = lp[k] - x[k];   // _calc_ldir (shape.py:128-131): normalize(lxyz[l] - x), eps 1e-6
                    sq += d[k] * d[k];
                }
                const float inv = 1.0f / sqrtf(fmaxf(sq, 1e-6f));
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] *= inv;
                posenc<4, CT>(d, h, c, pl);
                pre_pt[c] = a.pre + pt * 256;
                front[c] = true;
            } else {
                float cm[3], nr[3], rus[3], v[16];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    cm[k] = a.cam[pt * 3 + k];
                    nr[k] = a.normal[pt * 3 + k];
                }
                front[c] = brdf_row_rusink(x, lp, cm, nr, rus);
                brdf_fill_slots(rus, a.z + pt * a.z_dim, a.z_dim, h, v);
                brdf_cast_slots(v, pl, c);
                pre_pt[c] = nullptr;
            }
        }
        Acc<CT> accs[2];
        // initial accumulators of the layer-0 / layer-3 tiles: per-point pre-activations (MODE 0) or plain biases
        auto init03 = [&](int off_pre, int off_bias) {
            return [=](int ln, Acc<CT>& ac) {
                if constexpr (MODE == 0) InitPre<CT>{pre_rows, off_pre}(ln, ac);
                else InitBias{bias_lds + off_bias}(ln, ac);
            };
        };
        // park: the rows of THIS point tile were last read by tile 14's initialiser (LDS ops of a wave are in order)
        ladder<CT>(wlds, bias_lds, lane, pl, accs, init03, park_rows);
        if (h == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (m0[c] < n_rows) {
                    const float o = accs[0].v[c][0];
                    if constexpr (MODE == 0) {
                        const float v = sigmoidf(o);                                    // shape.py:93 sigmoid out
                        if constexpr (ROWS) {
                            const long long at = (long long)(((unsigned long long)ob_hi[c] << 32) | ob_lo[c]);
                            a.out[at + p] = v;
                            bad |= __ballot(!(v == v));
                        } else {
                            a.out[m0[c] + p] = v;
                        }
                    } else {
                        a.out[m0[c] + p] = front[c] ? softplusf(o) : 0.0f;              // brdf.py:65, back-lit rows 0
                    }
                }
        }
    }
    if constexpr (ROWS) {
        if (a.nan_flag != nullptr && bad != 0ull && lane == 0) atomicOr(a.nan_flag, 1);
    }
}


// ------------------------------------------------------------------------------------------------------------------
// Learned-BRDF specular term with FRONT-LIT COMPACTION (nerfactor.py:429-441: the reference evaluates the BRDF MLP on
// the rows with local l.z > 0 only and scatters them into a zero tensor; about half of the light sphere).
// Every wave works alone (no barrier after the one-time network load): it owns the points gw, gw + NW, gw + 2 NW, ...
// (interleaved, so spatially coherent normals do not unbalance the waves), FILLS a private LDS ring with the
// front-lit (point, light) rows of its next point — ballot + mbcnt prefix, back-lit rows get their 0 right there —
// and whenever the ring holds a full pass (CT x 32 rows) runs the 17-tile network on rows that may straddle points.
// GEO = 0: the per-row geometry of resident128_kernel<CT, 1> (same functions, bit-identical outputs).
// GEO = 1: Rusinkiewicz angles without the two Rodrigues rotations' sin / cos and without the half-vector azimuth
//          (cos phi_h = h_x / s, sin phi_h = h_y / s, sin theta_h = s = |h_xy|), polynomial acos / atan2, and the
//          two-band encoding of the three angles from double-angle identities instead of 6 v_sin / v_cos.
// ring of queued rows per wave: 1024 entries of 16 bits = (point slot << 10) | light, point slot = local point index
// mod 8 (a pass decodes it against the index of the newest filled point; the fill loop never lets the queue span 8
// points).  2 KiB per wave: 8 waves (two per SIMD) fit next to the network.
constexpr int kRing = 1024;
typedef unsigned short ring_t;
// queue geometry per wave: ring entries and point slots.  4 waves: 1024 entries, 8 slots.  8 waves (two per SIMD):
// 704 entries (>= 64 - 1 + 512 lights), 4 slots — what fits beside the network, the lights and the point tables
template <int NW> struct Queue {
    static constexpr int kCap = NW == 8 ? 704 : kRing, kSlots = NW == 8 ? 4 : 8;
    static constexpr int lds_bytes(int n_lights) {
        return kLdsNet + NW * kCap * (int)sizeof(ring_t) + (n_lights * 12 + 15) / 16 * 16 + NW * kSlots * 32 * 4;
    }
};
__device__ __forceinline__ int ring_wrap(int i, int cap) { return i >= cap ? i - cap : i; }   // i < 2 cap

// The rows' values come from brdf_row.hpp.  brdf_compact_kernel lets the half-0 lane of column p compute the closed-form row
// (brdf_row_angles: the values of BOTH lane halves) of column tile 2k and the half-1 lane the row of tile 2k + 1, and swaps
// halves (one exchange per slot): each lane runs the geometry of CT / 2 rows instead of CT (the two halves used to compute
// the same row twice).  The per-POINT half (brdf_point_frame) is computed once per point by the queue fill and parked in LDS.
//
// NW = 8, CT = 2 (default since r03): two waves per SIMD — one wave's queue fill and Rusinkiewicz VALU run under its
//   partner's MFMAs.  NW = 4 (CT = 2 | 3 | 4): one wave per SIMD, the shipped form of round 2.
// Round 2 measured the 8-wave form faster but NOT deterministic (a few thousand of 10^8 rows wrong, in groups of 16
// lanes of the second column tile, different from run to run) and did not find out why.  Round 3 did: the exchange of
// the two lane halves' geometry by v_permlane32_swap_b32.  With a partner wave on the SIMD the swap reads operands a
// VALU instruction wrote two wait states earlier before they have landed — with the hand-placed `s_nop 1` of rounds
// 1-2 (hand-timed asm: 11 000 rows of 10^8 wrong per call) AND with the compiler's own
// __builtin_amdgcn_permlane32_swap, whose hazard recogniser places the same two wait states (2 200 rows).  Through
// ds_bpermute (__shfl_xor, the form that ships: the LDS crossbar, counted by lgkmcnt) the 8-wave kernel is
// bit-identical to the 4-wave one on every call (scripts/soak_8wave.py).  One wave per SIMD never showed the fault
// (10^10 rows in round 2), but the shipped form does not depend on those wait states any more.
template <int CT, int GEO, int NW>
__global__ __launch_bounds__(NW * 64, NW / 4) void brdf_compact_kernel(Args a) {
    constexpr int kNW = NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using namespace m128;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: point indices and ring base live in SGPRs
    {   // the whole network, once
        const u32x4* src = reinterpret_cast<const u32x4*>(a.blob);
        u32x4* dst = reinterpret_cast<u32x4*>(smem);
        for (int i = tid; i < kLdsNet / 16; i += kNW * 64) dst[i] = src[i];
        // the light positions too (<= 12 KiB): the queue fill classifies all of them for every point, and a pass
        // gathers one per row — LDS reads instead of global loads with a vmcnt(0) per 64 lights
        float* ldst = reinterpret_cast<float*>(smem + kLdsNet + kNW * Queue<NW>::kCap * (int)sizeof(ring_t));
        for (int i = tid; i < 3 * a.n_lights; i += kNW * 64) ldst[i] = a.lxyz[i];
        __syncthreads();
    }
    const float* lx = reinterpret_cast<const float*>(smem + kLdsNet + kNW * Queue<NW>::kCap * (int)sizeof(ring_t));
    const char* wlds = smem;
    const float* bias_lds = reinterpret_cast<const float*>(smem + kMainWeightBytes);
    constexpr int kCap = Queue<NW>::kCap, kSlots = Queue<NW>::kSlots;
    ring_t* ring = reinterpret_cast<ring_t*>(smem + kLdsNet) + wave * kCap;
    // per-point table of the wave (kPark): 8 slots (the ring's 3-bit point slot) x 32 floats =
    //   [x(3) | view dir in the local frame(3) | local frame t, b, n (9) | z_0 | z_1, z_3, .. (8) | z_2, z_4, .. (8)]
    constexpr bool kPark = GEO == 1 && CT % 2 == 0;
    float* ptab = reinterpret_cast<float*>(smem + kLdsNet + kNW * kCap * (int)sizeof(ring_t) + (a.n_lights * 12 + 15) / 16 * 16)
                  + wave * (kSlots * 32);
    const int L = a.n_lights;
    const long long n = a.n;
    const long long nw = (long long)gridDim.x * kNW, gw = (long long)blockIdx.x * kNW + wave;
    constexpr int kPass = CT * 32;
    long long kfill = 0, k_head = 0;   // next point to fill; point of the oldest queued row
    int head = 0, cnt = 0;
    for (;;) {
        // ---- fill: front-lit rows of the next points until a whole pass is queued (ring: kPass - 1 + L <= kRing)
        while (cnt < kPass) {
            const long long pt = gw + kfill * nw;
            if (pt >= n) break;
            if (cnt > 0 && kfill - k_head >= kSlots - 1) break;   // the queue may span at most kSlots points (point slot)
            // the point's position and normal: wave-uniform scalar loads (a partner wave's MFMAs cover their latency)
            float x[3], nr[3], rot[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[k] = a.xyz[pt * 3 + k];
                nr[k] = a.normal[pt * 3 + k];
            }
            world2local(nr, rot);
            if constexpr (kPark) {
                float cm[3], prot[9], pvl[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) cm[k] = a.cam[pt * 3 + k];
                brdf_point_frame(x, cm, nr, prot, pvl);
                const float* zp = a.z + pt * a.z_dim;
                float zv[17];
#pragma unroll
                for (int i = 0; i < 17; ++i) zv[i] = i < a.z_dim ? zp[i] : 0.0f;
                if (lane == 0) {
                    f32x4* ps = reinterpret_cast<f32x4*>(ptab + (int)(kfill & (kSlots - 1)) * 32);
                    ps[0] = f32x4{x[0], x[1], x[2], pvl[0]};
                    ps[1] = f32x4{pvl[1], pvl[2], prot[0], prot[1]};
                    ps[2] = f32x4{prot[2], prot[3], prot[4], prot[5]};
                    ps[3] = f32x4{prot[6], prot[7], prot[8], zv[0]};
                    ps[4] = f32x4{zv[1], zv[3], zv[5], zv[7]};
                    ps[5] = f32x4{zv[9], zv[11], zv[13], zv[15]};
                    ps[6] = f32x4{zv[2], zv[4], zv[6], zv[8]};
                    ps[7] = f32x4{zv[10], zv[12], zv[14], zv[16]};
                }
            }
            // the light of the NEXT 64-group is read while this one is classified (a lone wave has nothing else to
            // put under an LDS round trip)
            float lpn[3];
            {
                const int lc = lane < L ? lane : L - 1;
                lpn[0] = lx[lc * 3]; lpn[1] = lx[lc * 3 + 1]; lpn[2] = lx[lc * 3 + 2];
            }
            for (int l0 = 0; l0 < L; l0 += 64) {
                const int l = l0 + lane;
                const bool valid = l < L;
                const float lp[3] = {lpn[0], lpn[1], lpn[2]};
                if (l0 + 64 < L) {
                    const int ln = l + 64 < L ? l + 64 : L - 1;
                    lpn[0] = lx[ln * 3]; lpn[1] = lx[ln * 3 + 1]; lpn[2] = lx[ln * 3 + 2];
                }
                // (classifying by the sign of n . (light - x) instead — the normalisations are positive scalings — measured
                // 1 % and flips 1 row in 10^8 where the product rounds to 0: not taken)
                float ldir[3], ll[3];
                dir_to(lp, x, ldir);
                mat3_apply(rot, ldir, ll);
                const bool fr = valid && ll[2] > 0.0f;                    // nerfactor.py:429-432
                const unsigned long long mask = __ballot(fr);
                const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                if (fr) ring[ring_wrap(head + cnt + pos, kCap)] = (ring_t)(((kfill & (kSlots - 1)) << 10) | l);
                else if (valid) a.out[pt * L + l] = 0.0f;                 // scatter_nd's zeros
                cnt += __popcll(mask);
            }
            ++kfill;
        }
        if (cnt == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int rows = cnt < kPass ? cnt : kPass;
        // ---- pass: CT column tiles of 32 queued rows
        bf16x8 pl[2][CT];
        long long orow[CT];
        long long rpt[CT];
        int rl[CT], rslot[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int r = c * 32 + p;
            const bool ok = r < rows;
            const unsigned e = ring[ring_wrap(head + (ok ? r : 0), kCap)];
            rslot[c] = (int)(e >> 10);
            const long long kk = (kfill - 1) - (((kfill - 1) - (long long)(e >> 10)) & (kSlots - 1));   // slot -> local point index
            rpt[c] = gw + kk * nw;
            rl[c] = (int)(e & 1023u);
            orow[c] = ok ? rpt[c] * L + rl[c] : -1;
        }
        if constexpr (GEO == 1 && CT % 2 == 0) {
            // lane half h runs the geometry of the row of column tile 2k + h; one lane-half exchange per input slot
            // hands each half its own values of both rows (brdf_row_angles; the per-point half comes from the table)
#pragma unroll
            for (int k2 = 0; k2 < CT; k2 += 2) {
                const int l = h ? rl[k2 + 1] : rl[k2];
                const f32x4* ps = reinterpret_cast<const f32x4*>(ptab + (h ? rslot[k2 + 1] : rslot[k2]) * 32);
                const f32x4 q0 = ps[0], q1 = ps[1], q2 = ps[2], q3 = ps[3];
                const float x[3] = {q0[0], q0[1], q0[2]}, vl[3] = {q0[3], q1[0], q1[1]};
                const float rot[9] = {q1[2], q1[3], q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2]};
                const float lp[3] = {lx[l * 3], lx[l * 3 + 1], lx[l * 3 + 2]};
                float S[8], C[8];
                brdf_row_angles(x, lp, rot, vl, S, C);
                float v[2][16];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    // S = [half 0: S(row 2k) ; half 1: S(row 2k+1)], C likewise; swap(S.hi, C.lo):
                    //   first  = [S(row 2k) ; C(row 2k)]     = slot q of column tile 2k for both halves
                    //   second = [S(row 2k+1) ; C(row 2k+1)] = slot q of column tile 2k + 1
                    float first = S[q], second = C[q];
                    // the exchange through ds_bpermute (LDS crossbar, counted by lgkmcnt), not v_permlane32_swap: the kernel's header
                    const float recv = __shfl_xor(h ? first : second, 32, 64);
                    first = h ? recv : first;
                    second = h ? second : recv;
                    v[0][q] = first;
                    v[1][q] = second;
                }
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    // the latent code of the row's point: z_0 (slot 7 of half 1) and this half's z_{1 + 2j + h}
                    const f32x4* pz = reinterpret_cast<const f32x4*>(ptab + rslot[k2 + cc] * 32);
                    const int hs = h;
                    const f32x4 za = pz[4 + 2 * hs], zb = pz[5 + 2 * hs];
                    if (hs) v[cc][7] = pz[3][3];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[cc][8 + j] = za[j];
                        v[cc][12 + j] = zb[j];
                    }
#pragma unroll
                    for (int sidx = 0; sidx < 2; ++sidx) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) pl[sidx][k2 + cc][j] = (__bf16)v[cc][8 * sidx + j];
                    }
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const long long pt = rpt[c];
                const int l = rl[c];
                float x[3], lp[3], cm[3], nr[3];
                const float* zsrc = a.z + pt * a.z_dim;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    x[k] = a.xyz[pt * 3 + k];
                    lp[k] = lx[l * 3 + k];
                    cm[k] = a.cam[pt * 3 + k];
                    nr[k] = a.normal[pt * 3 + k];
                }
                float v[16];
                brdf_row_inputs<GEO>(x, lp, cm, nr, zsrc, a.z_dim, h, v);
#pragma unroll
                for (int sidx = 0; sidx < 2; ++sidx) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) pl[sidx][c][j] = (__bf16)v[8 * sidx + j];
                }
            }
        }
        Acc<CT> accs[2];
        ladder<CT>(wlds, bias_lds, lane, pl, accs, [&](int, int off_bias) { return InitBias{bias_lds + off_bias}; }, [] {});
        if (h == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (orow[c] >= 0) a.out[orow[c]] = softplusf(accs[0].v[c][0]);   // brdf.py:65
        }
        head = ring_wrap(head + rows, kCap);
        cnt -= rows;
        if (cnt > 0) {
            const unsigned e = ring[head];
            k_head = (kfill - 1) - (((kfill - 1) - (long long)(e >> 10)) & (kSlots - 1));
        } else {
            k_head = kfill;
        }
    }
}

}  // namespace lv2
}  // namespace nfx

template <int CT, int MODE, int NW = 4, bool ROWS = false>
static int launch_res(const nfx::lv2::Args& a, int max_blocks, hipStream_t st) {
    using namespace nfx;
    const long long rows = a.n * a.n_lights, tile_rows = NW * CT * 32;
    const long long tiles = (rows + tile_rows - 1) / tile_rows;
    const int grid = (int)(tiles < max_blocks ? tiles : max_blocks);
    constexpr int lds = lv2::kLdsNet + NW * CT * 1024;
    static_assert(lds <= 160 * 1024, "LDS");
    auto k = lv2::resident128_kernel<CT, MODE, NW, ROWS>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(NW * 64), lds, st, a);
    return (int)hipGetLastError();
}

extern "C" int nfx_launch_lvis_v2(const float* xyz, long long n, const float* lxyz, int n_lights, const float* pre,
                                  const void* blob_main, float* lvis, int ct, int max_blocks, hipStream_t st,
                                  const int* out_row, int* nan_flag) {
    if (n <= 0) return 0;
    nfx::lv2::Args a{xyz, lxyz, pre, nullptr, nullptr, nullptr, 0, n, n_lights, (const char*)blob_main, lvis, out_row, nan_flag};
    if (out_row != nullptr) {     // (a NaN flag alone: the caller passes the identity rows — capi_nerfactor.cpp refuses it)
        if (ct == 8) return launch_res<2, 0, 8, true>(a, max_blocks, st);
        return launch_res<4, 0, 4, true>(a, max_blocks, st);     // variants 2 | 3 | 4: the one-wave-per-SIMD reference form
    }
    if (ct == 8) return launch_res<2, 0, 8>(a, max_blocks, st);   // variant 8: 8 waves x 2 column tiles
    if (ct == 2) return launch_res<2, 0>(a, max_blocks, st);
    if (ct == 3) return launch_res<3, 0>(a, max_blocks, st);
    return launch_res<4, 0>(a, max_blocks, st);
}

extern "C" int nfx_launch_brdf_spec_v2(const float* xyz, const float* cam, const float* normal, const float* z,
                                       int z_dim, const float* lxyz, int n_lights, const void* blob, long long n,
                                       float* spec, int ct, int max_blocks, hipStream_t st) {
    if (n <= 0) return 0;
    nfx::lv2::Args a{xyz, lxyz, nullptr, cam, normal, z, z_dim, n, n_lights, (const char*)blob, spec, nullptr, nullptr};
    if (ct == 2) return launch_res<2, 1>(a, max_blocks, st);
    if (ct == 3) return launch_res<3, 1>(a, max_blocks, st);
    return launch_res<4, 1>(a, max_blocks, st);
}

template <int CT, int GEO, int NW>
static int launch_compact(const nfx::lv2::Args& a, int max_blocks, hipStream_t st) {
    using namespace nfx;
    const long long want = (a.n + NW - 1) / NW;       // at least one point per wave
    const int grid = (int)(want < max_blocks ? want : max_blocks);
    const int lds = lv2::Queue<NW>::lds_bytes(a.n_lights);   // network + row rings + lights + per-point tables
    if (CT * 32 - 1 + a.n_lights > lv2::Queue<NW>::kCap) return -1;
    if (lds > 160 * 1024) return -1;   // (the caller falls back to the dense kernel)
    auto k = lv2::brdf_compact_kernel<CT, GEO, NW>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(NW * 64), lds, st, a);
    return (int)hipGetLastError();
}

// Front-lit compaction (brdf_compact_kernel).  geo: 0 = reference op sequence per row, 1 = closed-form Rusinkiewicz.
// ct: 8 = 8 waves x 2 column tiles (two waves per SIMD); 2 | 3 | 4 column tiles per wave, one wave per SIMD (anything else: 4).
// Returns -1 when the shape does not fit the row queue (the caller falls back to the dense kernel).
extern "C" int nfx_launch_brdf_spec_v3(const float* xyz, const float* cam, const float* normal, const float* z,
                                       int z_dim, const float* lxyz, int n_lights, const void* blob, long long n,
                                       float* spec, int ct, int geo, int max_blocks, hipStream_t st) {
    if (n <= 0) return 0;
    const int tiles = ct == 8 ? 2 : ct;
    if (n_lights > 1024 || tiles * 32 - 1 + n_lights > nfx::lv2::kRing) return -1;   // (launch_compact checks its own ring)
    nfx::lv2::Args a{xyz, lxyz, nullptr, cam, normal, z, z_dim, n, n_lights, (const char*)blob, spec};
    if (ct == 8) return geo ? launch_compact<2, 1, 8>(a, max_blocks, st) : launch_compact<2, 0, 4>(a, max_blocks, st);
    if (ct == 2) return geo ? launch_compact<2, 1, 4>(a, max_blocks, st) : launch_compact<2, 0, 4>(a, max_blocks, st);
    if (ct == 3) return geo ? launch_compact<3, 1, 4>(a, max_blocks, st) : launch_compact<3, 0, 4>(a, max_blocks, st);
    return geo ? launch_compact<4, 1, 4>(a, max_blocks, st) : launch_compact<4, 0, 4>(a, max_blocks, st);
}

