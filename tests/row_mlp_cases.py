"""Inputs and oracles for the forward width-128 row kernels (mlp128.hip, lvis_v2.hip, mlp128_x3.hip): no GPU here.

What the envmap grid cannot do, these inputs do:
  * lights are random directions at random radii 4 .. 8 around points in a +-0.3 box, so two neighbouring lights of a point,
    and two neighbouring points of a light, give clearly different rows;
  * the number of FRONT-LIT lights of a point is designed: all directions keep |n_a . d| > 0.35 against one tilted base
    normal n_a, and signs are flipped until exactly `a` of the L lights lie above its plane.  A point whose normal is +n_a
    (plus a small jitter) then has `a` front-lit lights, one with -n_a has L - a, and which point gets which sign is a free
    pattern (alternating, long runs, one pattern per wave of the compaction kernel);
  * the light counts are multiples of 32 that divide none of the tile sizes, sit on both sides of the limits at which the
    compaction kernel hands a shape to the dense kernel, and the point counts put n * L around every tile size.

The limits are derived below from the constants of lvis_v2.hip; tests/test_cpu_row_mlp_cases.py holds those constants to
the source text and the cases to the conditions stated here."""
import functools

import numpy as np

from oracle import nerf_ref, nerfactor_ref as R

# ---------------------------------------------------------------------------------------------- constants of the kernels
# (name of the source, pattern that must be found in it): test_cpu_row_mlp_cases.py
SOURCE_CONSTANTS = [
    ('lvis_v2.hip', r'constexpr int kRing = 1024;'),
    ('lvis_v2.hip', r'kCap = NW == 8 \? 704 : kRing, kSlots = NW == 8 \? 4 : 8;'),
    ('lvis_v2.hip', r'return kLdsNet \+ NW \* kCap \* \(int\)sizeof\(ring_t\) \+ \(n_lights \* 12 \+ 15\) / 16 \* 16 \+ NW \* kSlots \* 32 \* 4;'),
    ('lvis_v2.hip', r'typedef unsigned short ring_t;'),
    ('mlp128_resident.hpp', r'constexpr int kLdsNet = m128::kMainWeightBytes \+ m128::kMainBiasFloats \* 4;'),
    ('lvis_v2.hip', r'if \(CT \* 32 - 1 \+ a\.n_lights > lv2::Queue<NW>::kCap\) return -1;'),
    ('lvis_v2.hip', r'if \(lds > 160 \* 1024\) return -1;'),
    ('lvis_v2.hip', r'if \(cnt > 0 && kfill - k_head >= kSlots - 1\) break;'),
    ('lvis_v2.hip', r'constexpr int kTileRows = kNW \* CT \* 32;'),
    ('lvis_v2.hip', r'const long long want = \(a\.n \+ NW - 1\) / NW;'),
    ('mlp128_layout.hpp', r'constexpr int kMainFrags = 4 \* 4 \+ 4 \* 8 \+ 4 \* 8 \+ 4 \* 12 \+ 8;'),
    ('mlp128_layout.hpp', r'constexpr int kMainWeightBytes = kMainFrags \* 1024;'),
    ('mlp128_layout.hpp', r'constexpr int kMainBiasFloats = 4 \* 128 \+ 32;'),
    ('mlp128_layout.hpp', r'constexpr int kMaxZDim = 9;'),
    ('mlp128.hip', r'constexpr int kNW = 8; '),
    ('mlp128.hip', r'constexpr int kRowsPerTile = kNW \* 32;'),
    ('capi_nerfactor.cpp', r'nfx_option_int\("m128_blocks", 256\)'),
]
K_RING = 1024
K_CAP = {4: K_RING, 8: 704}
K_SLOTS = {4: 8, 8: 4}
LDS_NET = (4 * 4 + 4 * 8 + 4 * 8 + 4 * 12 + 8) * 1024 + (4 * 128 + 32) * 4
LDS_MAX = 160 * 1024
MAX_Z_DIM = 9
DEFAULT_BLOCKS = 256
STREAM_TILE = 8 * 32                                 # mlp128.hip: 8 waves x 32 rows
RESIDENT_TILES = {(2, 4): 256, (3, 4): 384, (4, 4): 512, (2, 8): 512}   # (CT, NW) -> NW * CT * 32 rows
TILE_SIZES = sorted(set(RESIDENT_TILES.values()) | {STREAM_TILE})
COMPACT_CTS = (2, 3, 4)


def compact_lds_bytes(nw, n_lights):
    """Queue<NW>::lds_bytes"""
    return LDS_NET + nw * K_CAP[nw] * 2 + (n_lights * 12 + 15) // 16 * 16 + nw * K_SLOTS[nw] * 32 * 4


def compact_fits(ct, nw, n_lights):
    """launch_compact / nfx_launch_brdf_spec_v3 take the shape (otherwise the dense kernel runs)"""
    return (n_lights <= 1024 and ct * 32 - 1 + n_lights <= K_RING and ct * 32 - 1 + n_lights <= K_CAP[nw] and
            compact_lds_bytes(nw, n_lights) <= LDS_MAX)


def compact_limit(ct, nw):
    """the largest light count (a multiple of 32) that brdf_compact_kernel<ct, ., nw> takes"""
    return max(L for L in range(32, 2048, 32) if compact_fits(ct, nw, L))


def ring_limit(ct, nw):
    """the same if only the ring bound: kPass - 1 + L <= kCap"""
    return max(L for L in range(32, 2048, 32) if ct * 32 - 1 + L <= K_CAP[nw])


# ------------------------------------------------------------------------------------------------------------- networks
def net128(seed, in_dims, out_dims, bias_scale=.2):
    """glorot-uniform width-128 network with non-zero biases (as tests/test_gpu_nerfactor.py::net128)"""
    rng = np.random.default_rng(seed)
    layers, out = R.init_mlp128(rng, in_dims, out_dims)
    for lst in (layers, out):
        for i, (k, b) in enumerate(lst):
            lst[i] = (k, rng.uniform(-bias_scale, bias_scale, size=b.shape).astype(np.float32))
    return layers, out


def f64(net):
    return [(k.astype(np.float64), b.astype(np.float64)) for k, b in net]


@functools.lru_cache(maxsize=None)
def brdf_net(zd):
    return net128(140 + zd, zd + 15, 1)


@functools.lru_cache(maxsize=None)
def lvis_net():
    return net128(130, 90, 1)


# ---------------------------------------------------------------------------------------------------------------- inputs
N_A = np.array([0.5, -0.4, 0.62]) / np.linalg.norm([0.5, -0.4, 0.62])    # 48 degrees off +z: world2local is regular there
LIGHT_MARGIN = 0.35
NORMAL_JITTER = 0.03
BOX = 0.3
CAM = np.array([2.4, -2.6, 1.8]) * 4 / np.linalg.norm([2.4, -2.6, 1.8])


def designed_lights(n_lights, above, seed):
    """[L, 3] float32 light positions: random directions with |n_a . d| > LIGHT_MARGIN at radii 4 .. 8, exactly `above`
    of them on the +n_a side, in random order."""
    assert 0 <= above <= n_lights
    rng = np.random.default_rng(seed)
    d = np.zeros((0, 3))
    while d.shape[0] < n_lights:
        c = rng.normal(size=(4 * n_lights, 3))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        d = np.concatenate((d, c[np.abs(c @ N_A) > LIGHT_MARGIN]))
    d = d[:n_lights]
    want = np.where(rng.permutation(n_lights) < above, 1., -1.)
    d = d * (want * np.sign(d @ N_A))[:, None]
    return (d * rng.uniform(4., 8., size=(n_lights, 1))).astype(np.float32)


# sign patterns: +1 = normal +n_a (`above` front-lit lights), -1 = normal -n_a (L - above)
def all_plus(n):
    return np.ones(n, int)


def alternating(n):
    return np.where(np.arange(n) % 2 == 0, 1, -1)


def runs(n, run):
    return np.where((np.arange(n) // run) % 2 == 0, 1, -1)


def mostly_plus(n, every=13):
    return np.where(np.arange(n) % every == every - 1, -1, 1)


def per_wave(n, nw=4):
    """One pattern per wave of a one-workgroup launch of brdf_compact_kernel<., ., 4>: a wave owns points gw + k nw, so its
    pattern is a function of (k, gw) = divmod(i, nw).  Wave 0: all +, wave 1: all -, wave 2: alternating in k, wave 3: runs
    of kSlots + 1 in k."""
    k, w = np.divmod(np.arange(n), nw)
    table = [np.ones_like(k), -np.ones_like(k), np.where(k % 2 == 0, 1, -1), np.where((k // (K_SLOTS[4] + 1)) % 2 == 0, 1, -1)]
    return np.choose(w % 4, table)


class Case:
    """One (points, lights) batch for the (point, light)-row kernels."""

    def __init__(self, name, n_lights, above, signs, zd, seed):
        rng = np.random.default_rng(seed)
        n = len(signs)
        self.name, self.L, self.above, self.n, self.zd, self.signs = name, n_lights, above, n, zd, np.asarray(signs)
        self.lxyz = designed_lights(n_lights, above, seed + 1)
        self.xyz = rng.uniform(-BOX, BOX, size=(n, 3)).astype(np.float32)
        # the points the light directions of the visibility MLP are taken from, when they are not the points themselves
        self.xyz_dir = (self.xyz + rng.uniform(-.05, .05, size=(n, 3))).astype(np.float32)
        self.cam = (CAM + rng.uniform(-.2, .2, size=(n, 3))).astype(np.float32)
        nrm = self.signs[:, None] * N_A + rng.uniform(-NORMAL_JITTER, NORMAL_JITTER, size=(n, 3))
        self.normal = (nrm * rng.uniform(.5, 2., size=(n, 1))).astype(np.float32)   # not unit length: the kernels normalise
        z = rng.normal(size=(n, zd))
        self.z = (np.sign(z) * np.maximum(np.abs(z), .05)).astype(np.float32)       # all of z non-zero
        self.front_count = np.where(self.signs > 0, above, n_lights - above)

    def __repr__(self):
        return self.name

    def take(self, idx):
        """the same case restricted to / re-ordered by the point indices `idx`"""
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        for k in ('xyz', 'xyz_dir', 'cam', 'normal', 'z', 'signs', 'front_count'):
            setattr(c, k, np.ascontiguousarray(getattr(self, k)[idx]))
        c.n = len(c.signs)
        return c

    # -------------------------------------------------------------------------------------------------------- oracles
    def local_lz(self, dtype=np.float32):
        """local l.z of every (point, light) row: what nerfactor.py:429-432 takes the sign of"""
        d = lambda a: a.astype(dtype)
        return np.einsum('nij,nlj->nli', R.gen_world2local(d(self.normal)), R.calc_ldir(d(self.xyz), d(self.lxyz)))[..., 2]

    def brdf(self, quant=None, dtype=np.float32):
        d = lambda a: a.astype(dtype)
        layers, out = brdf_net(self.zd)
        if dtype == np.float64:
            layers, out = f64(layers), f64(out)
        surf2l, surf2c = R.calc_ldir(d(self.xyz), d(self.lxyz)), R.calc_vdir(d(self.cam), d(self.xyz))
        return R.learned_spec(surf2l, surf2c, d(self.normal), d(self.z), {'brdf_mlp': layers, 'brdf_out': out}, quant=quant)

    def lvis(self, quant=None, dtype=np.float32, other_dir=False):
        d = lambda a: a.astype(dtype)
        layers, out = lvis_net()
        if dtype == np.float64:
            layers, out = f64(layers), f64(out)
        surf2l = R.calc_ldir(d(self.xyz_dir if other_dir else self.xyz), d(self.lxyz))
        return R.pred_lvis_at(d(self.xyz), surf2l, {'lvis_mlp': layers, 'lvis_out': out}, quant=quant)


# name -> (L, front-lit lights of a +n_a point, sign pattern, z_dim).  What each is for: test_cpu_row_mlp_cases.py
CASES_SPEC = {}
for _spec in [
        ('one',       32,  17,  all_plus(1),        3),    # a single live column tile, every other one clamped to row 0
        ('a0_alt',    32,  0,   alternating(40),    1),    # points with 0 and with all L rows, alternating
        ('a0_runs',   32,  0,   runs(300, 100),     2),    # ... in runs of >= kSlots points per wave at 1 and 3 workgroups
        ('a0_waves',  32,  0,   per_wave(150),      3),    # ... one pattern per wave
        ('a1',        32,  1,   mostly_plus(150),   9),    # one row per point: the slot-span break, partial passes in mid-stream
        ('a1_l96',    96,  1,   mostly_plus(150, 11), 2),   # 1 / 95 rows: the break fires on a queue whose head was decoded from the ring
        ('a33',       96,  33,  alternating(49),    2),    # 33 / 63 rows per point: passes that straddle 2 .. 4 points
        ('a31',       160, 31,  per_wave(29),       8),    # 31 / 129 rows per point
        ('l512',      512, 256, alternating(13),    3),    # the tile of the default forms: 13 tiles, every one starts at light 0
        ('l576',      576, 288, alternating(9),     9),    # the most lights the two-waves-per-SIMD queue takes
        ('l608',      608, 300, alternating(5),     1),    # ... and one step beyond
        ('l832_full', 832, 832, [1, 1, -1, 1, 1, 1], 3),   # the most lights of the one-wave-per-SIMD queue, all front-lit: ring at kPass - 1 + L
        ('l864',      864, 400, alternating(5),     2),    # one step beyond: the dense kernel
]:
    CASES_SPEC[_spec[0]] = _spec[1:]
CASE_NAMES = list(CASES_SPEC)
SMALL = [k for k, v in CASES_SPEC.items() if len(v[2]) <= 40]          # one launch per point
LVIS_CASES = ['one', 'a0_alt', 'a1', 'a33', 'a31', 'l512']            # L in {32, 96, 160, 512}
FP32_CASES = ['one', 'a0_alt', 'a33']
Z_DIMS = sorted({v[3] for v in CASES_SPEC.values()})


@functools.lru_cache(maxsize=None)
def case(name):
    n_lights, above, signs, zd = CASES_SPEC[name]
    return Case(name, n_lights, above, signs, zd, seed=1000 + 7 * CASE_NAMES.index(name))


@functools.lru_cache(maxsize=None)
def pre_case():
    """many points, few lights: the per-point kernel of the visibility MLP (lvis_pre_kernel) at the point counts XYZ_N"""
    return Case('pre', 32, 16, alternating(max(XYZ_N)), 3, seed=2000)


def wave_points(n, blocks, nw=4):
    """the points of every wave of brdf_compact_kernel<., ., nw> on a grid limited to `blocks` workgroups (launch_compact)"""
    grid = min(-(-n // nw), blocks)
    return [np.arange(gw, n, grid * nw) for gw in range(grid * nw)]


def simulate_queue(counts, n_lights, ct, nw=4):
    """Host model of the fill / pass loop of one wave of brdf_compact_kernel<ct, ., nw>; `counts` are the front-lit rows of
    the wave's points in its order.  Returns what happened: how often the slot-span break fired, partial passes that were
    not the wave's last, breaks on a queue whose oldest point was decoded from a ring entry, the largest ring fill, the most points a queue spanned and a pass straddled."""
    kpass, slots = ct * 32, K_SLOTS[nw]
    kfill = k_head = 0
    q, st = [], dict(breaks=0, partial_mid=0, max_fill=0, max_span=0, max_straddle=0, passes=0, rows=0, decoded_head=0, break_on_decoded=0)
    decoded = False
    while True:
        while len(q) < kpass:
            if kfill >= len(counts):
                break
            if q and kfill - k_head >= slots - 1:
                st['breaks'] += 1
                st['break_on_decoded'] += decoded
                break
            q += [kfill] * int(counts[kfill])
            kfill += 1
            st['max_fill'] = max(st['max_fill'], len(q))
        if not q:
            break
        rows = min(len(q), kpass)
        st['max_span'] = max(st['max_span'], kfill - q[0])
        st['max_straddle'] = max(st['max_straddle'], len(set(q[:rows])))
        st['partial_mid'] += rows < kpass and kfill < len(counts)
        st['passes'] += 1
        st['rows'] += rows
        q = q[rows:]
        decoded = bool(q)
        st['decoded_head'] += decoded
        k_head = q[0] if q else kfill
    assert st['max_fill'] <= kpass - 1 + n_lights <= K_CAP[nw] and st['max_span'] <= slots and st['rows'] == int(np.sum(counts))
    return st


def prefixes(c):
    """point counts k at which k * L sits below / one column tile short of / on / one column tile over a tile size, and around
    the number of waves of a grid of 1 and 3 workgroups of 4 waves"""
    ks = {1, 3, 4, 5, 11, 12, 13}
    for t in TILE_SIZES:
        for rows in (t - 32, t, t + 32, 2 * t - 32, 2 * t + 32):
            if rows % c.L == 0:
                ks.add(rows // c.L)
    return sorted(k for k in ks if 1 <= k < c.n)


def chunks(c):
    """contiguous chunks [a, b) of a larger case, of irregular lengths: the cuts fall inside tiles of every size"""
    scale, cuts, steps = max(1, c.n // 60), [0], (7, 13, 5, 17, 3, 11)
    while cuts[-1] < c.n:
        cuts.append(min(c.n, cuts[-1] + scale * steps[(len(cuts) - 1) % len(steps)]))
    return list(zip(cuts[:-1], cuts[1:]))


# ----------------------------------------------------------------------------------------------------- the xyz head kernels
XYZ_N = (1, 255, 256, 257, 1031)
XYZ_SCALE = 0.9
# (out_dim, out_act, post_scale, post_bias): 4 and 5 on both sides of the lane-half split of the store, 8 the last row
XYZ_HEADS = [(1, 'sigmoid', 1., 0.), (3, None, 1., 0.), (4, 'sigmoid', .77, .03), (5, None, 1.3, -.2), (8, 'sigmoid', 1., 0.),
             (8, None, .5, .25)]


@functools.lru_cache(maxsize=None)
def xyz_points():
    return np.random.default_rng(121).uniform(-1.2, 1.2, size=(max(XYZ_N), 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def xyz_net(out_dim):
    return net128(120 + out_dim, 63, out_dim)


def xyz_head(head, quant=None, dtype=np.float32):
    out_dim, act, scale, bias = head
    layers, out = xyz_net(out_dim)
    if dtype == np.float64:
        layers, out = f64(layers), f64(out)
    pe = nerf_ref.embed((np.float32(XYZ_SCALE) * xyz_points()).astype(dtype), 10)
    return scale * R.mlp128(pe, layers, out, act, quant=quant) + bias


def differs_from_next(v, axis, thresh=1e-4):
    """|v - v shifted by one along `axis`| > thresh (cyclic)"""
    return np.abs(v - np.roll(v, -1, axis)) > thresh
