"""Inputs and oracles for the NeRF point kernels (nerf_mlp_v6.hip and nerf_sigma_v6.hip on nerf_v6_engine.hpp, nerf_mlp.hip,
nerf_mlp_x3.hip, nerf_geom.hip and nerf_geom_x3.hip on nerf_geom_body.hpp, nerf_sigma_x3_pipe.hip): no GPU here.

Every one of these kernels gives a lane the flat point index m, reads z[m] and finds the ray with ray = m / n_samples.  What
the older shapes cannot do, these inputs do:
  * 840 points = 8 base rays x 105 samples.  840 is three 256-point tiles plus 72 points: the last tile holds one full wave,
    one wave that ends 8 points into its column tile 0 and two empty waves; for the 128-point tiles it is 6 tiles plus 72;
  * 105 = 3 . 5 . 7: the same 840 points, in the same flat order, are handed over as [840 / S, S] for every S in LAYOUTS, each
    base ray split into equal parts that repeat its origin and direction.  With S = 105 the ray edges fall at lane positions
    41, 18, 59, 36, 13, 54 and 31 of a 64-point wave; with S = 3, 5 and 7 at every position, in every wave and tile;
  * z is NOT sorted and the base rays are unrelated, so the points next to a point in flat order, and the points 32, 64, 128
    and 256 further on, have clearly different values, and every point's colour moves when it is given its neighbour ray's
    direction (tests/test_cpu_nerf_point_cases.py holds the thresholds).

tests/test_cpu_nerf_point_cases.py holds the constants below to the source text and the inputs to the conditions stated here."""
import functools

import numpy as np

from oracle import nerf_ref
from tests import common

# ---------------------------------------------------------------------------------------------- constants of the kernels
# (name of the source, pattern that must be found in it): test_cpu_nerf_point_cases.py
SOURCE_CONSTANTS = [
    # nerf_v6_engine.hpp: the tile of the render kernels (nerf_mlp_v6.hip) and of the density kernels (nerf_sigma_v6.hip), once
    ('nerf_v6_engine.hpp', r'constexpr int kNW = 4, kCT = 2;'),
    ('nerf_v6_engine.hpp', r'constexpr int kTilePts = kNW \* 32 \* kCT;'),
    ('nerf_mlp_v6.hip', r'm\[c\] = tl \* kTilePts \+ wave \* \(32 \* kCT\) \+ c \* 32 \+ p;'),
    ('nerf_mlp_v6.hip', r'const long long mm = m\[c\] < n_pts \? m\[c\] : n_pts - 1;\s*const long long ray = mm / n_samples;'),
    # the one density body: position m -> sample src(m) -> ray; every sample is src(m) = m, a listed one src(m) = list[m]
    ('nerf_sigma_v6.hip', r'const long long m = tl \* kTilePts \+ wave \* \(32 \* kCT\) \+ c \* 32 \+ p;'),
    ('nerf_sigma_v6.hip', r'const long long mm = src\(m < n_pts \? m : n_pts - 1\);\s*const long long ray = mm / n_samples;'),
    ('nerf_sigma_v6.hip', r'struct EverySample \{[^}]*operator\(\)\(long long m\) const \{ return m; \}'),
    ('nerf_sigma_v6.hip', r'struct ListedSample \{[^}]*operator\(\)\(long long m\) const \{ return list\[m\]; \}'),
    ('nerf_sigma_v6.hip', r'nerf_sigma_v6_body\(rayo, rayd, zbuf, n_pts, n_samples, blob, out, EverySample\{\}\);'),
    ('nerf_sigma_v6.hip', r'nerf_sigma_v6_body\(rayo, rayd, zbuf, n_pts, n_samples, blob, out, ListedSample\{list\}\);'),
    ('nerf_mlp.hip', r'return launch_variant<2, 4>\('),
    ('nerf_mlp.hip', r'return launch_variant<1, 8>\('),
    ('nerf_mlp.hip', r'return launch_variant<2, 4, true>\('),
    ('nerf_mlp.hip', r'return launch_variant<1, 8, true>\('),
    ('nerf_mlp.hip', r'constexpr int kTilePts = NW \* 32 \* CT;'),
    ('nerf_mlp.hip', r'const long long mm = m\[c\] < n_pts \? m\[c\] : n_pts - 1;\s*const long long ray = mm / n_samples;'),
    ('mlp_x3.hpp', r'constexpr int kNW = 4;'),
    ('nerf_mlp_x3.hip', r'constexpr int kTilePts = kNW \* 32;'),
    ('nerf_mlp_x3.hip', r'const long long mm = m < n_pts \? m : n_pts - 1;\s*const long long ray = mm / n_samples;'),
    # nerf_geom_body.hpp: the density march (the gradient kernels hold the same lines in their __global__ functions); a policy's kNW waves x 32 points per tile
    ('nerf_geom_body.hpp', r'constexpr int kRows = A::kNW \* 32;'),
    ('nerf_geom_body.hpp', r'const long long row = tile \* kRows \+ wave \* 32 \+ p;\s*const bool valid = row < n_pts;\s*const long long mm = pts.sample\(row, n_pts\);'),
    ('nerf_geom.hip', r'constexpr int kNW = 4;\s*constexpr int kRows = kNW \* 32;'),
    ('nerf_geom.hip', r'static constexpr int kNW = NW;'),
    ('nerf_geom.hip', r'using A = Bf16<kNW>;'),
    ('nerf_geom.hip', r'const long long row = tile \* kRows \+ wave \* 32 \+ p;\s*const bool valid = row < n;\s*const long long mm = pts.sample\(row, n\);'),
    ('nerf_geom.hip', r'constexpr int NW = 8;'),
    ('nerf_geom.hip', r'constexpr int kTilePts = NW \* 32;'),
    ('nerf_geom.hip', r'nerf_sigma_body<Bf16<NW>>\(pts, blob, out, smem\);'),
    ('nerf_geom_x3.hip', r'constexpr int kNW = x3::kNW;\s*constexpr int kRows = kNW \* 32;'),
    ('nerf_geom_x3.hip', r'static constexpr int kNW = x3::kNW;'),
    ('nerf_geom_x3.hip', r'const long long row = tile \* kRows \+ wave \* 32 \+ p;\s*const bool valid = row < n;\s*const long long mm = pts.sample\(row, n\);'),
    ('nerf_sigma_x3_pipe.hip', r'constexpr int kNW = x3::kNW;\s*constexpr int kRows = kNW \* 32;'),
    ('nerf_sigma_x3_pipe.hip', r'const long long row = tl \* kRows \+ wave \* 32 \+ p;\s*const bool valid = row < n_pts;\s*const long long mm = pts.sample\(row, n_pts\);'),
    # nerf_points.hpp: position m -> flat sample (every sample, listed, last sample of ray m) -> ray, and where the density goes
    ('nerf_points.hpp', r'long long mm = m < n_pts \? m : n_pts - 1;\s*if \(list != nullptr\) mm = list\[mm\];\s*else if \(last_sample\) mm = \(mm \+ 1\) \* n_samples - 1;'),
    ('nerf_points.hpp', r'const long long ray = mm / n_samples;\s*const float zz = z\[mm\];'),
    ('nerf_points.hpp', r'if \(list != nullptr \|\| last_sample\) out\[list_stride \* \(mm \+ 1\) - 1\] = sigma;\s*else out\[m\] = sigma;'),
    ('nerf_points.hpp', r'return list != nullptr \? mm : m;'),
    ('nerf_points.hpp', r'n = \*count;\s*if \(\(long long\)blockIdx.x \* tile_rows >= n\) return false;'),
    ('capi.cpp', r'nfx_option_int\("nerf_blocks", 256\)'),
    ('capi.cpp', r'nfx_option_int\("nerf_variant", 7\)'),
]
WAVE = 64                     # points of a wave of the 4 x 64 kernels: two column tiles of 32
COL_TILE = 32
TILE = 4 * 32 * 2             # nerf_v6_engine.hpp (nerf_mlp_v6.hip, nerf_sigma_v6.hip), nerf_mlp.hip <2, 4> and <1, 8>, nerf_sigma_geo_kernel (8 x 32)
TILE_X3 = 4 * 32              # nerf_mlp_x3.hip, nerf_geom.hip, nerf_geom_x3.hip, nerf_sigma_x3_pipe.hip
DEFAULT_BLOCKS = 256

N_RAYS, N_SAMPLES = 8, 105
N = N_RAYS * N_SAMPLES
LAYOUTS = (105, 35, 21, 15, 7, 5, 3, 1)
SETS = ('glorot', 'fitted')


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class PointSet:
    """840 points as 8 base rays x 105 samples and a network."""

    def __init__(self, name):
        self.name = name
        if name == 'glorot':
            rng = np.random.default_rng(4101)
            self.net = common.nerf_nets(seed=7)[0]
            self.rayo = rng.uniform(-3, 3, size=(N_RAYS, 3)).astype(np.float32)
            self.rayd = _unit(rng.normal(size=(N_RAYS, 3))).astype(np.float32)
            self.z = rng.uniform(2., 6., size=(N_RAYS, N_SAMPLES)).astype(np.float32)
        else:
            from tests.golden import golden_inputs as gi
            rng = np.random.default_rng(4202)
            self.net = gi.trained_nerf_nets()[1]
            o = 4. * _unit(rng.normal(size=(N_RAYS, 3)))
            self.rayo = o.astype(np.float32)
            self.rayd = _unit(-o / 4. + .15 * rng.normal(size=(N_RAYS, 3))).astype(np.float32)
            self.z = rng.uniform(2.5, 5.5, size=(N_RAYS, N_SAMPLES)).astype(np.float32)
        for a in (self.rayo, self.rayd, self.z):
            a.setflags(write=False)

    def __repr__(self):
        return self.name

    # --------------------------------------------------------------------------------------------------------- layouts
    def layout(self, s):
        """(rayo [840 / s, 3], rayd [840 / s, 3], z [840 / s, s]): every base ray in 105 / s parts that repeat its origin and
        direction; the flat point order is the same for every s"""
        assert N_SAMPLES % s == 0
        rep = N_SAMPLES // s
        return (np.repeat(self.rayo, rep, 0), np.repeat(self.rayd, rep, 0), np.ascontiguousarray(self.z.reshape(N // s, s)))

    def flat(self):
        """(o [840, 3], d [840, 3], z [840]) of every point, in flat order"""
        o, d, z = self.layout(1)
        return o, d, z.reshape(-1)

    def base_ray_order(self, order):
        """the S = 105 layout with its base rays in another order: (rayo, rayd, z, flat index of every point of the launch)"""
        order = np.asarray(order)
        idx = (order[:, None] * N_SAMPLES + np.arange(N_SAMPLES)[None, :]).reshape(-1)
        return self.rayo[order].copy(), self.rayd[order].copy(), self.z[order].copy(), idx

    def sample_order(self, s, seed):
        """the layout s with another random sample order inside every ray: (rayo, rayd, z, flat index of every point)"""
        rng = np.random.default_rng(seed)
        o, d, z = self.layout(s)
        perm = np.stack([rng.permutation(s) for _ in range(N // s)])
        idx = (np.arange(N // s)[:, None] * s + perm).reshape(-1)
        return o, d, np.take_along_axis(z, perm, 1), idx

    # --------------------------------------------------------------------------------------------------------- oracles
    def eval(self, kind, rayd=None):
        """[840, 4] (rgb logits, raw density) of every point: 'f32' the float32 oracle, 'q' the same with the kernels' bf16
        operand rounding, 'f64' float64; `rayd`: other view directions [8, 3] than the rays' own (the points stay)"""
        dt = np.float64 if kind == 'f64' else np.float32
        o, d, z = self.rayo.astype(dt), self.rayd.astype(dt), self.z.astype(dt)
        pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
        views = np.broadcast_to((d if rayd is None else rayd.astype(dt))[:, None, :], pts.shape)
        v = nerf_ref.eval_nerf_at(pts, views, self.net, quant=nerf_ref.bf16_round if kind == 'q' else None)
        assert v.dtype == dt
        return v.reshape(N, 4)

    @functools.lru_cache(maxsize=None)
    def want(self, kind):
        """the oracle values of every point: computed once, shared, never written to"""
        v = self.eval(kind)
        v.setflags(write=False)
        return v


@functools.lru_cache(maxsize=None)
def point_set(name):
    return PointSet(name)


# ------------------------------------------------------------------------------------------------------------ sub-batches
def prefixes():
    """point counts for the [P, 1] layout: around every column tile, wave and tile edge, the last wave's edge and the whole"""
    return [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 768, 769, 832, 833, 840]


def ray_prefixes():
    """the first 1 .. 8 base rays of the S = 105 layout"""
    return list(range(1, N_RAYS + 1))


def ray_edges(s=N_SAMPLES):
    """flat index of the first point of every ray of the layout s but the first"""
    return list(range(s, N, s))


def sampled_points():
    """about 60 points: both sides of every 32-point edge of tile 0, of every 256-point edge and of every base-ray edge, the
    points around the end of the last full wave, every 37th point and the last one"""
    pts = {0, N - 1, 831, 832, 833}
    for e in list(range(COL_TILE, TILE + 1, COL_TILE)) + list(range(TILE, N, TILE)) + ray_edges():
        pts |= {e - 1, e}
    pts |= set(range(0, N, 37))
    return sorted(pts)


def chunks():
    """contiguous chunks [a, b) of irregular lengths whose cuts all fall inside column tiles"""
    cuts = [0, 98, 280, 350, 588, 630, 784, N]
    return list(zip(cuts[:-1], cuts[1:]))


def differs(v, dist):
    """|v[i] - v[i + dist]| of every pair of points at flat distance `dist`"""
    return np.abs(v[:-dist] - v[dist:])
