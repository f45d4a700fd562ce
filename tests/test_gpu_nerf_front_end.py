"""The one-point-per-lane front end of the render kernels of nerf_mlp_v6.hip (nerf_variant 7, 6, 8, plain and fold::): each
lane fetches and encodes the point of column tile `lane >> 5`, trades half of the encoding with lane ^ 32, and the LDS-DMA
kernel (7) fetches its inputs of the next point tile during the pass.  nerf_mlp.hip (nerf_variant 0)
keeps the per-lane front end: every lane fetches and encodes the points of both column tiles itself.  It is the reference.

1. The whole [N, S, 4] of variant 7, 6 and 8 equals variant 0's bit for bit, folded and unfolded, at point counts on both sides
   of the lane-half boundary (31 .. 33, 63 .. 65: own point valid and the partner's past the end, and the reverse), of a wave
   and of a tile, at five tiles plus nine points, on 1, 2, 3 and 256 workgroups (2 with the three tiles of 600 points or the five
   of 1100: one workgroup fetches ahead a tile that exists while the other's next tile does not), with S in 1, 3, 7, 64 and 65
   (65: a ray edge inside a column tile and between the two lanes of a pair).
2. z, rayo and rayd as views into larger buffers with NaN in front of and behind them: the same bits as from exact-size buffers.
   A clamped or fetched-ahead value never reaches a stored point.  (That no load leaves the arrays is by construction — every
   index is clamped to n_pts - 1 before it becomes an address — and cannot be shown by a test.)
3. Two launches on the same inputs return the same bits.

Inputs: unrelated rays and unsorted depths, the construction of tests/nerf_point_cases.PointSet('glorot'), whose network this
file uses; 1300 rays of it, of which every case takes a prefix."""
import numpy as np
import pytest
import torch

from tests import common, nerf_point_cases as pc

pytestmark = pytest.mark.gpu

VARIANTS = (7, 6, 8)
FOLDS = (1, 0)
BLOCKS = (1, 2, 3, 256)
SAMPLES = (1, 3, 7, 64, 65)
# the stated point counts; 130 = 2 x 65 and 325 = 5 x 65 (a tile and 69 points), so that S = 65 has ray edges; and 600 and 1100
# points = 3 and 5 tiles: the stated counts give 1, 2 and 6 tiles, which two workgroups share evenly
COUNTS = (1, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, 289, 1289, 130, 325, 600, 1100)
CASES = [(n, s) for n in COUNTS for s in SAMPLES if n % s == 0]
POOL = 1300
PAD = 37          # NaN elements / rows in front of and behind a view: odd, so that the views start off every 16-byte boundary

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pool():
    """(rayo [1300, 3], rayd [1300, 3], z [1300]) — unrelated rays, depths not sorted"""
    def make():
        rng = np.random.default_rng(5301)
        d = rng.normal(size=(POOL, 3))
        return (rng.uniform(-3, 3, size=(POOL, 3)).astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32),
                rng.uniform(2., 6., size=POOL).astype(np.float32))
    return cached('pool', make)


def inputs(n, s, cuda):
    """n points as [n / s, s]: the first n / s rays and the first n depths of the pool, on the device"""
    def make():
        o, d, z = pool()
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (o[:n // s], d[:n // s], z[:n].reshape(n // s, s)))
    return cached(('in', n, s), make)


def blob(cuda):
    from nerfactor_amd import ops
    return cached('blob', lambda: ops.pack_nerf_weights(*common.nerf_layers(pc.point_set('glorot').net), prec='bf16').to(cuda))


def run(nfx_opt, cuda, variant, fold, blocks, o, d, z):
    from nerfactor_amd import ops
    nfx_opt.set('nerf_variant', variant)
    nfx_opt.set('nerf_fold', fold)
    if blocks is None:
        nfx_opt.unset('nerf_blocks')
    else:
        nfx_opt.set('nerf_blocks', blocks)
    return ops.nerf_mlp_fwd(o, d, z, blob(cuda), 'bf16')


def reference(nfx_opt, cuda, fold, n, s):
    """variant 0 (nerf_mlp.hip, the per-lane front end) on the default grid: computed once per case, shared"""
    def make():
        out = run(nfx_opt, cuda, 0, fold, None, *inputs(n, s, cuda))
        assert out.shape == (n // s, s, 4) and bool(torch.isfinite(out).all())
        return out
    return cached(('ref', fold, n, s), make)


def test_the_cases_are_the_stated_ones():
    assert {n for n, _ in CASES} == set(COUNTS) and {s for _, s in CASES} == set(SAMPLES)
    assert {1, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, 289, 1289} <= set(COUNTS)
    assert 1289 == 5 * pc.TILE + 9 and max(COUNTS) <= POOL
    # nerf_blocks 2 with an odd number of tiles: workgroup 0 walks one tile more than workgroup 1, so it fetches ahead a tile
    # that exists while workgroup 1's next tile does not; nerf_blocks 3 with 5 tiles likewise
    assert [-(-n // pc.TILE) for n in (289, 325, 600, 1100, 1289)] == [2, 2, 3, 5, 6]
    # S = 65: ray edges at flat index 65, 130, ...: lane 1 of the second wave, inside column tile 0; with 325 points also 195 and 260
    assert (130, 65) in CASES and (325, 65) in CASES and 65 % pc.WAVE == 1


@pytest.mark.parametrize('fold', FOLDS)
@pytest.mark.parametrize('variant', VARIANTS)
def test_one_point_per_lane_equals_the_per_lane_front_end(nfx_lib, cuda, nfx_opt, variant, fold):
    for n, s in CASES:
        want = reference(nfx_opt, cuda, fold, n, s)
        for blocks in BLOCKS:
            got = run(nfx_opt, cuda, variant, fold, blocks, *inputs(n, s, cuda))
            common.assert_same_bits(want, got, 'nerf_variant %d, nerf_fold %d, [%d, %d], nerf_blocks %d against nerf_variant 0' % (
                variant, fold, n // s, s, blocks), row_len=4)


def framed(t):
    """a view of t's shape into a buffer with PAD rows of NaN in front of and behind it"""
    big = torch.full((t.shape[0] + 2 * PAD,) + tuple(t.shape[1:]), float('nan'), dtype=t.dtype, device=t.device)
    big[PAD:PAD + t.shape[0]] = t
    view = big[PAD:PAD + t.shape[0]]
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + PAD * t[0].numel() * 4
    assert bool(torch.isnan(big[:PAD]).all()) and bool(torch.isnan(big[PAD + t.shape[0]:]).all())
    return big, view


@pytest.mark.parametrize('variant', VARIANTS)
def test_nothing_from_outside_the_batch_reaches_a_stored_point(nfx_lib, cuda, nfx_opt, variant):
    for n in (289, 600, 1289):
        exact = inputs(n, 1, cuda)
        # z as ONE buffer of n + 2 PAD depths: [n, 1] is a view of its middle
        frames = [framed(t) for t in exact]
        for fold in FOLDS:
            for blocks in (1, 2):
                want = run(nfx_opt, cuda, variant, fold, blocks, *exact)
                got = run(nfx_opt, cuda, variant, fold, blocks, *(v for _, v in frames))
                assert bool(torch.isfinite(want).all())
                common.assert_same_bits(want, got, 'nerf_variant %d, nerf_fold %d, %d points, nerf_blocks %d: inputs framed in NaN against '
                                        'exact-size inputs' % (variant, fold, n, blocks), row_len=4)
                common.assert_same_bits(reference(nfx_opt, cuda, fold, n, 1), got, 'the same against nerf_variant 0', row_len=4)
        for (big, _), t in zip(frames, exact):       # the launches wrote nothing into their inputs
            assert bool(torch.isnan(big[:PAD]).all()) and bool(torch.isnan(big[PAD + n:]).all()) and torch.equal(big[PAD:PAD + n], t)


@pytest.mark.parametrize('variant', VARIANTS)
def test_two_launches_return_the_same_bits(nfx_lib, cuda, nfx_opt, variant):
    for fold in FOLDS:
        for n, s, blocks in ((1289, 1, None), (1289, 1, 2), (325, 65, 1), (33, 3, None)):
            first = run(nfx_opt, cuda, variant, fold, blocks, *inputs(n, s, cuda))
            second = run(nfx_opt, cuda, variant, fold, blocks, *inputs(n, s, cuda))
            assert first.data_ptr() != second.data_ptr()
            common.assert_same_bits(first, second, 'nerf_variant %d, nerf_fold %d, [%d, %d], nerf_blocks %s: second launch against the first' % (
                variant, fold, n // s, s, blocks), row_len=4)
