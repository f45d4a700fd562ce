"""The conditions tests/nerf_point_cases.py states about its own inputs, held by the oracle alone (no GPU): a point that is
given a neighbour's position or a neighbour ray's direction changes its value, both signs of the density occur, every layout is
the same 840 points, the ray edges of the layouts reach every lane position, and the tile sizes the cases rely on are the ones
in the kernel sources.  The thresholds are fixed: if an input misses one, its seed changes."""
import os
import re

import numpy as np
import pytest

from tests import nerf_point_cases as pc
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'nerfactor_amd', 'csrc')
DISTANCES = (1, 32, 64, 128, 256)


def test_constants_are_the_sources():
    for name, pattern in pc.SOURCE_CONSTANTS:
        assert re.search(pattern, open(os.path.join(CSRC, name)).read()), (name, pattern)
    assert pc.WAVE == 2 * pc.COL_TILE == 64 and pc.TILE == 256 and pc.TILE_X3 == 128 and pc.DEFAULT_BLOCKS == 256
    # 840 points: three 256-point tiles and 72 points (one full wave, 8 points of the next wave's column tile 0, two empty
    # waves); six 128-point tiles and 72 points
    assert pc.N == 840 == 3 * pc.TILE + pc.WAVE + 8 == 6 * pc.TILE_X3 + 2 * pc.COL_TILE + 8
    assert -(-pc.N // pc.TILE) == 4 and -(-pc.N // pc.TILE_X3) == 7       # nerf_blocks 1: one workgroup walks 4 / 7 tiles
    assert pc.N < pc.DEFAULT_BLOCKS * pc.TILE_X3                          # the default grid: one tile per workgroup


@pytest.mark.parametrize('name', pc.SETS)
def test_the_inputs_are_the_stated_construction(name):
    ps = pc.point_set(name)
    assert ps.rayo.shape == ps.rayd.shape == (8, 3) and ps.z.shape == (8, 105)
    assert all(a.dtype == np.float32 for a in (ps.rayo, ps.rayd, ps.z))
    np.testing.assert_allclose(np.linalg.norm(ps.rayd, axis=1), 1., atol=1e-6)
    lo, hi = (2., 6.) if name == 'glorot' else (2.5, 5.5)
    assert lo <= ps.z.min() and ps.z.max() <= hi and ps.z.max() - ps.z.min() > 0.9 * (hi - lo)
    # not sorted: neighbouring samples are far apart (a sorted ray of 105 samples would step by (hi - lo) / 105)
    assert np.median(np.abs(np.diff(ps.z, axis=1))) > 0.15 * (hi - lo)
    if name == 'glorot':
        assert np.abs(ps.rayo).max() <= 3.
    else:
        np.testing.assert_allclose(np.linalg.norm(ps.rayo, axis=1), 4., atol=1e-5)
        assert ((ps.rayd * -ps.rayo / 4.).sum(1) > 0.8).all()           # they look at the scene


@pytest.mark.parametrize('name', pc.SETS)
def test_a_misplaced_point_changes_a_value(name):
    """In the same-rounding oracle every point differs from the points at flat distance 1, 32, 64, 128 and 256 by more than 1e-3 in
    some rgb logit, and at least 99 % of them by more than 1e-4 in density."""
    v = pc.point_set(name).want('q')
    for dist in DISTANCES:
        d = pc.differs(v, dist)
        rgb, sig = d[:, :3].max(1), d[:, 3]
        print('%s distance %3d: min rgb move %.3e, min density move %.3e, %.2f %% above 1e-4' % (name, dist, rgb.min(), sig.min(), 100 * (sig > 1e-4).mean()))
        assert rgb.min() > 1e-3, (name, dist, rgb.min())
        assert (sig > 1e-4).mean() >= 0.99, (name, dist)


@pytest.mark.parametrize('name', pc.SETS)
def test_a_neighbour_ray_s_direction_changes_the_colour_and_not_the_density(name):
    """With the next base ray's direction (the point itself stays) every point's rgb logits move by more than 1e-2 and its
    density by exactly 0; the same with the previous one (a lane may take either neighbour's)."""
    ps = pc.point_set(name)
    for kind in ('q', 'f32'):
        for shift in (-1, 1):
            other = ps.eval(kind, rayd=np.roll(ps.rayd, shift, 0))
            move = np.abs(other - ps.want(kind))
            print('%s %s, direction of base ray %+d: min rgb move %.3e' % (name, kind, -shift, move[:, :3].max(1).min()))
            assert move[:, :3].max(1).min() > 1e-2, (name, kind, shift)
            assert np.array_equal(other[:, 3], ps.want(kind)[:, 3])


@pytest.mark.parametrize('name', pc.SETS)
def test_both_signs_of_the_density_occur(name):
    """10 % .. 90 % of the points have a positive raw density, in every oracle the same points up to a few on the edge: the
    gradient kernels' row list is neither empty nor everything."""
    ps = pc.point_set(name)
    for kind in ('q', 'f32', 'f64'):
        frac = (ps.want(kind)[:, 3] > 0).mean()
        print('%s %s: %.1f %% of the points have a positive density' % (name, kind, 100 * frac))
        assert 0.1 <= frac <= 0.9, (name, kind, frac)
    # the list is no multiple of the gradient kernels' tile: its last tile is a partial one
    assert int((ps.want('q')[:, 3] > 0).sum()) % pc.TILE_X3 not in (0, pc.TILE_X3 - 1)
    assert np.isfinite(ps.want('f64')).all() and ps.want('f64').dtype == np.float64


@pytest.mark.parametrize('name', pc.SETS)
def test_every_layout_is_the_same_points(name):
    ps = pc.point_set(name)
    o, d, z = ps.flat()
    assert o.shape == d.shape == (pc.N, 3) and z.shape == (pc.N,)
    assert np.array_equal(o, np.repeat(ps.rayo, 105, 0)) and np.array_equal(z, ps.z.reshape(-1))
    for s in pc.LAYOUTS:
        lo, ld, lz = ps.layout(s)
        assert lo.shape == ld.shape == (pc.N // s, 3) and lz.shape == (pc.N // s, s)
        ray = np.arange(pc.N) // s                                     # what the kernels compute
        assert np.array_equal(lo[ray].view(np.uint32), o.view(np.uint32))
        assert np.array_equal(ld[ray].view(np.uint32), d.view(np.uint32))
        assert np.array_equal(lz.reshape(-1).view(np.uint32), z.view(np.uint32))
    # the re-ordered launches name every point once
    for ro, rd, rz, idx in (ps.base_ray_order(np.arange(8)[::-1]), ps.sample_order(105, 1), ps.sample_order(7, 2)):
        s = rz.shape[1]
        assert np.array_equal(np.sort(idx), np.arange(pc.N))
        assert np.array_equal(rz.reshape(-1), z[idx]) and np.array_equal(ro[np.arange(pc.N) // s], o[idx])
        assert np.array_equal(rd[np.arange(pc.N) // s], d[idx]) and not np.array_equal(idx, np.arange(pc.N))


def test_the_ray_edges_reach_every_lane_position():
    """A ray edge at flat index e puts the first point of a new ray on lane position e % 64 of a 4 x 64 kernel's wave.  S = 105: 41,
    18, 59, 36, 13, 54 and 31: edges in both column tiles, in every wave (1, 3, 0, 2, 0, 1, 3 of its tile) and in the tiles 0, 1
    and 2; the last one starts a ray on the last lane of column tile 0, so that column tile 1 is wholly the new ray's while column
    tile 0 is not.  No multiple of 105 below 840 is a multiple of 32: an edge exactly between lanes 31 | 32, and one between
    two waves, comes from S = 3, 5 and 7: each of them puts an edge on every lane position, in tile 0 and again on later trips, and in both column
    tiles of every wave of every tile.  With S = 1 every point is an edge."""
    pos = [e % pc.WAVE for e in pc.ray_edges(105)]
    assert pos == [41, 18, 59, 36, 13, 54, 31]
    assert {p // pc.COL_TILE for p in pos} == {0, 1} and pc.COL_TILE - 1 in pos
    assert [e % pc.TILE // pc.WAVE for e in pc.ray_edges(105)] == [1, 3, 0, 2, 0, 1, 3]
    assert {e // pc.TILE for e in pc.ray_edges(105)} == {0, 1, 2}
    assert not [e for e in pc.ray_edges(105) if e % pc.COL_TILE == 0]
    for s in (3, 5, 7):
        # every wave of every tile holds edges in both of its column tiles (the last wave has 8 points: column tile 0 only)
        held = {(e // pc.TILE, e % pc.TILE // pc.WAVE, e % pc.WAVE // pc.COL_TILE) for e in pc.ray_edges(s)}
        assert held == {(t, w, c) for t in range(4) for w in range(4) for c in range(2) if t * pc.TILE + w * pc.WAVE + c * pc.COL_TILE < pc.N}
        assert {e % pc.WAVE for e in pc.ray_edges(s)} == set(range(64))
        assert {e % pc.WAVE for e in pc.ray_edges(s) if e >= pc.TILE} == set(range(64))       # ... on a later trip as well
    assert {e % pc.WAVE for s in pc.LAYOUTS for e in pc.ray_edges(s)} == set(range(64))
    assert all(105 % s == 0 for s in pc.LAYOUTS) and pc.LAYOUTS[0] == 105 and pc.LAYOUTS[-1] == 1


def test_the_sub_batches_meet_the_edges():
    pre = pc.prefixes()
    assert pre == [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 768, 769, 832, 833, 840]
    for t in (pc.COL_TILE, pc.WAVE, pc.TILE_X3, pc.TILE):
        assert {t - 1, t, t + 1} <= set(pre)
    assert pc.ray_prefixes() == [1, 2, 3, 4, 5, 6, 7, 8]
    pts = pc.sampled_points()
    assert 50 <= len(pts) <= 75 and pts[0] == 0 and pts[-1] == pc.N - 1 and len(set(pts)) == len(pts)
    for e in list(range(32, 257, 32)) + [512, 768] + pc.ray_edges():
        assert {e - 1, e} <= set(pts), e
    ch = pc.chunks()
    assert ch[0][0] == 0 and ch[-1][1] == pc.N and all(a[1] == b[0] for a, b in zip(ch[:-1], ch[1:]))
    assert all(a % pc.COL_TILE not in (0, 31) for a, _ in ch[1:])          # every cut falls inside a column tile
    assert {a % pc.WAVE // pc.COL_TILE for a, _ in ch[1:]} == {0, 1}       # ... of both
