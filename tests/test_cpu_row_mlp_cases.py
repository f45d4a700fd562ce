"""The conditions tests/row_mlp_cases.py states about its own inputs, held by the oracle alone (no GPU): the designed front-lit
counts are exact and far from the step, a misplaced row changes a value, the constants the shapes are derived from are the
ones in the kernel sources, and the cases together contain every shape property the GPU file relies on."""
import os
import re

import numpy as np
import pytest

from tests import row_mlp_cases as rc
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'nerfactor_amd', 'csrc')


def test_constants_are_the_sources():
    for name, pattern in rc.SOURCE_CONSTANTS:
        assert re.search(pattern, open(os.path.join(CSRC, name)).read()), (name, pattern)
    assert rc.LDS_NET == 136 * 1024 + 544 * 4 and rc.STREAM_TILE == 256 and rc.TILE_SIZES == [256, 384, 512]


def test_queue_limits_follow_from_the_constants():
    """Where brdf_compact_kernel hands a shape to the dense kernel: the LDS size binds before the ring does, for every form."""
    for ct in rc.COMPACT_CTS:
        assert rc.compact_limit(ct, 4) == 832 < rc.ring_limit(ct, 4)
        assert rc.compact_fits(ct, 4, 832) and not rc.compact_fits(ct, 4, 864)
    assert rc.compact_limit(2, 8) == 576 < rc.ring_limit(2, 8)
    assert rc.compact_fits(2, 8, 576) and not rc.compact_fits(2, 8, 608)
    # the bytes on both sides
    assert rc.compact_lds_bytes(4, 832) <= rc.LDS_MAX < rc.compact_lds_bytes(4, 864)
    assert rc.compact_lds_bytes(8, 576) <= rc.LDS_MAX < rc.compact_lds_bytes(8, 608)
    lights = {c.L for c in map(rc.case, rc.CASE_NAMES)}
    for ct, nw in [(2, 4), (3, 4), (4, 4), (2, 8)]:
        lim = rc.compact_limit(ct, nw)
        assert {lim, lim + 32} <= lights, (ct, nw, lim)
    full = rc.case('l832_full')
    assert full.L == full.above == rc.compact_limit(4, 4) and (full.signs > 0).sum() >= 4   # every wave of a workgroup meets the full ring


@pytest.mark.parametrize('name', rc.CASE_NAMES + ['pre'])
def test_front_lit_counts_are_the_designed_ones(name):
    c = rc.pre_case() if name == 'pre' else rc.case(name)
    lz = c.local_lz()
    assert lz.shape == (c.n, c.L) and c.L % 32 == 0
    assert np.array_equal((lz > 0).sum(1), c.front_count)
    assert np.abs(lz).min() >= 0.1
    lz64 = c.local_lz(np.float64)
    assert np.array_equal(lz64 > 0, lz > 0)
    nz = np.abs(c.normal[:, :2]).max(1) / np.linalg.norm(c.normal, axis=1)
    assert np.degrees(np.arcsin(nz)).min() > 20 * 0.5 and np.degrees(np.arccos(abs(rc.N_A[2]))) >= 20   # world2local is regular
    assert np.all(c.z != 0) and c.z.shape == (c.n, c.zd) and 1 <= c.zd <= rc.MAX_Z_DIM
    r = np.linalg.norm(c.lxyz, axis=1)
    assert r.min() >= 4 - 1e-5 and r.max() <= 8 + 1e-5 and np.abs(c.xyz).max() <= rc.BOX


@pytest.mark.parametrize('name', rc.CASE_NAMES)
def test_a_misplaced_brdf_row_changes_a_value(name):
    """at least 99 % of the front-lit rows differ from the row of the next light and from the row of the next point by more
    than 1e-4 in the float32 oracle"""
    c = rc.case(name)
    v, front = c.brdf(), c.local_lz() > 0
    assert np.all(v[front] > 0) and np.all(v[~front] == 0)
    assert rc.differs_from_next(v, 1)[front].mean() >= 0.99
    assert c.n == 1 or rc.differs_from_next(v, 0)[front].mean() >= 0.99


@pytest.mark.parametrize('name', rc.LVIS_CASES)
def test_a_misplaced_lvis_row_changes_a_value(name):
    c = rc.case(name)
    for other in (False, True):
        v = c.lvis(other_dir=other)
        assert rc.differs_from_next(v, 1).mean() >= 0.99
        assert c.n == 1 or rc.differs_from_next(v, 0).mean() >= 0.99
    assert np.abs(c.lvis() - c.lvis(other_dir=True)).max() > 1e-3       # xyz_dir is not xyz


def test_a_misplaced_xyz_row_changes_a_value():
    for head in rc.XYZ_HEADS:
        v = rc.xyz_head(head)
        assert v.shape == (1031, head[0])
        assert rc.differs_from_next(v, 0).mean() >= 0.99
        assert head[0] == 1 or rc.differs_from_next(v, 1).mean() >= 0.99    # ... and a misplaced output column


def _row_counts(c):
    return {k * c.L for k in rc.prefixes(c) + [c.n]}


def test_the_cases_contain_every_shape_property():
    cases = {n: rc.case(n) for n in rc.CASE_NAMES}
    lv = [cases[n] for n in rc.LVIS_CASES]
    # lights: 32, 96, 160 and 512.  160 divides no tile size and 96 only the 384 rows of the three-column-tile form (4 x 96), so
    # in every form at least one of the two makes tiles start at varying lights; both put several points into one tile
    assert {c.L for c in lv} == {32, 96, 160, 512}
    assert all(t % 160 for t in rc.TILE_SIZES) and [t for t in rc.TILE_SIZES if t % 96 == 0] == [384]
    # rows: below a tile, one column tile over and one short of it, for every tile size, in the dense and in the lvis cases
    for group in (lv, list(cases.values())):
        rows = set().union(*map(_row_counts, group))
        for t in rc.TILE_SIZES:
            assert min(rows) < t and {t - 32, t + 32} <= rows, t
    assert cases['one'].n == 1 and cases['one'].L == 32
    # at least 3 trips of every workgroup at m128_blocks 1 and 3, at every light count and in the largest tile
    for L in (32, 96, 160, 512):
        assert max(c.n * c.L for c in lv if c.L == L) >= 3 * 3 * max(rc.TILE_SIZES)
    # the xyz kernels
    assert rc.XYZ_N == (1, 255, 256, 257, 1031) and -(-1031 // rc.STREAM_TILE) == 5 and rc.pre_case().n == 1031
    assert {h[0] for h in rc.XYZ_HEADS} == {1, 3, 4, 5, 8}
    for i, off in ((1, None), (2, 1.), (3, 0.)):
        assert off in {h[i] for h in rc.XYZ_HEADS} and len({h[i] for h in rc.XYZ_HEADS}) >= 2
    # z_dim
    assert set(rc.Z_DIMS) >= {1, 2, 8, 9} and max(rc.Z_DIMS) == rc.MAX_Z_DIM
    # points below, equal to and above the number of waves of a grid of 1 and 3 workgroups
    for name in ('a1', 'a0_alt', 'a33'):
        assert {3, 4, 5, 11, 12, 13} <= set(rc.prefixes(cases[name]))
    assert rc.SMALL and all(cases[n].n <= 40 for n in rc.SMALL)
    assert all(len(rc.chunks(c)) <= 12 and rc.chunks(c)[0][0] == 0 and rc.chunks(c)[-1][1] == c.n for c in cases.values())


def _queue_stats(c, blocks, ct):
    return [rc.simulate_queue(c.front_count[pts], c.L, ct) for pts in rc.wave_points(c.n, blocks)]


def test_the_compaction_queue_meets_its_edges():
    """A host model of the fill / pass loop (row_mlp_cases.simulate_queue) on the cases' designed counts: which mechanism runs
    where.  m128_blocks 1 and 3: a wave then owns many points."""
    case = rc.case
    straddles = set()
    for blocks in (1, 3):
        for ct in rc.COMPACT_CTS:
            # a = 0, mixed signs: points with no row and with all L rows; runs of >= kSlots equal signs within a wave
            for name in ('a0_alt', 'a0_runs', 'a0_waves'):
                c = case(name)
                assert c.above == 0 and set(c.front_count) == {0, c.L}
            c = case('a0_runs')
            for pts in rc.wave_points(c.n, blocks):
                s = c.signs[pts]
                longest = max(len(r) for r in re.findall(r'1+|0+', ''.join('1' if v > 0 else '0' for v in s)))
                assert longest >= rc.K_SLOTS[4]
            # a = 1: the slot-span break fires again and again, partial passes in mid-stream
            st = _queue_stats(case('a1'), blocks, ct)
            assert all(s['breaks'] >= (2 if blocks == 1 else 1) and s['partial_mid'] >= s['breaks'] for s in st)
            assert all(s['max_span'] == rc.K_SLOTS[4] - 1 for s in st)      # the widest queue the break allows
            # a in {31, 33}: passes that straddle 2 .. 4 points
            for name in ('a33', 'a31'):
                st = _queue_stats(case(name), blocks, ct)
                straddles.update(s['max_straddle'] for s in st)
                assert any(s['decoded_head'] >= 1 for s in st)
        # 1 and 95 rows: a full pass leaves rows behind (k_head decoded from a ring entry), then one-row points until the break
        st = _queue_stats(case('a1_l96'), blocks, 2)
        assert sum(s['break_on_decoded'] for s in st) >= (4 if blocks == 1 else 1) and sum(s['partial_mid'] for s in st) >= 4
        # a = L at the largest L: the ring at its maximal fill, kPass - 1 + L can only be approached with rows left over
        c = case('l832_full')
        for ct in rc.COMPACT_CTS:
            st = _queue_stats(c, blocks, ct)
            assert max(s['max_fill'] for s in st) >= c.L
    assert {2, 3, 4} <= straddles
    # one pattern per wave of a one-workgroup launch
    c = case('a0_waves')
    w = [c.signs[p] for p in rc.wave_points(c.n, 1)]
    assert np.all(w[0] > 0) and np.all(w[1] < 0) and np.all(w[2][::2] > 0) and np.all(w[2][1::2] < 0)
    assert np.all(w[3][:rc.K_SLOTS[4] + 1] > 0) and np.all(w[3][rc.K_SLOTS[4] + 1:2 * rc.K_SLOTS[4] + 2] < 0)
    c = case('a31')
    w = [c.front_count[p] for p in rc.wave_points(c.n, 1)]
    assert set(w[0]) == {31} and set(w[1]) == {129} and set(w[2]) == {31, 129}


def test_the_ring_reaches_its_largest_fill():
    """The ring's bound is kPass - 1 + L entries: a pass's worth less one row queued, then a point with all L rows (the model
    takes it).  With the two front-lit counts of one case, 0 and L, a wave reaches L + L % kPass: two full points in a row,
    which waves 0 and 1 of a one-workgroup launch of l832_full own."""
    c = rc.case('l832_full')
    for ct in rc.COMPACT_CTS:
        st = rc.simulate_queue([ct * 32 - 1, c.L], c.L, ct)
        assert st['max_fill'] == ct * 32 - 1 + c.L <= rc.K_CAP[4]
    # in the case itself: two full points in a row on one wave leave L % kPass rows queued when the second arrives
    for ct in rc.COMPACT_CTS:
        st = rc.simulate_queue([c.L, c.L], c.L, ct)
        assert st['max_fill'] == c.L % (ct * 32) + c.L
    pts = rc.wave_points(c.n, 1)
    assert np.array_equal(c.front_count[pts[0]], [c.L, c.L]) and np.array_equal(c.front_count[pts[1]], [c.L, c.L])
