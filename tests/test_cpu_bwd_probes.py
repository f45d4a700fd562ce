"""The conditions tests/bwd_probes.py states about its own inputs, checked without a GPU: every shipped probe keeps its
margins, the NeRF points are exact, the probe gradients are non-zero where stated, and the constants the row positions are
derived from are the ones in the kernel sources."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bwd_probes as bp
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'nerfactor_amd', 'csrc')


SETS = {name: (lambda name=name: bp.xyz_probes(name)) for name in bp.XYZ_NETS}
SETS.update(ldir=bp.ldir_probes, nerf=bp.nerf_probes, brdf_rows=bp.brdf_rows_probes)
SETS.update({'brdf_spec_z%d' % zd: (lambda zd=zd: bp.brdf_spec_probes(zd)) for zd in bp.BRDF_SPEC_ZDIMS})


def _sets():
    return [make() for make in SETS.values()]


def test_constants_are_the_sources():
    for name, pattern in bp.SOURCE_CONSTANTS:
        assert re.search(pattern, open(os.path.join(CSRC, name)).read()), (name, pattern)
    assert bp.TILE_ROWS == 4 * bp.WAVE_ROWS and bp.NERF_TILE_ROWS == 8 * bp.WAVE_ROWS
    assert bp.N_SWEEP == 260 and bp.N_SWEEP % bp.TILE_ROWS == 4
    nl, n = bp.LDIR_SWEEP
    assert bp.TILE_ROWS // nl == 4 and (nl * n) % bp.TILE_ROWS != 0
    rays, s = bp.NERF_SWEEP
    assert rays * s == 2 * bp.TILE_ROWS + 5 and bp.TILE_ROWS % s != 0 and bp.NERF_TILE_ROWS % s != 0
    rays, s = bp.NERF_PAIR
    assert rays * s > bp.LIST_BLOCK and bp.LIST_BLOCK % s == 0
    assert bp.BRDF_SWEEP[0] % bp.BRDF_LIGHT_MULTIPLE == 0
    assert bp.ldir_wide_rows() == [(0, 0), (0, 127), (0, 128), (0, 511), (1, 0), (1, 511)]
    assert bp.edge_rows(1) == [0] and bp.edge_rows(129) == [0, 128]


@pytest.mark.parametrize('which', sorted(SETS))
def test_margins_hold_for_every_shipped_probe(which):
    """Condition 1 against the r.m.s. over all the draws, condition 2 at the set's margin (>= the 1e-6 the device's
    Cody-Waite sine alone would need)."""
    p = SETS[which]()
    assert p.name == which and p.enc.shape[0] == bp.N_PROBES >= 8
    halves = [(p.pre, p.draw_pre, p.enc)]
    if which == 'brdf_rows':
        halves.append((p.pre_reci, p.draw_pre_reci, p.enc_reci))
    margin = bp.BRDF_SPEC_ENC_MARGIN if p.name.startswith('brdf_spec') else bp.ENC_MARGIN
    assert margin >= 1e-6
    for pre, draw, enc in halves:
        for z, zd in zip(pre, draw):
            rms = float(zd.pow(2).mean().sqrt())
            assert float(z.abs().min()) > bp.RELU_MARGIN * rms
        assert not bool(bp.near_bf16_boundary(enc, margin).any())
        lo, hi = bp.bf16(enc - margin), bp.bf16(enc + margin)
        assert torch.equal(lo, hi) and torch.equal(lo, bp.bf16(enc))
    # the share of robust rows the selection drew from: not a needle in a haystack
    share = float(bp.robust_rows(p.draw_pre, p.draw_enc, margin).double().mean())
    assert share > 0.05, share


def test_nerf_points_are_exact():
    p = bp.nerf_probes()
    i = p.inputs
    for a, step in ((i['rayo'], 2. ** -8), (i['rayd'], 2. ** -8), (i['z'], 2. ** -6)):
        assert np.array_equal(np.round(a / step) * step, a) and float(np.abs(a).max()) < 4.
    p32 = bp.nerf_points(i['rayo'], i['rayd'], i['z'], np.float32)
    p64 = bp.nerf_points(i['rayo'], i['rayd'], i['z'], np.float64)
    assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p64)
    # and the same for every filler row of the sweeps (the rows next to the probe are finite, exact inputs too)
    for rays, s in (bp.NERF_SWEEP, bp.NERF_PAIR):
        f = bp.nerf_fill(rays, s)
        for j in range(s):
            a, b = (bp.nerf_points(f['rayo'], f['rayd'], f['z'][:, j], t) for t in (np.float32, np.float64))
            assert np.array_equal(a.astype(np.float64), b)
    assert float(np.abs(i['rayd']).max()) * 8 <= 8.5      # the 4-band encoder's measured range


def test_light_directions_start_from_exact_differences():
    p = bp.ldir_probes()
    for f in (p.inputs, bp.ldir_fill(*bp.LDIR_SWEEP[::-1]), bp.ldir_fill(*bp.LDIR_WIDE[::-1])):
        d32 = f['lxyz'][:, None, :] - f['xyz_dir'][None, :, :]
        d64 = f['lxyz'].astype(np.float64)[:, None, :] - f['xyz_dir'].astype(np.float64)[None, :, :]
        assert np.array_equal(d32.astype(np.float64), d64) and float(np.linalg.norm(d64, axis=-1).min()) > 1.


def test_probe_gradients_are_nonzero_where_stated():
    for p in _sets():
        assert bool((p.g != 0).all()), p.name
    g = bp.nerf_probes().g_kinds
    assert bool((g['density'][:, :3] == 0).all()) and bool((g['density'][:, 3] != 0).all())
    assert bool((g['colour'][:, 3] == 0).all()) and bool((g['colour'][:, :3] != 0).all())
    assert np.array_equal(g['density'] + g['colour'], g['full'])


def test_reciprocal_half_adds_pi_in_fp32():
    p = bp.brdf_rows_probes()
    r = bp.reciprocal(p.inputs['rusink'])
    assert r.dtype == np.float32 and np.array_equal(r[:, 0], (p.inputs['rusink'][:, 0] + bp.PI32).astype(np.float32))
    assert np.array_equal(r[:, 1:], p.inputs['rusink'][:, 1:])


def test_spec_probes_are_front_lit_off_the_edge():
    for zd in bp.BRDF_SPEC_ZDIMS:
        assert float(bp.brdf_spec_probes(zd).lz.min()) > bp.BRDF_SPEC_MIN_NL


def test_spec_probes_leave_the_bound_its_factor_over_the_oracles_own_floor():
    """d_z and d_normal are projections of the input gradient: the float64 oracle with and without the per-layer bf16 rounding
    of dZ may sit further apart than the bound on a row that meets conditions 1 and 2 (bwd_probes.brdf_spec_probes).  The
    shipped probes keep that floor under bound / 3.5, and most rows do."""
    for zd in bp.BRDF_SPEC_ZDIMS:
        p = bp.brdf_spec_probes(zd)
        for k in range(bp.N_PROBES):
            fl = bp.spec_floor(p, k)
            assert fl == p.floor[k] and max(fl) <= bp.TOL_BRDF / bp.FLOOR_FACTOR, (zd, k, fl)
        kept = np.mean([max(fl) <= bp.TOL_BRDF / bp.FLOOR_FACTOR for fl in p.floors.values()])
        assert kept > 1 / 3, (zd, kept)
        # the finding the condition answers: among the first eight rows of conditions 1 and 2 alone the oracle pair is beyond
        # the bound itself (4.27e-2 at z_dim 3; 3.32e-2, 3.03e-2, 5.48e-2 at z_dim 1)
        first = [max(p.floors[int(i)]) for i in p.two_conditions[:bp.N_PROBES]]
        assert sum(f > bp.TOL_BRDF for f in first) == (1 if zd == 3 else 3), (zd, first)


def test_oracles_have_a_gradient_in_every_tensor():
    """a probe whose oracle gradient vanished in a tensor could not hold the kernel to anything there"""
    for name in bp.XYZ_NETS:
        p = bp.xyz_probes(name)
        assert all(float(g.abs().max()) > 0 for g in bp.mlp128_oracle(p, 0))
    assert all(float(g.abs().max()) > 0 for g in bp.mlp128_oracle(bp.ldir_probes(), 0))
    p = bp.nerf_probes()
    assert all(float(g.abs().max()) > 0 for g in bp.nerf_oracle(p, 0))
    dens, col = bp.nerf_oracle(p, 0, 'density'), bp.nerf_oracle(p, 0, 'colour')
    for layer in (9, 10, 11):          # bottleneck and both colour layers: untouched by a density-only gradient
        assert dens[layer] is None or not bool(dens[layer].any())
    assert col[8] is None or not bool(col[8].any())
    dz, dn = bp.brdf_spec_oracle(bp.brdf_spec_probes(3), 0)
    assert float(dz.abs().max()) > 0 and float(dn.abs().max()) > 0


def test_input_recovery_on_an_exact_outer_product():
    x = bp.bf16(torch.randn(7, dtype=torch.float64))
    d = bp.bf16(torch.randn(5, dtype=torch.float64))
    d[2] = 0.
    dw = torch.outer(x, d).float()
    assert bp.input_recovery(dw, d.float(), x) == (0, 4)
    dw[3, 1] = dw[3, 1] * (1 + 2. ** -20)
    assert bp.input_recovery(dw, d.float(), x)[0] == 1
