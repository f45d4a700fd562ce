"""The conditions under which tests/test_gpu_generic_exact.py may ask for equality, proved from each case's own data
(tests/generic_exact_cases.py) — not from interval bounds — and the coverage of the case set.  No GPU needed."""
import os

import numpy as np
import pytest

from oracle import nerf_ref
from tests import generic_exact_cases as G
from tests.conftest import ROOT

NAMES = sorted(G.SHAPES)


def test_bf16_round_is_round_to_nearest_even_on_ties():
    """integers between 256 and 512 are 2 apart in bf16: odd ones are ties"""
    got = nerf_ref.bf16_round(np.array([257, 259, 261, 263, -257, -259, 256, 258, 513, 514, 515, 518, 65535], np.float32))
    assert got.tolist() == [256, 260, 260, 264, -256, -260, 256, 258, 512, 512, 516, 520, 65536]
    hi, lo = G.hi_lo(np.array([257, 511, 65535, 40001, -12345], np.int64))
    assert (hi + lo).tolist() == [257, 511, 65535, 40001, -12345]          # 16 significant bits: the pair is the value


def test_float64_product_is_the_int64_product():
    rng = np.random.default_rng(0)
    a, b = rng.integers(-4000, 4000, size=(70, 300)), rng.integers(-4000, 4000, size=(300, 50))
    assert np.array_equal(G.imatmul(a, b), a @ b) and G.imatmul(a, b).dtype == np.int64


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_every_sum_is_exact_in_fp32(name, prec):
    """worst = max over every accumulator the three kernels form — forward layers (+ bias), transposed dgrad, the input
    gradient summed over the layers that read x, dW = IN^T dZ and db over ALL rows (+ what the buffers held) — of the sum of
    |products|, with the operands as the matrix pipe sees them (pairs mode: |hi| + |lo|).  All terms are integers, so any
    order of summation, any row split and any MFMA form yields the same fp32 number."""
    r = G.reference(name, prec)
    assert r.worst < 2 ** 24, r.worst
    if prec == 'fp32':
        assert r.peak < 2 ** 16, r.peak        # hi + lo is the value itself
        assert G.dropped_lo_lo(name) == [0] * len(G.case(name).layers)      # dW = IN^T dZ drops lo x lo of two ACTIVATIONS: none here
    c = G.case(name)
    for k, b in c.layers:
        assert set(np.unique(k)) <= {-1, 0, 1}
        hi, lo = G.hi_lo(k)
        assert not lo.any()                    # the weights' lo plane is zero: forward and dgrad drop nothing
    assert np.abs(c.x).max() <= 3 and np.abs(c.dy).max() <= (9 if name == 'two_skips' else 1)
    assert np.array_equal(G.bf16(c.x), c.x) and np.array_equal(G.bf16(c.dy), c.dy)
    # the batch is prefixes of the same rows: smaller launches sum subsets of these terms


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_the_case_is_not_blind(name, prec):
    c, r = G.case(name), G.reference(name, prec)
    for i, h in enumerate(r.hs):
        if c.acts[i] == 'relu':
            never = float(((h > 0).sum(0) == 0).mean())
            assert never <= 0.10, (i, never)
    y = r.y
    if y.shape[1] >= 3:
        differs = (y[:-32] != y[1:-31]).any(1) & (y[:-32] != y[32:]).any(1)
        assert differs.mean() >= 0.95, differs.mean()
    # pre-activations that are exactly 0 decide the mask convention, and masked units exist on most rows
    zeros = sum(int(((r.ins[i] @ c.layers[i][0] + c.layers[i][1]) == 0).sum()) for i in range(len(c.layers)) if c.acts[i] == 'relu')
    assert zeros >= 20, zeros
    # gradients reach every tensor, the edge rows included
    dws, dbs = G.weight_grads(name, prec, G.N_MAX)
    for i in range(len(c.layers)):
        assert (dws[i] != c.dw0[i]).mean() > 0.3 and (dbs[i] != c.db0[i]).any(), i
    for row in (0, 31, 32, 127, 128, 288, G.N_MAX - 1):
        assert r.dx[row].any() and c.dy[row].any(), row
    if prec == 'bf16' and name in ('wide288', 'w256x8_skip4'):       # the bf16 roundings act, forward and backward
        exact = G.reference(name, 'fp32_native')
        assert r.peak > 256 and not np.array_equal(exact.y, y)
    if prec == 'bf16' and name == 'two_skips':
        exact = G.reference(name, 'fp32_native')       # (dy up to 9: the rounding of the propagated gradients acts too)
        assert max(int(np.abs(d).max()) for d in r.dzs) > 256 and not np.array_equal(exact.dx, r.dx)


@pytest.mark.parametrize('name', NAMES)
def test_every_fragment_holds_a_non_zero(name):
    """every 16-row k-step of every 32-column tile of every layer's weights (the forward's A fragment), and every 32-row tile
    x 16-column k-step (the transposed fragment of the dgrad): a fragment fetched from the wrong place changes a number"""
    c = G.case(name)
    for i, (k, _) in enumerate(c.layers):
        prev = c.widths[i - 1] if i else 0
        for part in ([k[:prev], k[prev:]] if prev and k.shape[0] > prev else [k]):      # hidden rows and skip rows: own fragments
            for r0 in range(0, part.shape[0], 16):
                for c0 in range(0, part.shape[1], 32):
                    assert part[r0:r0 + 16, c0:c0 + 32].any(), (i, r0, c0)
            for r0 in range(0, part.shape[0], 32):
                for c0 in range(0, part.shape[1], 16):
                    assert part[r0:r0 + 32, c0:c0 + 16].any(), ('transposed', i, r0, c0)


def test_the_cases_cover_the_code_paths():
    insts = {(prec,) + G.instantiation(name, prec, n) for name in NAMES for prec in G.PRECS for n in G.ROWS}
    assert insts == {('bf16', 1, False), ('bf16', 1, True)} | {(p, nw, False) for p in ('fp32', 'fp32_native') for nw in (1, 2, 4)} \
        | {(p, 1, True) for p in ('fp32', 'fp32_native')}
    # NW = 1 of the fp32 modes at a FULL batch (not only because one row tile leaves nothing to share), and every NW at N_MAX
    at_full = {G.instantiation(name, 'fp32', G.N_MAX) for name in NAMES}
    assert at_full == {(1, False), (2, False), (4, False), (1, True)}
    assert G.instantiation('in539', 'fp32', G.N_MAX) == (1, False) and G.instantiation('w96x4_skip1', 'fp32', 33) == (2, False)
    cs = [G.case(n) for n in NAMES]
    assert {c.d_in for c in cs} >= {3, 27, 63, 283, 539} and all(d % 16 for d in (3, 27, 63, 283, 539))
    assert {c.widths[-1] for c in cs} >= {1, 3, 4, 5, 33}
    tiles = {G.n_tiles(w) for c in cs for w in c.widths}
    assert {9, 2, 7} <= tiles and any(G.n_tiles(w) == 2 and w == 40 for c in cs for w in c.widths)      # 288 -> 9, 40 -> 2 (half empty), 200 -> 7
    assert any(c.skip_at == [0, 1] for c in cs) and any(0 in c.skip_at for c in cs) and any(len(c.widths) == 9 for c in cs)
    assert sum(len(c.widths) == 1 for c in cs) >= 1
    assert any(c.acts[-1] == 'relu' for c in cs) and any(c.acts[-1] is None for c in cs)
    for name in NAMES:
        s, cuts = G.wgrad_splits(name, G.N_MAX)
        assert s == 10 and len({t1 - t0 for t0, t1 in cuts}) == 2, (name, s, cuts)      # several UNEVEN splits
        s3, cuts3 = G.wgrad_splits(name, G.N_MAX, cap=3)
        assert s3 == 3 and len({t1 - t0 for t0, t1 in cuts3}) == 2
        assert G.wgrad_splits(name, 289)[0] == 2 and G.wgrad_splits(name, 129)[0] == 1
    # under nerf_blocks = 1 (8 waves in all) 289 rows = 10 row tiles: two waves walk a second tile; under 3, N_MAX's 41 > 24
    assert (289 + 31) // 32 > 8 and (G.N_MAX + 31) // 32 > 24 and G.N_MAX % 32 not in (0, 1)


def test_restated_host_decisions_match_the_source():
    hip = open(os.path.join(ROOT, 'nerfactor_amd', 'csrc', 'mlp_generic.hip')).read()
    cpp = open(os.path.join(ROOT, 'nerfactor_amd', 'csrc', 'capi_generic.cpp')).read()
    for text in ('static constexpr int kRingGroups = 3;', 'static constexpr int kFrag = 32 * 16 * kElem;', 'if (a.mode == kBf16) return 1;',
                 'if (wide_layers(a)) return 1;', 'if (a.layer[l].n_tiles > 8) return true;', 'int nw = 4;',
                 'while (nw > 1 && (ring + nw * act > 160 * 1024 || tiles < nw)) nw /= 2;',
                 'act = 32 * (a.x_pitch + a.h_pitch);', 'const int ring = a.mode == kBf16 ? P<kBf16>::kRingBytes : P<kNative>::kRingBytes;',
                 # one dispatch for the forward and the backward kernel: NW = 4 | 2 in the fp32 modes only, else WIDE or not
                 'if constexpr (M != kBf16) {', 'if (nw == 4) return launch<M, 4, false>(args, grid, lds, st);',
                 'if (nw == 2) return launch<M, 2, false>(args, grid, lds, st);',
                 'if (wide_layers(f)) return launch<M, 1, true>(args, grid, lds, st);', 'return launch<M, 1, false>(args, grid, lds, st);',
                 'return launch_for<NFX_GENERIC_TU>(args, *args, nw, grid, lds, st);', 'launch_for<NFX_GENERIC_TU>(ba, ba->f, nw, grid, lds, st)',
                 'const long long t0 = a.tiles * sp / a.splits, t1 = a.tiles * (sp + 1) / a.splits;',
                 'const long long wgs = (tiles + nw - 1) / nw, cap = max_blocks / nw > 0 ? max_blocks / nw : 1;'):
        assert text in hip, text
    for text in ('a->x_pitch = (a->d_in + 63) / 64 * 64 * elem + 16;', 'a->h_pitch = (widest + 1) / 2 * 64 * elem + 16;',
                 'long long s = (8192 + n_jobs - 1) / n_jobs;', 'if (s > tiles / 4) s = tiles / 4;',
                 'const int cap = nfx_option_int("wgrad_splits", 256);',
                 'jobs += ((m_in + 1) / 2) * ((L.n_tiles + 1) / 2);', '8 * nfx_option_int("nerf_blocks", 256)',
                 'wa.map = nfx_option_int("wgrad_map", 1);'):
        assert text in cpp, text
    assert G.pitches(63, [96, 5], 'bf16') == (64 * 2 + 16, 2 * 64 * 2 + 16) and G.pitches(539, [256, 3], 'fp32') == (576 * 4 + 16, 4 * 64 * 4 + 16)
    assert G.wgrad_jobs('in539') == 9 * 4 + 4 * 1 and G.wgrad_jobs('two_skips') == 1 * 1 + 2 * 4 + 4 * 1
