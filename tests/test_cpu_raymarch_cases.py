"""Conditions on the rays and references of tests/raymarch_cases.py, for every shape tests/test_gpu_raymarch_edges.py uses.

These are conditions on the CASES and on the REFERENCES, not measurements of a kernel: a case that breaks one is a badly
chosen case.  Three kinds:

  * the named rays are what their names say (an opaque sample's oracle weight is above 0.999, the empty and zero-density
    rays have all-zero weights, the repeated-depth ray has zero intervals, a zero-weight ray's fine samples all sit on the
    last midpoint, ...);
  * every tolerance of the GPU file leaves the reference alone a factor of at least two (MARGIN):
      (a) composite_kernel's evaluation order in NumPy float32 (raymarch_cases.composite_scan_emulation: 64-sample chunks,
          Hillis-Steele product, carry, butterfly sums), as it is and with every exp moved by +-1 ulp at random, against
          nerf_ref.accumulate in float32 (S = 1, which the oracle cannot take: the float64 torch formula);
      (b) the compositing formulas differentiated by torch in float32 against float64 autograd, under the backward
          tolerance, up to S = 4096;
  * sample_fine's two ranking rules (all pairs / two sorted lists) give the same permutation on every fine_cases ray, whose
    deterministic fine samples are non-decreasing — what the sorted-lists shortcut assumes.

Worst ratios error / tolerance measured on this catalogue, on the CPU (0.5 is the cap; printed by the tests, pytest -s):
  (a) rgb 0.43, occu 0.29, weights 0.29, depth 0.20, all four at S = 200 and the same with every exp moved by +-1 ulp
      (the order of the products sets them, not exp: on the repeated-depth ray the oracle multiplies 0.968 by 1 + 1e-6
      198 times in a row and rounds the same way every time, the scan multiplies powers of 1 + 1e-6, which are exact);
      at most 0.08 at every other shape;
  (b) backward: 0.009 up to S = 65, 0.04 up to S = 200, 0.11 at S = 257, 0.15 / 0.16 at S = 2048 / 2049, 0.36 at S = 4096.
The composited colour against FLOAT64 (the check that the backward's forward is the forward kernel's) has no such room on
every ray: raymarch_cases.forward_compared_rays leaves out the rays where float32 itself is more than half the tolerance
from float64 — none up to S = 129, two at S = 200, one at S = 257 — and says why; this file caps their number.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import raymarch_cases as C

MARGIN = 0.5
ids2 = lambda cases: ['n%d-S%d' % c for c in cases]
ids3 = lambda cases: ['n%d-nc%d-nf%d' % c for c in cases]


def _oracle_forward(n, s, white_bg, use_noise):
    """(rgb, occu, depth, weights): nerf_ref.accumulate in float32; for S = 1 the float64 torch formula."""
    rgbs, z, rayd, noise, _ = C.edge_rays(n, s)
    if s >= 2:
        rgb, occu, depth, _, w = nerf_ref.accumulate(rgbs, z, rayd, white_bg=white_bg, noise=noise if use_noise else None)
        return rgb, occu, depth, w
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    return tuple(v.numpy() for v in C.torch_composite_all(t(rgbs), t(z), t(rayd), white_bg, t(noise) if use_noise else None))


# ------------------------------------------------------------------------------------------------ the cases
def test_the_shape_lists_are_the_issue_s():
    assert [s for n, s in C.COMPOSITE_CASES if n == 13] == [1, 2, 7, 63, 64, 65, 128, 129, 200, 257]
    assert sorted(n for n, s in C.COMPOSITE_CASES if s == 65) == [1, 2, 3, 5, 13, 129]
    assert set(C.BWD_CASES) - set(C.COMPOSITE_CASES) == {(5, 2048), (5, 2049), (5, 4096)}
    assert len(C.FINE_SHAPES) == 11 and {(n, nc, nf) for n, nc, nf in C.FINE_CASES if n != 13} == {(n, 67, 65) for n in (1, 2, 3, 5)}
    lds = lambda nc, nf: 4 * (2 * (nc - 1) + nc + nf) * 4
    assert all(lds(nc, nf) <= 64 * 1024 for nc, nf in C.FINE_SHAPES)
    assert lds(258, 3400) > 64 * 1024                         # the shape the GPU file expects to be refused
    assert 4 * 2 * 2048 * 4 == 64 * 1024 < 4 * 2 * 2049 * 4   # composite_bwd: S = 2049 is the first large-LDS launch
    assert np.float32(1) / np.float32(1e-10) == np.float32(1e10)     # disp of an empty ray


@pytest.mark.parametrize("n,s", C.BWD_CASES, ids=ids2(C.BWD_CASES))
def test_edge_rays_are_what_their_names_say(n, s):
    rgbs, z, rayd, noise, g = C.edge_rays(n, s)
    assert rgbs.shape == (n, s, 4) and z.shape == noise.shape == (n, s) and rayd.shape == g.shape == (n, 3)
    assert all(a.dtype == np.float32 and not a.flags.writeable for a in (rgbs, z, rayd, noise, g))
    assert np.all(np.diff(z, axis=1) >= 0)
    rows = C.edge_rows(n, s)
    assert len(rows) <= n - min(n, C.N_RANDOM) and (n < 13 or len(rows) == (10 if s > 2 else 9))
    w = _oracle_forward(n, s, True, False)[3]
    for name in ('empty', 'zero', 'negzero'):
        if name in rows:
            assert np.all(w[rows[name]] == 0), name
    if 'negzero' in rows:
        assert np.all(np.signbit(rgbs[rows['negzero'], :, 3])) and not np.any(np.signbit(rgbs[rows['zero'], :, 3]))
    for name, k in (('opaque_first', 0), ('opaque_mid', s // 2), ('last_only', s - 1)):
        if name in rows:
            assert w[rows[name], k] > 0.999, (name, w[rows[name], k])
    if 'opaque_first' in rows:
        assert abs(float(w[rows['opaque_first'], 0]) - 1.) <= 1e-7
    if 'saturated' in rows:
        assert w[rows['saturated']].sum() > 0.999
    if 'repeated_z' in rows:
        d = np.diff(z[rows['repeated_z']])
        assert np.all(d[1:] == 0) and d[0] > 0
    if 'dir_small' in rows:
        norm = np.linalg.norm(rayd, axis=1)
        assert norm[rows['dir_small']] < 1e-2 and norm[rows['dir_large']] > 1e2
    # the plain random rays are neither empty nor opaque at once: the sums have many terms
    plain = w[len(rows):]
    if s >= 7:
        assert np.all((plain > 1e-4).sum(1) >= 2)


@pytest.mark.parametrize("n,nc,nf", C.FINE_CASES, ids=ids3(C.FINE_CASES))
def test_fine_cases_are_what_their_names_say_and_the_ranking_rules_agree(n, nc, nf):
    z, w = C.fine_cases(nc, nf, n=n)
    assert z.shape == w.shape == (n, nc) and z.dtype == w.dtype == np.float32
    assert np.all(np.diff(z, axis=1) >= 0) and np.all(w >= 0)
    rows = C.fine_rows(n)
    assert n < 13 or len(rows) == 8
    zf = C.fine_samples(z, w, nf)
    assert zf.shape == (n, nf)
    mid_last = np.float32(.5) * (z[:, -1] + z[:, -2])
    for name in ('all_zero', 'outer_first', 'outer_last'):
        if name in rows:
            assert np.all(zf[rows[name]] == mid_last[rows[name]]), name
    if 'one_inner' in rows:
        assert np.count_nonzero(w[rows['one_inner']]) == 1 and w[rows['one_inner'], 0] == 0 == w[rows['one_inner'], -1]
    if 'mostly_zero' in rows and nc >= 64:
        assert 0.5 < np.mean(w[rows['mostly_zero'], 1:-1] == 0) < 0.9
    if 'uniform' in rows:
        assert np.all(w[rows['uniform'], 1:-1] == 0.25)
    if 'repeated_z' in rows:
        assert np.all(z[rows['repeated_z'], nc // 2:] == z[rows['repeated_z'], nc // 2])
    # what the sorted-lists shortcut of the kernel assumes, and that it then ranks as the all-pairs rule does
    assert np.all(np.diff(zf, axis=1) >= 0)
    want = nerf_ref.gen_z_fine(z, w, nf)
    for r in range(n):
        zall = np.concatenate((z[r], zf[r]))
        general = C.rank_general(zall)
        assert np.array_equal(np.sort(general), np.arange(nc + nf))          # a permutation
        assert np.array_equal(general, C.rank_sorted_lists(z[r], zf[r])), r
        out = np.empty_like(zall)
        out[general] = zall
        assert np.array_equal(out, want[r])                                  # the scatter by rank IS the oracle's sort


def test_chosen_u_hits_the_cdf_entries():
    z, w, u, row = C.chosen_u_case()
    _, cdf = C.fine_pdf_cdf(w[row])
    assert cdf.size == 5 and np.all(np.diff(cdf) > 0) and cdf[-1] < 1
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1)) and u[row].min() == 0 and u[row].max() == np.nextafter(np.float32(1), np.float32(0))
    assert all(np.any(u[row] == c) for c in cdf[1:])
    zf = C.fine_samples(z, w, u.shape[1], u=u)
    mid = np.float32(.5) * (z[row, 1:] + z[row, :-1])
    for k in (1, 2, 3):         # u == cdf[k]: the oracle's `<=` puts the sample into bin k, at its lower edge
        hit = u[row] == cdf[k]
        assert np.all(zf[row, hit] == mid[k])
        below = u[row] == np.nextafter(cdf[k], np.float32(0))
        assert below.any() and np.all(zf[row, below] <= mid[k]) and np.all(zf[row, below] > mid[k - 1])   # (bin k - 1)


# ------------------------------------------------------------------------------------------------ room in the tolerances
@pytest.mark.parametrize("n,s", C.COMPOSITE_CASES, ids=ids2(C.COMPOSITE_CASES))
def test_forward_tolerances_leave_the_scan_order_room(n, s):
    rgbs, z, rayd, noise, _ = C.edge_rays(n, s)
    worst = {}
    for white_bg, use_noise in ((True, False), (False, True)):
        want = dict(zip(('rgb', 'occu', 'depth', 'weights'), _oracle_forward(n, s, white_bg, use_noise)))
        for tag, rng in (('as is', None), ('1 ulp', np.random.default_rng(s + n))):
            got = C.composite_scan_emulation(rgbs, z, rayd, noise if use_noise else None, white_bg, ulp_rng=rng)
            assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in got.values())
            for name, tol in (('rgb', C.TOL_FWD), ('occu', C.TOL_FWD), ('weights', C.TOL_FWD), ('depth', C.TOL_DEPTH)):
                ratio = float(np.abs(got[name].astype(np.float64) - want[name]).max()) / tol
                worst[tag, name] = max(worst.get((tag, name), 0.), ratio)
    print('n %d S %d: error / tolerance ' % (n, s) + ', '.join('%s %s %.3f' % (k + (v,)) for k, v in sorted(worst.items())))
    assert max(worst.values()) <= MARGIN, worst


@pytest.mark.parametrize("n,s", C.BWD_CASES, ids=ids2(C.BWD_CASES))
def test_backward_tolerance_leaves_float32_autograd_room(n, s):
    worst_b, left_out = 0., 0
    for white_bg, use_noise in C.BWD_COMBOS:
        want, rgb64 = C.backward_ref(n, s, white_bg, use_noise)
        got, rgb32 = C.backward_ref(n, s, white_bg, use_noise, 'float32')
        assert np.isfinite(want).all() and np.isfinite(got).all() and np.abs(want).max() > 0
        worst_b = max(worst_b, C.bwd_error_ratio(got, want))
        if (n, s) in C.COMPOSITE_CASES:       # the forward the backward recomputes is compared at these shapes only
            left_out = max(left_out, int((~C.forward_compared_rays(n, s, white_bg, use_noise)).sum()))
    print('n %d S %d: float32 autograd error / tolerance %.4f; composited colour against float64: %d rays left out' % (
        n, s, worst_b, left_out))
    assert worst_b <= MARGIN
    # the colour against float64: every ray up to S = 129; beyond, at most the three rays with a long empty run in front
    assert left_out <= (0 if s <= 129 else 3)


def test_backward_tolerance_sees_a_wrong_gradient():
    """The atol of the backward tolerance is relative to the largest gradient of the case: no single ray may set it so high
    that the others vanish under it (the last sample's interval of 1e10 could)."""
    for n, s in C.BWD_CASES:
        for white_bg, use_noise in C.BWD_COMBOS:
            want = C.backward_ref(n, s, white_bg, use_noise)[0]
            per_ray = np.abs(want).reshape(n, -1).max(1)
            assert per_ray.max() < 1e3, (n, s, per_ray.max())
            plain = per_ray[len(C.edge_rows(n, s)):]
            if s >= 7:          # (a one- or two-sample ray with negative densities has no gradient at all)
                assert np.all(plain > 100 * C.BWD_ATOL * per_ray.max()), (n, s, white_bg, use_noise, plain.min(), per_ray.max())
