"""Conditions on the inputs and restatements of tests/step_kernel_cases.py, for every shape tests/test_gpu_step_kernels.py uses.

These are conditions on the CASES and on the RESTATEMENTS, not measurements of a kernel.  Three kinds:

  * the shape lists are the ones the kernels branch on, every named row is where the lists say and is what its name says (the
    exact-eps row has sum x^2 == eps in float32, its neighbour lies below), and no input or restatement holds a NaN or an Inf;
  * every float32 restatement stays within HALF (MARGIN) of the tolerance the project already uses for that quantity, against a
    float64 evaluation of the plain formula (torch autograd in float64 for the gradients) — so that the GPU file's float64
    assertions hold by construction wherever its bit equalities do;
  * fma32, which sincos_cw rests on, is the correctly rounded fused multiply-add: against fractions.Fraction on random
    operands and on constructed halfway cases, where rounding the float64 sum a second time would go wrong.

Worst shares error / tolerance measured on this catalogue (0.5 is the cap; pytest -s prints them per case):
  pair_loss     loss 0.04; gradients 0.33 (a grid-blended A against a full-precision B whose difference nearly cancels).  Grid
                inputs wherever a term blends — see step_kernel_cases.py: with full-precision blended inputs float32 itself is
                1e-3 from float64 at rtol 1e-5, so those inputs were changed and not the tolerance
  l2_normalize  y 0.06, gradient 0.015 of the scaled tolerance
  light         loss 0.07, gradient 0.06
  amsgrad       p 0.009, vhat 0.03 — without the `underflow` element's vhat, a float32 denormal of 7 bits, named for it
  embed         modes 0 - 2 (against the float64 encoding of the float32 vector, as the existing test): 0.03 at 1 band ... 0.0003
                at 10 bands; mode 3 (against the float64 normalisation as well): 0.05 at 0 bands ... 0.21 at 10 bands;
                embed_bwd 0.001; sincos_cw alone: 0.9e-7 from sine and cosine up to |y| = 1536
The step size: nfx_amsgrad_step_size equals the restatement bit for bit, and lies at most STEP_SIZE_TF_ULP float32 steps from
TensorFlow's all-float32 evaluation (a documented, deliberate difference — it gates no kernel).
"""
import ctypes
from fractions import Fraction

import numpy as np

from tests import step_kernel_cases as C

MARGIN = 0.5
F = np.float32
WORST = {}


def _share(key, err, tol):
    share = float(np.max(np.asarray(err, dtype=np.float64) / np.asarray(tol, dtype=np.float64))) if np.size(err) else 0.
    WORST[key] = max(WORST.get(key, 0.), share)
    print('%-28s share %.4f' % (key, share))
    return share


def _finite(*arrays):
    return all(a is None or bool(np.isfinite(a).all()) for a in arrays)


# ------------------------------------------------------------------------------------------------ the lists
def test_the_shape_lists_are_the_issue_s():
    assert [d for n, d in C.LOSS_SHAPES if n == 13] == [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 512]
    assert [n for n, d in C.LOSS_SHAPES if n != 13] == [1, 2, 3, 4, 5] and all(d == 65 for n, d in C.LOSS_SHAPES if n != 13)
    assert len(C.EIGHT_D) == len(C.EIGHT_W) == 8 and min(C.EIGHT_W) < 0 and 0. in C.EIGHT_W
    assert [d for n, d in C.NORM_SHAPES if n == 13] == list(range(1, 17))
    assert [n for n, d in C.NORM_SHAPES if n != 13] == [1, 255, 256, 257, 513]
    assert F(2. ** -10) * F(2. ** -10) == F(C.NORM_EPS[1]) and C.NORM_EPS[0] == 1e-6
    assert (5, 17) in C.LIGHT_SHAPES and 5 * 17 * 3 == 255 and (2, 43) in C.LIGHT_SHAPES and 2 * 43 * 3 == 258
    assert len(C.LIGHT_SHAPES) == 11 and max(h * w * 3 for h, w in C.LIGHT_SHAPES) == 17 * 33 * 3
    assert C.ADAM_N == (1, 255, 256, 257, 1000) and C.ADAM_STEPS == 6
    assert {c[0] for c in C.EMBED_CASES} == {0, 1, 2, 3} and {c[1] for c in C.EMBED_CASES} == {0, 1, 2, 4, 10}
    assert {c[3] for c in C.EMBED_CASES} == {1, 4, 5, 13} and {c[4] for c in C.EMBED_CASES} == {1, 7}
    assert {c[5] for c in C.EMBED_CASES} == {0, 13} and not any(c[1] == 0 and not c[2] for c in C.EMBED_CASES)
    assert max(c[3] * c[4] * ((3 if c[2] else 0) + 6 * c[1]) for c in C.EMBED_CASES) > 256      # more than one block


# ------------------------------------------------------------------------------------------------ fma32
def _fma_exact(a, b, c):
    """The float32 nearest (ties to even) to a*b + c, by rational arithmetic."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = F(float(exact))             # (float() of a Fraction rounds correctly; this second rounding may be wrong by one step)
    cands = sorted({near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(-np.inf))}, key=float)
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(C.bits(v).reshape(())) & 1))
    return best


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(0)
    a = rng.normal(size=4000).astype(F)
    b = rng.normal(size=4000).astype(F)
    c = (rng.normal(size=4000) * 10. ** rng.integers(-8, 3, size=4000)).astype(F)
    c[:1000] = -(a[:1000] * b[:1000])              # cancellation: the result is the product's rounding error
    # halfway cases: p = a*b exact with few bits, c = half a float32 step of p plus or minus a term below float64's reach of the sum
    ha = (1. + rng.integers(1, 2 ** 11, size=2000) * 2. ** -11).astype(F)
    hb = (1. + rng.integers(1, 2 ** 11, size=2000) * 2. ** -11).astype(F)
    hp = ha.astype(np.float64) * hb.astype(np.float64)              # in [1, 4), 22 bits behind the point
    half = np.where(hp < 2., 2. ** -24, 2. ** -23)
    mid = np.floor(hp / (2 * half)) * (2 * half) + half             # a float32 halfway point next to p
    hc1 = (mid - hp).astype(F)                                      # exact: p + c is the halfway point (ties to even)
    a = np.concatenate([a, ha, ha])
    b = np.concatenate([b, hb, hb])
    c = np.concatenate([c, hc1, hc1])
    got = C.fma32(a, b, c)
    want = np.array([_fma_exact(*v) for v in zip(a, b, c)], dtype=F)
    assert C.same_bits(got, want), np.argwhere(C.bits(got) != C.bits(want))[:4].tolist()
    # c so large that the low bits of the product fall below float64's sum: the two-sum error term is not zero
    b2 = (hb.astype(np.float64) * (1 + 2. ** -23)).astype(F)
    for big in (F(2. ** 30), F(-2. ** 31), F(3. * 2. ** 29)):
        got2 = C.fma32(ha, b2, np.full_like(ha, big))
        want2 = np.array([_fma_exact(x, y, big) for x, y in zip(ha, b2)], dtype=F)
        assert C.same_bits(got2, want2)
    # a constructed double-rounding trap: s = p + c falls within 2^-53 relative of a float32 halfway point
    x, y = F(1. + 2. ** -12), F(1. + 2. ** -12)                     # p = 1 + 2^-11 + 2^-24: exactly halfway between two float32
    for cc, step in ((F(2. ** -60), 1), (F(-2. ** -60), 0), (F(0.), 0)):
        want3 = F(1. + 2. ** -11) if step == 0 else np.nextafter(F(1. + 2. ** -11), F(2))
        assert C.fma32(x, y, cc) == want3 == _fma_exact(x, y, cc), (cc, C.fma32(x, y, cc), want3)
    assert F(np.float64(x) * np.float64(y) + np.float64(F(2. ** -60))) != np.nextafter(F(1. + 2. ** -11), F(2))   # the naive way fails it


def test_sincos_cw_restatement_is_sine_and_cosine():
    y = np.random.default_rng(1).uniform(-1536., 1536., size=20000).astype(F)
    sn, cs = C.sincos_cw(y)
    err = np.maximum(np.abs(sn - np.sin(y.astype(np.float64))), np.abs(cs - np.cos(y.astype(np.float64))))
    assert _share('sincos_cw |y| < 1536', err.max(), 2.5e-7) <= 1.


# ------------------------------------------------------------------------------------------------ pair_loss
def loss_cases():
    for n, d in C.LOSS_SHAPES:
        for kind in ('mse', 'mae'):
            for ba, bb in ((True, True), (True, False), (False, False)):
                for bg in C.LOSS_BG:
                    yield 'one-n%d-D%d-%s-%d%d-bg%d' % (n, d, kind, ba, bb, bg), C.loss_one_term(n, d, kind, ba, bb, bg)
    for name in C.LOSS_SETS:
        for bg in C.LOSS_BG:
            yield '%s-bg%d' % (name, bg), C.loss_term_set(name, bg)


def _full_plan(case):
    """A plan with a buffer on every side (the null-pointer cases leave a tensor's second contribution out on purpose: the
    float64 comparison needs the whole gradient)."""
    return C.loss_plan(case['spec'], len(case['tensors']))


def test_pair_loss_restatement_against_float64():
    for key, case in loss_cases():
        assert _finite(case['alpha'], case['up'], *case['tensors']), key
        want, want_g = C.pair_loss_float64(case)
        got = C.pair_loss_fwd(case['tensors'], case['spec'], case['alpha'], case['bg'])
        assert got.dtype == F and _finite(got)
        _share('pair_loss loss', np.abs(got - want), C.LOSS_ATOL + C.LOSS_RTOL * np.abs(want))
        init = {i: np.full(case['tensors'][i].shape, np.nan, F) for i in want_g}
        got_g = C.pair_loss_bwd(case['tensors'], case['spec'], _full_plan(case), case['alpha'], case['bg'], case['up'], init)
        for i, g in got_g.items():
            assert g.dtype == F and _finite(g), (key, i)
            _share('pair_loss grad', np.abs(g - want_g[i]), C.LOSS_G_ATOL + C.LOSS_G_RTOL * np.abs(want_g[i]))
    assert WORST['pair_loss loss'] <= MARGIN and WORST['pair_loss grad'] <= MARGIN, WORST


def test_pair_loss_cases_are_what_they_say():
    one = C.loss_one_term(13, 65, 'mae', True, True, 1.)
    assert one['alpha'][0] == 0 and one['alpha'][1] == 1 and 0 < one['alpha'][2:].min() and one['alpha'][2:].max() < 1
    assert one['up'][3] < 0 and not any(a.flags.writeable for a in one['tensors'])
    assert np.all(one['tensors'][0][2:5, :7] == one['tensors'][1][2:5, :7])           # the ties
    sets = {name: C.loss_term_set(name) for name in C.LOSS_SETS}
    assert len(sets['eight']['spec']) == 8 and {t[3] for t in sets['eight']['spec']} == {'mse', 'mae'}
    assert sets['a_twice']['plan'] == [(0, 1, False, False), (0, 2, True, False)]
    assert sets['b_twice']['plan'] == [(1, 0, False, False), (2, 0, False, True)]
    assert sets['a_then_b']['plan'] == [(0, 1, False, False), (2, 0, False, True)]
    assert sets['no_alpha']['alpha'] is None and all(t[4] for t in sets['no_alpha']['spec'])
    assert sets['null_ga']['plan'][1] == (None, 2, False, False) and sets['null_gb']['plan'][1] == (2, None, False, False)
    # a term's blended operands lie on the grid: the blend is exact in float32
    al = one['alpha'].astype(np.float64)[:, None]
    x = one['tensors'][0]
    assert np.array_equal(C.blend(x, one['alpha'][:, None], 1.).astype(np.float64), x * al + (1. - al))


# ------------------------------------------------------------------------------------------------ l2_normalize_rows
def test_l2_normalize_rows_restatement_against_float64():
    for n, d in C.NORM_SHAPES:
        for eps in C.NORM_EPS:
            x, dy = C.norm_case(n, d, eps)
            assert _finite(x, dy)
            yr, gr, scale = C.l2_normalize_float64(x, dy, eps)
            y, g = C.l2_normalize_rows(x, eps), C.l2_normalize_rows_bwd(x, dy, eps)
            assert y.dtype == g.dtype == F and _finite(y, g)
            _share('l2_normalize y', np.abs(y - yr), C.NORM_TOL_Y)
            _share('l2_normalize grad', np.abs(g - gr) / scale, C.NORM_TOL_G)
    assert WORST['l2_normalize y'] <= MARGIN and WORST['l2_normalize grad'] <= MARGIN, WORST


def test_l2_normalize_named_rows():
    for eps in C.NORM_EPS:
        for n, d in C.NORM_SHAPES:
            x, dy = C.norm_case(n, d, eps)
            rows = C.norm_rows(n)
            assert (len(rows) == 7) == (n >= 10) and (rows or n == 1)
            if not rows:
                continue
            sq = C._row_sum(x * x)
            assert not np.any(x[rows['zero']]) and not np.signbit(x[rows['zero']]).any()
            assert not np.any(x[rows['negzero']]) and np.signbit(x[rows['negzero']]).all()
            assert sq[rows['below_eps']] < F(eps) and 0 < sq[rows['in_clamp']] < F(eps)
            assert sq[rows['large']] > 1e3 or d == 1 and sq[rows['large']] > 1.
            assert sq[rows['one_hot']] == 1 and np.count_nonzero(x[rows['one_hot']]) == 1
            if eps == C.NORM_EPS[1]:
                assert sq[rows['exact_eps']] == F(eps) == F(2. ** -20)          # sq >= eps decides; sq > eps would cut the gradient
                assert sq[rows['below_eps']] == np.nextafter(np.nextafter(F(eps), F(0)), F(0))
                g = C.l2_normalize_rows_bwd(x, dy, eps)
                r, k = rows['exact_eps'], rows['exact_eps'] % d
                assert g[r, k] == 0 and (d == 1 or np.all(np.delete(g[r], k) != 0))     # the norm takes the radial part away ...
                rb = rows['below_eps']
                assert g[rb, rb % d] != 0                                                # ... and below eps it does not


# ------------------------------------------------------------------------------------------------ light_smoothness
def test_light_smoothness_restatement_against_float64():
    for h, w in C.LIGHT_SHAPES:
        light = C.light_case(h, w)
        assert light.shape == (h, w, 3) and _finite(light) and not light.flags.writeable
        for tv, achro in C.LIGHT_WEIGHTS:
            ref, gr = C.light_float64(light, tv, achro)
            loss, grad = C.light_smoothness(light, tv, achro)
            assert loss.dtype == grad.dtype == F and _finite(loss, grad)
            _share('light loss', abs(float(loss) - ref), C.LIGHT_TOL * abs(ref) + 1e-12)
            _share('light grad', np.abs(grad - gr).max(), C.LIGHT_TOL * np.abs(gr).max() + 1e-12)
    assert WORST['light loss'] <= MARGIN and WORST['light grad'] <= MARGIN, WORST
    loss, grad = C.light_smoothness(C.light_case(1, 1), 0.25, 0.)
    assert loss == 0 and not grad.any()                   # every spatial neighbour of the only texel is the texel


# ------------------------------------------------------------------------------------------------ amsgrad
def test_amsgrad_restatement_against_float64_and_named_elements():
    for n in C.ADAM_N:
        p0, gs = C.adam_case(n)
        rows = C.adam_rows(n)
        assert (len(rows) == 5) == (n >= 255) and _finite(p0, gs)
        p, m, v, vh = p0.copy(), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        ref = C.amsgrad_float64(p0, gs)
        for step in range(1, C.ADAM_STEPS + 1):
            g = gs[step - 1]
            lr_t = C.amsgrad_step_size(C.ADAM_LR, C.ADAM_B1, C.ADAM_B2, step)
            p, m, v, vh = C.amsgrad(p, g, m, v, vh, lr_t)
            assert all(a.dtype == F for a in (p, m, v, vh)) and _finite(p, m, v, vh)
            p64, vh64 = ref[step - 1]
            keep = np.ones(n, bool)
            if rows:
                keep[rows['underflow']] = False           # vhat there is a float32 denormal (the element is named for it)
            _share('amsgrad p', np.abs(p - p64), C.ADAM_P_ATOL + C.ADAM_P_RTOL * np.abs(p64))
            _share('amsgrad vhat', np.abs(vh - vh64)[keep], (C.ADAM_VH_RTOL * np.abs(vh64))[keep] + 1e-300)
            if rows and step >= 2:
                assert vh[rows['spike']] > v[rows['spike']] and vh[rows['alternating']] == v[rows['alternating']]
        if rows:
            assert p[rows['zero_grad']] == p0[rows['zero_grad']] and m[rows['zero_grad']] == 0
            assert 0 < vh[rows['underflow']] < np.finfo(F).tiny and p[rows['underflow']] != p0[rows['underflow']] or \
                abs(p0[rows['underflow']]) > 1e-3
            assert vh[rows['huge']] > 1e30
    assert WORST['amsgrad p'] <= MARGIN and WORST['amsgrad vhat'] <= MARGIN, WORST


def test_step_size_is_the_library_s_bit_for_bit(nfx_lib):
    fn = nfx_lib.lib.nfx_amsgrad_step_size
    for lr in C.STEP_SIZE_LR:
        for step in C.STEP_SIZE_STEPS:
            got = F(fn(lr, C.ADAM_B1, C.ADAM_B2, step))
            want = C.amsgrad_step_size(lr, C.ADAM_B1, C.ADAM_B2, step)
            assert C.same_bits(got, want), (lr, step, got, want)
    assert isinstance(fn.restype(), ctypes.c_float)


def test_step_size_distance_from_tensorflow():
    worst = 0
    for lr in C.STEP_SIZE_LR:
        for step in C.STEP_SIZE_STEPS:
            ours, tf = C.amsgrad_step_size(lr, C.ADAM_B1, C.ADAM_B2, step), C.tf_step_size(lr, C.ADAM_B1, C.ADAM_B2, step)
            assert tf.dtype == F
            dist = C.ulp_distance(ours, tf)
            print('lr %g step %7d: library %.9g, all-float32 %.9g, %d ulp' % (lr, step, ours, tf, dist))
            worst = max(worst, dist)
    assert worst <= 2 * C.STEP_SIZE_TF_ULP, worst
    assert worst >= C.STEP_SIZE_TF_ULP // 2, worst           # (the constant is a measurement, not a guess from above)


# ------------------------------------------------------------------------------------------------ embed
def test_embed_restatement_against_float64():
    for mode, L, incl, n_src, per, col0 in C.EMBED_CASES:
        x, dirs, z = C.embed_inputs(mode, n_src, per)
        assert _finite(x, dirs, z)
        got = C.embed(mode, L, incl, x, dirs, z, per)
        assert got.dtype == F and got.shape == (n_src * per, (3 if incl else 0) + 6 * L) and _finite(got)
        want = C.embed_float64(mode, L, incl, x, dirs, z, per)
        _share('embed mode %d, %2d bands' % (mode, L), np.abs(got - want).max(), C.embed_tol(L))
        if mode == 3 and n_src >= 4:                      # light 0 sits on point 2: the zero vector, sin 0 = 0, cos 0 = 1
            row = got[2 * per]
            assert np.array_equal(row, C.embed_of(np.zeros((1, 3), F), L, incl)[0]) and not np.any(C.embed_vectors(3, x, dirs, z, per)[2 * per])
    assert max(v for k, v in WORST.items() if k.startswith('embed mode')) <= MARGIN, WORST


def test_embed_bwd_restatement_against_float64():
    for L, incl, n, col0 in C.EMBED_BWD_CASES:
        v, d_out = C.embed_bwd_case(L, incl, n, col0)
        got = C.embed_bwd(v, L, incl, d_out, col0)
        assert got.dtype == F and got.shape == (n, 3) and _finite(got, v, d_out)
        want = C.embed_bwd_float64(v, L, incl, d_out, col0)
        _share('embed_bwd', np.abs(got - want).max(), C.EMBED_BWD_TOL * np.abs(want).max())
    assert WORST['embed_bwd'] <= MARGIN, WORST
