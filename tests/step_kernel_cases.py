"""Inputs, shape lists and float32 NumPy restatements of the small kernels of a training step: pair_loss_kernel (csrc/loss.hip),
l2_normalize_rows_kernel and light_smoothness_kernel (csrc/regularizers.hip), amsgrad_kernel / amsgrad_dev_kernel (csrc/train.hip)
and embed_kernel / embed_bwd_kernel (csrc/mlp_generic.hip).  No GPU: tests/test_cpu_step_kernel_cases.py checks the cases and the
room every tolerance leaves, tests/test_gpu_step_kernels.py holds the kernels to the restatements BIT FOR BIT.

Why one right answer exists: the library is compiled with -ffp-contract=off and correctly rounded `/` and sqrtf (none of the
five files is in build.py's FAST_DIV list), float32 denormals are kept, and none of these kernels uses an atomic or a reduction
whose order depends on the launch.  So every restatement below keeps every intermediate in np.float32 and follows the kernel's
operation order, written from the kernels' comments, include/nfx.h and the reference's formulas:

  pair_loss          blend = x*al + bg*(1 - al); lane l of the ray's wave adds elements l, l + 64, ... in order, the 64 lane sums
                     meet in an xor butterfly over offsets 32, 16, 8, 4, 2, 1 (all lanes end equal: asserted), then
                     total += w*(s/float(D)) in term order.  Backward: c = (up*w)/float(D), g = c*(2*diff) or c*sign(diff) with
                     sign(0) = 0, A gets g or g*al, B gets -g or (-g)*al, written or added in term order.
  l2_normalize_rows  sq = the sequential sum of v[k]*v[k], inv = 1/sqrt(max(sq, eps)), y = v*inv; pull-back
                     c = ((dot*inv)*inv)*inv where sq >= eps (0 elsewhere), dx = g*inv - v*c.
  light_smoothness   thread t sums tv*(dx*dx + dy*dy) + achro*(dc*dc) over elements t, t + 256, ...; the tree adds
                     part[t] += part[t + k] for k = 128 ... 1; the gradient as the kernel writes it.
  amsgrad            the five lines of the kernel; the step size is float32 of the double formula with the betas (and lr) first
                     rounded to float32.
  embed / embed_bwd  the four input modes, the mode-3 normalisation, and sincos_cw, whose fmaf needs an exact float32 fma: fma32
                     below (float64 product of two float32 is exact; the float64 sum may round once more, which the two-sum error
                     term repairs at the float32 halfway points).

Inputs.  A tensor that a loss term blends, and every alpha, lies on a grid (k/256, k/64): x*al + bg*(1 - al) is then exact in
float32 and the float64 comparison of the gradients keeps its meaning (a blended difference of full-precision values cancels
AFTER rounding, which puts float32 itself 1e-3 from float64 at rtol 1e-5).  `grid=False` gives the same cases with full-
precision values for the bit-equality tests, where cancellation is no concern.
"""
import functools
import math

import numpy as np

F = np.float32

# ------------------------------------------------------------------------------------------------ the shape lists
LOSS_D = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 512)
LOSS_N_ALL, LOSS_D_ALL = 13, 65
LOSS_N = (1, 2, 3, 4, 5)
LOSS_SHAPES = tuple((LOSS_N_ALL, d) for d in LOSS_D) + tuple((n, LOSS_D_ALL) for n in LOSS_N)
LOSS_BG = (0., 1.)
LOSS_SETS = ('eight', 'a_twice', 'b_twice', 'a_then_b', 'no_alpha', 'null_ga', 'null_gb')
EIGHT_D = (1, 3, 64, 65, 129, 512, 2, 200)
EIGHT_W = (1., 0.1, -0.01, 0.05, 0., 0.3, 0.01, 0.7)        # one negative, one zero

NORM_D = tuple(range(1, 17))
NORM_N_ALL, NORM_D_ALL = 13, 3
NORM_N = (1, 255, 256, 257, 513)
NORM_SHAPES = tuple((NORM_N_ALL, d) for d in NORM_D) + tuple((n, NORM_D_ALL) for n in NORM_N)
NORM_EPS = (1e-6, 2. ** -20)                                  # the shipped epsilon; one that a float32 row can hit exactly
NORM_NAMES = ('zero', 'negzero', 'exact_eps', 'below_eps', 'in_clamp', 'large', 'one_hot')

LIGHT_SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (3, 5), (5, 17), (2, 43), (16, 32), (17, 33))
LIGHT_WEIGHTS = ((0.25, 0.), (0., 0.5), (5e-6, 1e-3))         # (tv, 0), (0, achro), the pair of the existing probe test

ADAM_N = (1, 255, 256, 257, 1000)
ADAM_STEPS = 6
ADAM_NAMES = ('zero_grad', 'spike', 'alternating', 'underflow', 'huge')
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 5e-3, 0.9, 0.999, 1e-7
STEP_SIZE_STEPS = (1, 2, 3, 5, 10, 100, 10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6)
STEP_SIZE_LR = (5e-3, 5e-4)
# The library evaluates lr_t in double from the float32 lr and betas and rounds once; TensorFlow 2.2 evaluates pow, 1 - x, sqrt
# and the quotient in float32.  Distance between the two in float32 steps, measured on the CPU by tests/
# test_cpu_step_kernel_cases.py::test_step_size_distance_from_tensorflow (pytest -s prints every figure):
#   step          1   2   3   5  10  100  >= 1000
#   lr = 5e-3     0  34  26  35   3    1        0
#   lr = 5e-4     0  54  42  29   3    1        0
# (1 - b2^t is the float32 difference of two nearby numbers while t is small.)  Worst: 54.  A deliberate, documented
# difference that gates no kernel; the test asserts it with a factor of two.
STEP_SIZE_TF_ULP = 54

EMBED_FREQS = (0, 1, 2, 4, 10)
EMBED_SRC = (1, 4, 5, 13)
EMBED_PER = (1, 7)
EMBED_COL0 = (0, 13)
EMBED_PAD = 5                                                 # columns of the wider matrix behind the encoding


def _embed_cases():
    cases = []
    for mode in range(4):
        for L in EMBED_FREQS:                                   # every band count, with and without the input, in a wider matrix
            for incl in ((True, False) if L else (True,)):
                cases.append((mode, L, incl, 13, 7, 13))
        for n_src in (1, 4, 5):                                 # the small row counts, one and seven rows per vector
            for per in EMBED_PER:
                cases.append((mode, 4, True, n_src, per, 0))
        cases.append((mode, 10, True, 13, 1, 0))
    return tuple(cases)


EMBED_CASES = _embed_cases()                                    # (mode, n_freqs, incl_input, n_src, per_ray, col0)
EMBED_BWD_CASES = tuple((L, incl, n, col0) for L in EMBED_FREQS for incl in ((True, False) if L else (True,))
                        for n, col0 in ((13, 13), (5, 0))) + tuple((4, True, n, 0) for n in (1, 4))

# the tolerances against float64, each the figure of a test the project already has
LOSS_RTOL, LOSS_ATOL = 2e-6, 1e-7          # tests/test_gpu_train.py::test_fused_pair_loss_vs_torch, the loss
LOSS_G_RTOL, LOSS_G_ATOL = 1e-5, 1e-9      # the same test, the gradients
NORM_TOL_Y, NORM_TOL_G = 2e-6, 2e-5        # tests/test_gpu_regularizers.py::test_l2_normalize_rows_and_gradient (g: of the scale)
LIGHT_TOL = 2e-6                           # ::test_light_smoothness_and_gradient, relative
ADAM_P_RTOL, ADAM_P_ATOL, ADAM_VH_RTOL = 2e-5, 2e-6, 1e-5     # tests/test_gpu_train.py::test_amsgrad_matches_keras_semantics
EMBED_BWD_TOL = 1e-4                       # x max |want|: tests/test_gpu_generic.py::test_embed_backward_and_input_gradient_only_mode


def embed_tol(n_freqs):                    # tests/test_gpu_generic.py::test_embed_kernel_is_the_embedder
    return 4e-6 * max(1, 2 ** n_freqs) / 16 + 2e-6


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def same_bits(a, b):
    """float32 arrays equal bit for bit (-0 is not +0)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ulp_distance(a, b):
    """|a - b| in float32 steps, for finite values of one sign."""
    return int(abs(int(bits(F(a)).reshape(())) - int(bits(F(b)).reshape(()))))


# ================================================================================================ an exact float32 fma
def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: a*b + c rounded ONCE to float32.  The float64 product of two float32 is exact (48
    bits); the float64 sum s = p + c is rounded, by an error e that two-sum recovers exactly.  Rounding s to float32 is then
    wrong only where s sits exactly halfway between two float32 values and e != 0: there the sign of e decides."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        r = s.astype(F)
        up, dn = np.nextafter(r, F(np.inf)), np.nextafter(r, F(-np.inf))
        r64 = r.astype(np.float64)
        tie_up = (s - r64 == (up.astype(np.float64) - r64) * 0.5) & (e > 0)        # s above r by half a step, truth above s
        tie_dn = (s - r64 == (dn.astype(np.float64) - r64) * 0.5) & (e < 0)
        ok = np.isfinite(s) & np.isfinite(r)
    return np.where(ok & tie_up, up, np.where(ok & tie_dn, dn, r)).astype(F)


_SC = [F(v) for v in (0.6366197466850281, -1.5707963705062866, 4.371138828673793e-08,
                      -1.9515295891e-4, 8.3321608736e-3, -1.6666654611e-1,
                      2.443315711809948e-5, -1.388731625493765e-3, 4.166664568298827e-2)]


def sincos_cw(y, cos_sign_bit=None):
    """(sin y, cos y) as csrc/nfx_common.hpp:sincos_cw computes them: two-constant Cody-Waite reduction by fmaf, the Cephes
    polynomials by fmaf, the quadrant from (int)rintf(y 2/pi)."""
    y = np.asarray(y, dtype=F)
    two_over_pi, hi, lo, s1, s2, s3, c1, c2, c3 = _SC
    n = np.rint(y * two_over_pi).astype(F)
    r = fma32(n, hi, y)
    r = fma32(n, lo, r)
    q = n.astype(np.int32)
    r2 = r * r
    ps = fma32(r2, s1, s2)
    ps = fma32(ps, r2, s3)
    ps = fma32(ps * r2, r, r)
    pc = fma32(r2, c1, c2)
    pc = fma32(pc, r2, c3)
    pc = fma32(pc * r2, r2, fma32(r2, F(-0.5), F(1.0)))
    odd = (q & 1) != 0
    s0, c0 = np.where(odd, pc, ps), np.where(odd, ps, pc)
    return np.where((q & 2) != 0, -s0, s0).astype(F), np.where(((q + 1) & 2) != 0, -c0, c0).astype(F)


# ================================================================================================ pair_loss
def blend(x, al, bg):
    return x * al + F(bg) * (F(1.0) - al)


def _operands(tensors, term, al, bg):
    ia, ib, w, kind, ba, bb = term
    a, b = tensors[ia], tensors[ib]
    assert a.dtype == b.dtype == F and a.shape == b.shape
    x = blend(a, al[:, None], bg) if ba else a
    y = blend(b, al[:, None], bg) if bb else b
    return x - y


def _alpha_or_one(alpha, n):
    return np.ones(n, F) if alpha is None else np.asarray(alpha, dtype=F).reshape(n)


def pair_loss_fwd(tensors, spec, alpha, bg):
    """loss[n] of pair_loss_kernel<false>."""
    n = tensors[spec[0][0]].shape[0]
    al = _alpha_or_one(alpha, n)
    total = np.zeros(n, F)
    lanes = np.arange(64)
    for term in spec:
        diff = _operands(tensors, term, al, bg)
        d = diff.shape[1]
        e = np.abs(diff) if term[3] == 'mae' else diff * diff
        s = np.zeros((n, 64), F)
        for j in range(0, d, 64):                      # lane l adds elements l, l + 64, ... in order
            chunk = e[:, j:j + 64]
            s[:, :chunk.shape[1]] = s[:, :chunk.shape[1]] + chunk
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        assert np.array_equal(bits(s), bits(np.repeat(s[:, :1], 64, 1))), 'the butterfly leaves the lanes unequal'
        total = total + F(term[2]) * (s[:, 0] / F(d))
    return total


def loss_plan(spec, n_tensors, need=None, null=()):
    """Per term (index of the buffer for dA or None, for dB or None, accumulate A, accumulate B): the first term that holds a
    tensor writes its gradient, later ones add (what autograd.PairLoss does).  need[i] = False: tensor i gets no buffer;
    null = ((term, 'a' | 'b'), ...): that side of that term gets a null pointer although the tensor has a buffer."""
    need = [True] * n_tensors if need is None else need
    written = [False] * n_tensors
    plan = []
    for ti, (ia, ib, *_) in enumerate(spec):
        ga = ia if need[ia] and (ti, 'a') not in null else None
        gb = ib if need[ib] and (ti, 'b') not in null else None
        plan.append((ga, gb, ga is not None and written[ia], gb is not None and written[ib]))
        written[ia] = written[ia] or ga is not None
        written[ib] = written[ib] or gb is not None
    return plan


def pair_loss_bwd(tensors, spec, plan, alpha, bg, up, init):
    """The gradient buffers {tensor index: array} after pair_loss_kernel<true>, from their contents `init` before it."""
    n = tensors[spec[0][0]].shape[0]
    al = _alpha_or_one(alpha, n)
    up = np.asarray(up, dtype=F).reshape(n)
    bufs = {i: np.array(b, dtype=F) for i, b in init.items()}
    for term, (ga, gb, acc_a, acc_b) in zip(spec, plan):
        _, _, w, kind, ba, bb = term
        diff = _operands(tensors, term, al, bg)
        c = ((up * F(w)) / F(diff.shape[1]))[:, None]
        sign = (diff > 0).astype(F) - (diff < 0).astype(F)
        g = c * (sign if kind == 'mae' else F(2.0) * diff)
        if ga is not None:
            v = g * al[:, None] if ba else g
            bufs[ga] = bufs[ga] + v if acc_a else v.copy()
        if gb is not None:
            v = (-g) * al[:, None] if bb else -g
            bufs[gb] = bufs[gb] + v if acc_b else v.copy()
    return bufs


def _loss_inputs(rng, n, dims, blended, grid):
    """tensors of the given widths; the blended ones on the grid k/256 when `grid`."""
    out = []
    for d, bl in zip(dims, blended):
        if grid and bl:
            out.append((rng.integers(0, 256, size=(n, d)) / 256.).astype(F))
        else:
            out.append(rng.uniform(size=(n, d)).astype(F))
    return out


def _alpha_up(rng, n, grid):
    alpha = (rng.integers(1, 64, size=n) / 64.).astype(F) if grid else rng.uniform(size=n).astype(F)
    up = rng.uniform(size=n).astype(F)
    if n >= 4:                      # rows 0 and 1: a background and an opaque ray; row 3 pulls back a negative gradient
        alpha[0], alpha[1] = 0., 1.
        up[3] = -up[3]
    return alpha, up


def _ties(tensors, spec):
    """MAE terms (and the MSE ones, harmlessly): B = A in the first columns of rows 2 .. 4, so that diff == 0 exactly when
    both sides are blended alike."""
    for ia, ib, *_ in spec:
        a, b = tensors[ia], tensors[ib]
        b[2:5, :min(7, (b.shape[1] + 1) // 2)] = a[2:5, :min(7, (a.shape[1] + 1) // 2)]


@functools.lru_cache(maxsize=None)
def loss_one_term(n, d, kind, blend_a, blend_b, bg, grid=True):
    """One term between two tensors: dict(tensors, spec, plan, alpha, bg, up)."""
    rng = np.random.default_rng([n, d, int(kind == 'mae'), int(blend_a), int(blend_b), int(bg), int(grid)])
    tensors = _loss_inputs(rng, n, (d, d), (blend_a, blend_b), grid)
    spec = ((0, 1, 0.05, kind, blend_a, blend_b),)
    _ties(tensors, spec)
    alpha, up = _alpha_up(rng, n, grid)
    _frozen(alpha, up, *tensors)
    return dict(tensors=tensors, spec=spec, plan=loss_plan(spec, 2), alpha=alpha, bg=bg, up=up)


@functools.lru_cache(maxsize=None)
def loss_term_set(name, bg=1., grid=True):
    """The named term sets of LOSS_SETS at n = 13."""
    n, d = LOSS_N_ALL, LOSS_D_ALL
    rng = np.random.default_rng([LOSS_SETS.index(name), int(bg), int(grid)])
    null = ()
    if name == 'eight':            # eight terms of mixed width and kind over sixteen tensors
        dims = [w for w in EIGHT_D for _ in (0, 1)]
        spec = tuple((2 * t, 2 * t + 1, EIGHT_W[t], 'mae' if t % 2 else 'mse', t % 3 != 2, t % 3 == 0) for t in range(8))
    elif name == 'a_twice':        # tensor 0 is A of both terms: the second adds into its gradient (ACCUM_A)
        dims, spec = [d] * 3, ((0, 1, 1., 'mse', True, True), (0, 2, 0.05, 'mae', True, False))
    elif name == 'b_twice':        # ... B of both terms (ACCUM_B)
        dims, spec = [d] * 3, ((1, 0, 1., 'mse', True, True), (2, 0, 0.05, 'mae', False, True))
    elif name == 'a_then_b':       # A of the first, B of the second
        dims, spec = [d] * 3, ((0, 1, 0.1, 'mae', True, True), (2, 0, 0.5, 'mse', False, False))
    elif name == 'no_alpha':       # blend flags without an alpha: alpha = 1
        dims, spec = [d] * 3, ((0, 1, 1., 'mse', True, True), (0, 2, 0.05, 'mae', True, False))
    elif name in ('null_ga', 'null_gb'):   # tensor 0 has a buffer, which the second term must leave alone
        dims = [d] * 3
        spec = ((0, 1, 1., 'mse', True, True), (0, 2, 0.3, 'mae', False, False)) if name == 'null_ga' else \
            ((1, 0, 1., 'mse', True, True), (2, 0, 0.3, 'mae', False, False))
        null = ((1, 'a' if name == 'null_ga' else 'b'),)
    else:
        raise KeyError(name)
    blended = [any((ia == i and ba) or (ib == i and bb) for ia, ib, _, _, ba, bb in spec) for i in range(len(dims))]
    tensors = _loss_inputs(rng, n, dims, blended, grid)
    _ties(tensors, spec)
    alpha, up = _alpha_up(rng, n, grid)
    if name == 'no_alpha':
        alpha = None
    _frozen(alpha, up, *tensors)
    return dict(tensors=tensors, spec=spec, plan=loss_plan(spec, len(dims), null=null), alpha=alpha, bg=bg, up=up)


def loss_nan_init(case):
    """NaN-filled gradient buffers for every tensor of the case that the plan gives one."""
    idx = {i for ga, gb, _, _ in case['plan'] for i in (ga, gb) if i is not None}
    return {i: np.full(case['tensors'][i].shape, np.nan, F) for i in idx}


# ================================================================================================ l2_normalize_rows
def norm_rows(n):
    return {name: i for i, name in enumerate(NORM_NAMES)} if n >= len(NORM_NAMES) + 3 else {}


@functools.lru_cache(maxsize=None)
def norm_case(n, d, eps):
    """(x [n, d], dy [n, d]) in float32, read-only: N(0, 1) rows with the named rows of norm_rows(n) written over the first.
    exact_eps / below_eps are sqrt(eps) e_k and its float32 neighbour below (for eps = 2^-20: sq == eps exactly)."""
    rng = np.random.default_rng([n, d, int(eps * 2 ** 40)])
    x = rng.normal(size=(n, d)).astype(F)
    dy = rng.normal(size=(n, d)).astype(F)
    root = F(math.sqrt(eps))
    for name, r in norm_rows(n).items():
        k = r % d
        if name == 'zero':
            x[r] = 0.
        elif name == 'negzero':
            x[r] = -0.
        elif name == 'exact_eps':
            x[r] = 0.
            x[r, k] = root
        elif name == 'below_eps':
            x[r] = 0.
            x[r, k] = -np.nextafter(root, F(0))
        elif name == 'in_clamp':
            x[r] *= F(1e-4)
        elif name == 'large':
            x[r] *= F(1e3)
        elif name == 'one_hot':
            x[r] = 0.
            x[r, k] = 1.
    return _frozen(x, dy)


def _row_sum(terms):
    s = np.zeros(terms.shape[0], F)
    for k in range(terms.shape[1]):
        s = s + terms[:, k]
    return s


def l2_normalize_rows(x, eps):
    sq = _row_sum(x * x)
    inv = F(1.0) / np.sqrt(np.maximum(sq, F(eps)))
    return x * inv[:, None]


def l2_normalize_rows_bwd(x, dy, eps):
    sq = _row_sum(x * x)
    inv = F(1.0) / np.sqrt(np.maximum(sq, F(eps)))
    dot = _row_sum(x * dy)
    c = np.where(sq >= F(eps), ((dot * inv) * inv) * inv, F(0.0)).astype(F)
    return dy * inv[:, None] - x * c[:, None]


# ================================================================================================ light_smoothness
@functools.lru_cache(maxsize=None)
def light_case(h, w):
    """light [h, w, 3] uniform in [0, 3) (the recipe of the existing probe test), float32, read-only."""
    return _frozen(np.random.default_rng([h, w]).uniform(0., 3., size=(h, w, 3)).astype(F))[0]


def light_smoothness(light, tv, achro):
    """(loss, grad [h, w, 3]) of light_smoothness_kernel."""
    tv, achro = F(tv), F(achro)
    v = light
    pw, nw = np.roll(v, 1, 1), np.roll(v, -1, 1)
    ph, nh = np.roll(v, 1, 0), np.roll(v, -1, 0)
    pc, nc = np.roll(v, 1, 2), np.roll(v, -1, 2)        # channel (c + 2) % 3 and (c + 1) % 3
    dx, dy, dc = v - pw, v - ph, v - pc
    val = (tv * (dx * dx + dy * dy) + achro * (dc * dc)).reshape(-1)
    grad = F(2.0) * (tv * ((dx - (nw - v)) + (dy - (nh - v))) + achro * (dc - (nc - v)))
    part = np.zeros(256, F)
    for e0 in range(0, val.size, 256):                   # thread t adds elements t, t + 256, ... in order
        chunk = val[e0:e0 + 256]
        part[:chunk.size] = part[:chunk.size] + chunk
    k = 128
    while k > 0:
        part[:k] = part[:k] + part[k:2 * k]
        k >>= 1
    return part[0], grad.astype(F)


# ================================================================================================ amsgrad
def amsgrad_step_size(lr, beta1, beta2, step):
    """nfx_amsgrad_step_size: lr and the betas arrive as float32; the formula runs in double and is rounded once."""
    lr, b1, b2 = float(F(lr)), float(F(beta1)), float(F(beta2))
    return F(lr * math.sqrt(1.0 - math.pow(b2, float(step))) / (1.0 - math.pow(b1, float(step))))


def tf_step_size(lr, beta1, beta2, step):
    """Keras OptimizerV2 Adam._prepare_local (TF 2.2): pow, 1 - x, sqrt and the quotient all in float32."""
    lr, b1, b2, t = F(lr), F(beta1), F(beta2), F(step)
    return (lr * np.sqrt(F(1) - np.power(b2, t))) / (F(1) - np.power(b1, t))


def amsgrad(p, g, m, v, vhat, lr_t, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """(p, m, v, vhat) after amsgrad_kernel."""
    lr_t, b1, b2, eps = F(lr_t), F(b1), F(b2), F(eps)
    mi = m * b1 + g * (F(1.0) - b1)
    vi = v * b2 + (g * g) * (F(1.0) - b2)
    vh = np.maximum(vhat, vi)
    return p - (lr_t * mi) / (np.sqrt(vh) + eps), mi, vi, vh


def adam_rows(n):
    return {name: i for i, name in enumerate(ADAM_NAMES)} if n >= 255 else {}


@functools.lru_cache(maxsize=None)
def adam_case(n):
    """(p [n], g [ADAM_STEPS, n]) in float32, read-only; adam_rows(n) names the elements written over the first."""
    rng = np.random.default_rng(n)
    p = rng.normal(size=n).astype(F)
    g = rng.normal(size=(ADAM_STEPS, n)).astype(F)
    g[1] *= F(10.)                                         # (the existing test's second step)
    for name, i in adam_rows(n).items():
        if name == 'zero_grad':
            g[:, i] = 0.
        elif name == 'spike':                              # vhat stays above v from the second step on
            g[:, i] = 1e-3
            g[0, i] = 50.
        elif name == 'alternating':
            g[:, i] = F(0.7) * (-1.) ** np.arange(ADAM_STEPS)
        elif name == 'underflow':                          # g*g = 1e-40 is a float32 denormal, (1 - b2) g*g has 7 bits left
            g[:, i] = 1e-20
        elif name == 'huge':
            g[:, i] = 1e18
    return _frozen(p, g)


# ================================================================================================ embed
@functools.lru_cache(maxsize=None)
def embed_inputs(mode, n_src, per_ray):
    """(x, dir, z) as nfx_embed takes them for `mode`, float32, read-only, arguments inside +-3:
    0: x [n_src, 3]; 1: x = origins, dir = unit directions, z [n_src, per_ray] in [0.5, 2); 2: dir = unit directions;
    3: x = points [n_src, 3] in +-1, dir = lights [per_ray, 3] in +-3 — and, where there are 4 points or more, light 0 sits
    exactly on point 2 (the clamp makes that direction the zero vector)."""
    rng = np.random.default_rng([mode, n_src, per_ray])
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F)
    x = dirs = z = None
    if mode == 0:
        x = rng.uniform(-3, 3, size=(n_src, 3)).astype(F)
    elif mode == 1:
        x = rng.uniform(-1, 1, size=(n_src, 3)).astype(F)
        dirs = unit(rng.normal(size=(n_src, 3)))
        z = np.sort(rng.uniform(0.5, 2., size=(n_src, per_ray)).astype(F), 1)
    elif mode == 2:
        dirs = unit(rng.normal(size=(n_src, 3)))
    else:
        x = rng.uniform(-1, 1, size=(n_src, 3)).astype(F)
        dirs = rng.uniform(-3, 3, size=(per_ray, 3)).astype(F)
        if n_src >= 4:
            dirs[0] = x[2]
    return _frozen(x, dirs, z)


def embed_vectors(mode, x, dirs, z, per_ray):
    """v [rows, 3]: the vector embed_kernel encodes in each row."""
    if mode == 0:
        return np.repeat(x, per_ray, 0)
    if mode == 1:
        return (x[:, None, :] + dirs[:, None, :] * z[:, :, None]).reshape(-1, 3).astype(F)
    if mode == 2:
        return np.repeat(dirs, per_ray, 0)
    v = (dirs[None, :, :] - x[:, None, :]).reshape(-1, 3)
    sq = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    inv = F(1.0) / np.sqrt(np.maximum(sq, F(1e-6)))
    return (v * inv[:, None]).astype(F)


def embed_of(v, n_freqs, incl_input):
    """[v | sin(2^0 v) | cos(2^0 v) | sin(2^1 v) | ...] with sincos_cw."""
    cols = [v] if incl_input else []
    for f in range(n_freqs):
        sn, cs = sincos_cw(v * F(1 << f))
        cols += [sn, cs]
    return np.concatenate(cols, 1).astype(F)


def embed(mode, n_freqs, incl_input, x, dirs, z, per_ray):
    return embed_of(embed_vectors(mode, x, dirs, z, per_ray), n_freqs, incl_input)


@functools.lru_cache(maxsize=None)
def embed_bwd_case(n_freqs, incl_input, n, col0):
    """(v [n, 3] in +-3, d_out [n, col0 + d + EMBED_PAD] N(0, 1)), float32, read-only."""
    rng = np.random.default_rng([n_freqs, int(incl_input), n, col0])
    d = (3 if incl_input else 0) + 6 * n_freqs
    return _frozen(rng.uniform(-3, 3, size=(n, 3)).astype(F), rng.normal(size=(n, col0 + d + EMBED_PAD)).astype(F))


def embed_bwd(v, n_freqs, incl_input, d_out, col0):
    d = d_out[:, col0:]
    g = d[:, :3].copy() if incl_input else np.zeros((v.shape[0], 3), F)
    c = 3 if incl_input else 0
    for f in range(n_freqs):
        s = F(1 << f)
        sn, cs = sincos_cw(v * s)
        g = g + s * (cs * d[:, c:c + 3] - sn * d[:, c + 3:c + 6])
        c += 6
    return g.astype(F)


# ================================================================================================ the plain formulas in float64
# (torch on the host, imported where it is used: the rest of this module needs NumPy only)
def _t64(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def pair_loss_float64(case):
    """(loss [n], {tensor index: d sum(loss up) / d tensor}) by torch autograd."""
    import torch
    ts = [_t64(a, True) for a in case['tensors']]
    n = case['tensors'][0].shape[0]
    al = torch.ones(n, 1, dtype=torch.float64) if case['alpha'] is None else _t64(case['alpha']).reshape(n, 1)
    on_bg = lambda x: x * al + case['bg'] * (1. - al)
    total = 0.
    for ia, ib, w, kind, ba, bb in case['spec']:
        diff = (on_bg(ts[ia]) if ba else ts[ia]) - (on_bg(ts[ib]) if bb else ts[ib])
        total = total + float(F(w)) * (diff.abs() if kind == 'mae' else diff ** 2).mean(-1)
    used = sorted({i for ia, ib, *_ in case['spec'] for i in (ia, ib)})
    grads = torch.autograd.grad((total * _t64(case['up'])).sum(), [ts[i] for i in used])
    return total.detach().numpy(), {i: g.numpy() for i, g in zip(used, grads)}


def l2_normalize_float64(x, dy, eps):
    """(y, dx, the scale of a row's gradient as tests/test_gpu_regularizers.py takes it)."""
    import torch
    xr = _t64(x, True)
    yr = xr * torch.rsqrt(torch.clamp(torch.sum(xr * xr, dim=1, keepdim=True), min=float(F(eps))))
    (gr,) = torch.autograd.grad(yr, xr, _t64(dy))
    scale = np.abs(dy).max(axis=1, keepdims=True) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-3)
    return yr.detach().numpy(), gr.numpy(), scale


def light_float64(light, tv, achro):
    import torch
    lr = _t64(light, True)
    dx, dy, dc = lr - torch.roll(lr, 1, 1), lr - torch.roll(lr, 1, 0), lr - torch.roll(lr, 1, 2)
    ref = float(F(tv)) * (dx ** 2 + dy ** 2).sum() + float(F(achro)) * (dc ** 2).sum()
    (gr,) = torch.autograd.grad(ref, lr)
    return float(ref.detach()), gr.numpy()


def embed_float64(mode, n_freqs, incl_input, x, dirs, z, per_ray):
    """Modes 0 - 2 encode the float32 vector the kernel encodes (the existing test's reference: a float64 point moves the 2^9
    band by more than the tolerance); mode 3 normalises in float64 as well."""
    if mode == 3:
        v = dirs.astype(np.float64)[None] - x.astype(np.float64)[:, None]
        v = (v / np.sqrt(np.maximum((v * v).sum(2, keepdims=True), float(F(1e-6))))).reshape(-1, 3)
    else:
        v = embed_vectors(mode, x, dirs, z, per_ray).astype(np.float64)
    cols = [v] if incl_input else []
    for f in range(n_freqs):
        cols += [np.sin(v * 2. ** f), np.cos(v * 2. ** f)]
    return np.concatenate(cols, 1)


def embed_bwd_float64(v, n_freqs, incl_input, d_out, col0):
    v64, d = v.astype(np.float64), d_out.astype(np.float64)[:, col0:]
    want = d[:, :3].copy() if incl_input else np.zeros((v.shape[0], 3))
    c = 3 if incl_input else 0
    for k in range(n_freqs):
        want += 2. ** k * (np.cos(2. ** k * v64) * d[:, c:c + 3] - np.sin(2. ** k * v64) * d[:, c + 3:c + 6])
        c += 6
    return want


def amsgrad_float64(p0, gs, lr=ADAM_LR):
    """[(p, vhat) after each step] in float64, with the float32 betas, eps and step sizes the kernel gets."""
    b1, b2, eps = (float(F(a)) for a in (ADAM_B1, ADAM_B2, ADAM_EPS))
    n = p0.shape[0]
    p, m, v, vh = p0.astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n)
    out = []
    for step in range(1, gs.shape[0] + 1):
        g = gs[step - 1].astype(np.float64)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        vh = np.maximum(vh, v)
        p = p - float(amsgrad_step_size(lr, ADAM_B1, ADAM_B2, step)) * m / (np.sqrt(vh) + eps)
        out.append((p.copy(), vh.copy()))
    return out
