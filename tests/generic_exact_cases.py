"""Integer networks for the runtime-shaped MLP kernels (csrc/mlp_generic.hip) and their int64 reference.

Nothing inside mlp_generic_kernel / mlp_generic_bwd_kernel / mlp_generic_wgrad_kernel is transcendental once the activations
are ReLU or linear: a forward or backward pass is sums of products of numbers the test chooses.  With small integer inputs,
biases and dy, and weights in {-1, 0, +1}, every partial sum the kernels can form is an integer below 2^24 — exact in fp32 in
ANY order, under any split of the rows and in any of the three MFMA forms — so the kernels are held to an integer reference
with no tolerance.  The reference applies the roundings the kernels apply, where they apply them:
  bf16         the network input, every hidden activation and every propagated gradient dZ is rounded to bf16 (round to
               nearest even) when it is stored to LDS; the accumulators, the output row y and the input gradient dx are fp32;
  fp32_native  nothing is rounded;
  fp32         (hi / lo bf16 pairs) hi + lo is the value itself while it stays below 2^16; the forward and the dgrad drop
               a_lo b_lo with a = the weights, whose lo plane is zero for -1 / 0 / +1; the weight-gradient kernel drops
               lo(IN) lo(dZ), where NEITHER operand is a weight: dropped_lo_lo() is what it leaves out, and the CPU test
               holds it to zero row by row (one of the two factors always has at most 8 significant bits).
ReLU's derivative at 0 is 0 (TensorFlow's convention); integer data gives many pre-activations that are exactly 0.

tests/test_cpu_generic_exact_cases.py proves the conditions from each case's own data; tests/test_gpu_generic_exact.py runs them.
"""
import functools

import numpy as np

from oracle import nerf_ref

PRECS = ('bf16', 'fp32', 'fp32_native')
N_MAX = 1299                      # 41 row tiles, the last one 19 rows: wgrad_splits() gives 10 uneven splits
# every row count a case is run at (prefixes of its N_MAX rows): one row, around one tile, around four tiles (= one
# workgroup of four waves), 10 tiles (under nerf_blocks = 1 = 8 waves, two of them walk a second row tile), 41 tiles
ROWS = (1, 31, 32, 33, 127, 128, 129, 289, N_MAX)

# name: (d_in, widths, acts, skip_at, non-zero weights per column (None: dense), share of rows with a non-zero dy[, max |dy|:
# 1 unless stated; 'two_skips' takes 9, so that its propagated gradients pass 256 and the bf16 mode's rounding of dZ acts])
# The shapes of test_generic_mlp_vs_oracle / test_generic_mlp_backward_vs_oracle with ReLU for softplus / sigmoid on hidden
# layers and a linear output ('one256' keeps its ReLU output: the output layer's own mask, taken from the logit).
SHAPES = {
    'w96x4_skip1': (63, [96, 96, 96, 96, 5], ['relu'] * 4 + [None], [1], 8, 1.0),
    'in3': (3, [64, 64, 4], ['relu', 'relu', None], None, None, 1.0),
    'w256x8_skip4': (90, [256] * 8 + [1], ['relu'] * 8 + [None], [4], 6, 0.25),
    'two_skips': (27, [40, 200, 33], ['relu', 'relu', None], [0, 1], None, 1.0, 9),
    'one256': (128, [256], ['relu'], None, None, 1.0),
    'in283': (283, [128, 3], ['relu', None], None, None, 1.0),
    'w128x3_skip1': (39, [128, 128, 128, 1], ['relu'] * 3 + [None], [1], 8, 1.0),
    'wide288': (63, [512, 512, 288, 512, 4], ['relu'] * 4 + [None], [1], 16, 1.0),
    'wide320': (63, [512, 320, 512, 2], ['relu'] * 3 + [None], [1], 16, 1.0),
    'in539': (539, [256, 3], ['relu', None], None, None, 1.0),
}


class Case:
    pass


def _ternary(rng, fan_in, fan_out, nnz):
    w = np.zeros((fan_in, fan_out), np.int64)
    if nnz is None or nnz >= fan_in or fan_out <= 33:
        # dense (narrow output layers stay dense: every fragment of their transposed form holds a non-zero too)
        w[:] = rng.integers(-1, 2, size=w.shape)
        return w
    for c in range(fan_out):
        rows = rng.choice(fan_in, size=nnz, replace=False)
        w[rows, c] = rng.choice([-1, 1], size=nnz)
    return w


@functools.lru_cache(maxsize=None)
def case(name):
    d_in, widths, acts, skip_at, nnz, dy_share = SHAPES[name][:6]
    dy_max = SHAPES[name][6] if len(SHAPES[name]) > 6 else 1
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 1000)
    c = Case()
    c.name, c.d_in, c.widths, c.acts, c.skip_at, c.nnz, c.dy_share = name, d_in, list(widths), list(acts), list(skip_at or []), nnz, dy_share
    c.in_dims, prev = [], d_in
    c.layers = []
    for i, w in enumerate(widths):
        c.in_dims.append(prev)
        # a positive bias on hidden layers keeps most units alive at small fan-ins
        c.layers.append((_ternary(rng, prev, w, nnz), rng.integers(-2, 4, size=w).astype(np.int64)))
        prev = w + (d_in if i in c.skip_at else 0)
    c.x = rng.integers(-3, 4, size=(N_MAX, d_in)).astype(np.int64)
    c.dy = rng.integers(-dy_max, dy_max + 1, size=(N_MAX, widths[-1])).astype(np.int64)
    c.dy[rng.random(N_MAX) >= dy_share] = 0
    c.dy[[0, 30, 31, 32, 126, 127, 128, 288, N_MAX - 1]] = dy_max * (1 - 2 * rng.integers(0, 2, size=(9, widths[-1])))   # the edge rows always count
    # what dW / db hold before the call: the kernels ADD
    c.dw0 = [rng.integers(-50, 51, size=k.shape).astype(np.int64) for k, _ in c.layers]
    c.db0 = [rng.integers(-50, 51, size=b.shape).astype(np.int64) for _, b in c.layers]
    return c


# ---------------------------------------------------------------------------------------------------- the reference
def imatmul(a, b):
    """a @ b of int64 matrices through float64 BLAS: exact while every sum of |products| stays below 2^53 (the conditions keep
    them below 2^24; tests/test_cpu_generic_exact_cases.py compares with numpy's int64 product)."""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def bf16(a):
    return nerf_ref.bf16_round(a.astype(np.float32)).astype(np.int64)


def hi_lo(a):
    hi = bf16(a)
    return hi, bf16(a - hi)


def stored(prec, a):
    """what an activation or gradient becomes when the kernel stores it to LDS / the workspace"""
    return bf16(a) if prec == 'bf16' else a


def _mag(prec, a):
    """|operand| as the matrix pipe sees it: the pairs mode multiplies hi and lo separately"""
    if prec == 'fp32':
        hi, lo = hi_lo(a)
        return np.abs(hi) + np.abs(lo)
    return np.abs(a)


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(name, prec):
    """Everything per row for the case's N_MAX rows (a launch on n rows sees the first n): y, dx, every layer's stored input IN
    and stored gradient dZ, and `worst` = the largest sum of |products| (+ |bias|) any accumulator of the three kernels can
    hold, `peak` = the largest |activation or gradient|."""
    c = case(name)
    r = Ref()
    nl = len(c.layers)
    x = stored(prec, c.x)
    r.ins, r.hs, worst, peak = [], [], 0, int(np.abs(x).max())
    h = x
    for i, (k, b) in enumerate(c.layers):
        r.ins.append(h)
        z = imatmul(h, k) + b
        worst = max(worst, int((imatmul(_mag(prec, h), np.abs(k)) + np.abs(b)).max()))
        if i == nl - 1:
            r.z_last = z
            r.y = np.maximum(z, 0) if c.acts[i] == 'relu' else z
            break
        h = stored(prec, np.maximum(z, 0) if c.acts[i] == 'relu' else z)
        r.hs.append(h)
        peak = max(peak, int(np.abs(h).max()))
        if i in c.skip_at:
            h = np.concatenate([h, x], 1)
    # backward: relu'(0) = 0
    d = c.dy * (r.z_last > 0) if c.acts[-1] == 'relu' else c.dy
    r.dzs = [None] * nl
    r.dx, dx_abs = np.zeros_like(c.x), np.zeros_like(c.x)
    for i in range(nl - 1, -1, -1):
        d = stored(prec, d)
        r.dzs[i] = d
        peak = max(peak, int(np.abs(d).max()))
        k = c.layers[i][0]
        prev = c.widths[i - 1] if i else 0
        if k.shape[0] > prev:                      # this layer reads the network input: its share of dx (fp32, added in place)
            r.dx = r.dx + imatmul(d, k[prev:].T)
            dx_abs = dx_abs + imatmul(_mag(prec, d), np.abs(k[prev:].T))
        if i:
            g = imatmul(d, k[:prev].T)
            worst = max(worst, int(imatmul(_mag(prec, d), np.abs(k[:prev].T)).max()))
            d = g * (r.hs[i - 1] > 0) if c.acts[i - 1] == 'relu' else g
    worst = max(worst, int(dx_abs.max()))
    peak = max(peak, int(np.abs(r.dx).max()))
    for i in range(nl):                            # dW = IN^T dZ and db = 1^T dZ over all rows, plus what the buffers held
        s = imatmul(_mag(prec, r.ins[i]).T, _mag(prec, r.dzs[i])) + np.abs(c.dw0[i])
        worst = max(worst, int(s.max()), int((_mag(prec, r.dzs[i]).sum(0) + np.abs(c.db0[i])).max()))
    r.worst, r.peak = worst, peak
    return r


@functools.lru_cache(maxsize=64)
def weight_grads(name, prec, n):
    """(dW, db) a launch on the first n rows leaves in buffers that held case.dw0 / db0"""
    c, r = case(name), reference(name, prec)
    dws, dbs = [], []
    for i in range(len(c.layers)):
        dws.append(c.dw0[i] + imatmul(r.ins[i][:n].T, r.dzs[i][:n]))
        dbs.append(c.db0[i] + r.dzs[i][:n].sum(0))
    return dws, dbs


def dropped_lo_lo(name):
    """per layer, sum over all rows of |lo(IN)|^T |lo(dZ)|: what the pairs mode's weight-gradient kernel does not add"""
    r = reference(name, 'fp32')
    return [int(imatmul(np.abs(hi_lo(i)[1]).T, np.abs(hi_lo(d)[1])).max()) for i, d in zip(r.ins, r.dzs)]


# ---------------------------------------------------------------------- what the host decides, restated (capi_generic.cpp)
def n_tiles(w):
    return (w + 31) // 32


def pitches(d_in, widths, prec):
    elem = 2 if prec == 'bf16' else 4
    widest = max(n_tiles(w) for w in widths)
    return (d_in + 63) // 64 * 64 * elem + 16, (widest + 1) // 2 * 64 * elem + 16


def instantiation(name, prec, n):
    """(NW, WIDE) of mlp_generic_kernel / mlp_generic_bwd_kernel<M, NW, WIDE> that a launch on n rows runs: generic_waves()
    and wide_layers() of mlp_generic.hip."""
    c = case(name)
    wide = any(n_tiles(w) > 8 for w in c.widths)
    if prec == 'bf16' or wide:
        return 1, wide
    xp, hp = pitches(c.d_in, c.widths, prec)
    ring, act, tiles, nw = 3 * 4 * 2048, 32 * (xp + hp), (n + 31) // 32, 4
    while nw > 1 and (ring + nw * act > 160 * 1024 or tiles < nw):
        nw //= 2
    return nw, False


def wgrad_jobs(name):
    c = case(name)
    mx, jobs = n_tiles(c.d_in), 0
    for i, w in enumerate(c.widths):
        reads_x = i == 0 or (i - 1) in c.skip_at
        m_in = (n_tiles(c.widths[i - 1]) if i else 0) + (mx if reads_x else 0)
        jobs += (m_in + 1) // 2 * ((n_tiles(w) + 1) // 2)
    return jobs


def wgrad_splits(name, n, cap=256):
    """wgrad_splits() of capi_generic.cpp, and the row tiles [t0, t1) each split sums (mlp_generic_wgrad_kernel)"""
    tiles, jobs = (n + 31) // 32, wgrad_jobs(name)
    s = max(1, min((8192 + jobs - 1) // jobs, tiles // 4, cap))
    return s, [(tiles * sp // s, tiles * (sp + 1) // s) for sp in range(s)]
