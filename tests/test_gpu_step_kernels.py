"""The small kernels of a training step — pair_loss_kernel (csrc/loss.hip), l2_normalize_rows_kernel and light_smoothness_kernel
(csrc/regularizers.hip), amsgrad_kernel / amsgrad_dev_kernel (csrc/train.hip), embed_kernel / embed_bwd_kernel
(csrc/mlp_generic.hip) — against the float32 restatements of tests/step_kernel_cases.py, BIT FOR BIT, at the shapes where they
change course: a loss width on either side of the 64-lane stride, ray counts that leave waves of the last workgroup idle, every
row width of the normaliser and the row whose sum of squares IS eps, probes whose previous and next neighbour are one texel and
element counts on either side of the 256-thread stride, the optimizer at the 256-thread boundary, every input mode of the encoder.

Why the bit equalities must hold: the library is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded in these
files, float32 denormals are kept, and no reduction depends on the launch — each kernel has one right answer per input, which the
restatement gives (include/nfx.h states the operation order).  -0 is not +0 here: the comparison is on the bits.
Beside the bits:
  * exactly the stated elements are written: outputs start NaN-filled with guard rows around them (the encoder: guard columns on
    both sides too), no NaN stays and no guard changes; a null ga / gb leaves that tensor's buffer alone;
  * a ray, row or element evaluated alone gives the bits it gives inside the batch;
  * the same outputs against float64 at the tolerances the project already uses (step_kernel_cases.*_TOL) — which
    tests/test_cpu_step_kernel_cases.py shows to hold with a factor of two to spare whenever the bits are right;
  * refusals are error codes and no launch follows; n = 0 is NFX_OK and writes nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_kernel_cases as C

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL = -1
NAN = float('nan')


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(cuda)       # (a copy: the cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _guarded(shape, cuda, fill=NAN):
    """(buffer [rows + 2, ...] full of `fill`, its rows 1 .. rows as the tensor the kernel gets)."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=torch.float32, device=cuda)
    return buf, buf[1:shape[0] + 1]


def _guards_kept(buf, what):
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), what + ': written outside the output'


def _written(buf, what):
    _guards_kept(buf, what)
    assert not bool(torch.isnan(buf[1:-1]).any()), what + ': a slot was never written'


def _assert_bits(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype == F and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    differ = np.argwhere(C.bits(got) != C.bits(want))
    assert len(differ) == 0, (what, len(differ), differ[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in differ[:4]])


def _close(got, want, rtol, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    over = np.abs(got - want) - (atol + rtol * np.abs(want))
    assert over.max() <= 0, (what, float(np.abs(got - want).max()))


# ================================================================================================ pair_loss
def _loss_launch(case, cuda, init=None, rows=slice(None)):
    """Runs nfx_pair_loss_fwd into a guarded NaN-filled loss and ops.pair_loss_bwd into guarded buffers that start as `init`
    (NaN where not given).  Returns (loss, {tensor index: gradient buffer}) on the host."""
    from nerfactor_amd import _capi, ops
    tensors = [dev(t[rows], cuda) for t in case['tensors']]
    n = tensors[0].shape[0]
    alpha = dev(case['alpha'][rows], cuda) if case['alpha'] is not None else None
    terms = [(tensors[ia], tensors[ib], w, kind, ba, bb) for ia, ib, w, kind, ba, bb in case['spec']]
    table, n_ = ops._loss_table(terms)
    lbuf, loss = _guarded((n,), cuda)
    _capi.check(_capi.lib.nfx_pair_loss_fwd(table, len(terms), _ptr(alpha), float(case['bg']), n_, loss.data_ptr(), _stream()), 'fwd')
    torch.cuda.synchronize()
    _written(lbuf, 'loss')
    init = C.loss_nan_init(case) if init is None else init
    bufs = {}
    for i, a in init.items():
        bufs[i] = _guarded(a[rows].shape, cuda)
        bufs[i][1].copy_(dev(a[rows], cuda))
    grads = [(bufs[ga][1] if ga is not None else None, bufs[gb][1] if gb is not None else None, acc_a, acc_b)
             for ga, gb, acc_a, acc_b in case['plan']]
    ops.pair_loss_bwd(terms, grads, dev(case['up'][rows], cuda), alpha=alpha, bg=case['bg'])
    torch.cuda.synchronize()
    for i, (buf, _) in bufs.items():
        _written(buf, 'gradient of tensor %d' % i)
    return host(loss), {i: host(g) for i, (_, g) in bufs.items()}


def _loss_check(case, cuda, what, float64):
    loss, grads = _loss_launch(case, cuda)
    _assert_bits(loss, C.pair_loss_fwd(case['tensors'], case['spec'], case['alpha'], case['bg']), what + ' loss')
    want = C.pair_loss_bwd(case['tensors'], case['spec'], case['plan'], case['alpha'], case['bg'], case['up'], C.loss_nan_init(case))
    assert set(want) == set(grads)
    for i in want:
        _assert_bits(grads[i], want[i], what + ' gradient of tensor %d' % i)
    if float64:
        ref, ref_g = C.pair_loss_float64(case)
        _close(loss, ref, C.LOSS_RTOL, C.LOSS_ATOL, what + ' loss against float64')
        full = all(ga is not None and gb is not None for ga, gb, _, _ in case['plan'])
        for i in (grads if full else ()):
            _close(grads[i], ref_g[i], C.LOSS_G_RTOL, C.LOSS_G_ATOL, what + ' gradient %d against float64' % i)


LOSS_IDS = ['n%d-D%d' % c for c in C.LOSS_SHAPES]


@pytest.mark.parametrize("n,d", C.LOSS_SHAPES, ids=LOSS_IDS)
def test_pair_loss_one_term_is_bit_equal_to_the_restatement(nfx_lib, cuda, n, d):
    for kind in ('mse', 'mae'):
        for ba, bb in ((True, True), (True, False), (False, False)):
            for bg in C.LOSS_BG:
                for grid in (True, False):
                    case = C.loss_one_term(n, d, kind, ba, bb, bg, grid)
                    _loss_check(case, cuda, '%s blend %d%d bg %g grid %d' % (kind, ba, bb, bg, grid), float64=grid)


@pytest.mark.parametrize("n,d", [(13, 65), (5, 65), (13, 1)], ids=['n13-D65', 'n5-D65', 'n13-D1'])
def test_pair_loss_accumulate_flags_and_null_buffers(nfx_lib, cuda, n, d):
    """The flags are the caller's: ACCUM_A / ACCUM_B on the only term add to what the buffers hold, without them the same
    buffers are overwritten; with ga (gb) null the other side gets the same bits and nothing else is touched."""
    rng = np.random.default_rng(n + d)
    for kind in ('mse', 'mae'):
        case = dict(C.loss_one_term(n, d, kind, True, False, 1., False))
        held = {i: rng.normal(size=(n, d)).astype(F) for i in (0, 1)}
        for acc_a, acc_b in ((True, True), (True, False), (False, True), (False, False)):
            case['plan'] = [(0, 1, acc_a, acc_b)]
            _, grads = _loss_launch(case, cuda, init=held)
            want = C.pair_loss_bwd(case['tensors'], case['spec'], case['plan'], case['alpha'], case['bg'], case['up'], held)
            for i in (0, 1):
                _assert_bits(grads[i], want[i], 'accumulate %d%d tensor %d' % (acc_a, acc_b, i))
        both = C.pair_loss_bwd(case['tensors'], case['spec'], [(0, 1, False, False)], case['alpha'], case['bg'], case['up'], held)
        for plan, kept in (([(0, None, False, False)], 0), ([(None, 1, False, False)], 1)):
            case['plan'] = plan
            _, grads = _loss_launch(case, cuda)
            assert set(grads) == {kept}
            _assert_bits(grads[kept], both[kept], 'one side only')


@pytest.mark.parametrize("name", C.LOSS_SETS)
def test_pair_loss_term_sets_are_bit_equal_to_the_restatement(nfx_lib, cuda, name):
    for bg in C.LOSS_BG:
        for grid in (True, False):
            _loss_check(C.loss_term_set(name, bg, grid), cuda, '%s bg %g grid %d' % (name, bg, grid), float64=grid)


@pytest.mark.parametrize("name", ['eight', 'a_then_b'])
def test_pair_loss_ray_alone_equals_the_ray_in_the_batch(nfx_lib, cuda, name):
    case = C.loss_term_set(name, 1., False)
    loss, grads = _loss_launch(case, cuda)
    for r in (0, 1, 3, 4, 12):
        one_loss, one_grads = _loss_launch(case, cuda, rows=slice(r, r + 1))
        _assert_bits(one_loss, loss[r:r + 1], 'loss of ray %d' % r)
        for i in grads:
            _assert_bits(one_grads[i], grads[i][r:r + 1], 'gradient %d of ray %d' % (i, r))


def test_pair_loss_autograd_bookkeeping_against_float64(nfx_lib, cuda):
    """autograd.PairLoss decides what the kernel writes and what it adds: a tensor in two terms (A then B), a term neither of
    whose operands needs a gradient (skipped in the backward), a tensor that needs a gradient and is in no term (zeros), and
    the refusal of a term of a tensor with itself."""
    from nerfactor_amd import autograd
    n, d = 13, 65
    rng = np.random.default_rng(5)
    grid = lambda: (rng.integers(0, 256, size=(n, d)) / 256.).astype(F)
    arrays = [grid() for _ in range(6)]
    needs = [True, False, True, False, False, True]              # tensor 5 is in no term; term (3, 4) needs nothing
    spec = ((0, 1, 1., 'mse', True, True), (2, 0, 0.3, 'mae', False, True), (3, 4, 0.5, 'mse', False, False),
            (2, 1, 0.05, 'mse', True, False))
    alpha, up = C._alpha_up(rng, n, True)
    case = dict(tensors=arrays, spec=spec, alpha=alpha, bg=1., up=up)
    want, want_g = C.pair_loss_float64(case)
    ts = [dev(a, cuda).requires_grad_(nd) for a, nd in zip(arrays, needs)]
    got = autograd.PairLoss.apply(dev(alpha, cuda).reshape(n, 1), 1., spec, *ts)
    _assert_bits(got, C.pair_loss_fwd(arrays, spec, alpha, 1.), 'loss')
    _close(host(got), want, C.LOSS_RTOL, C.LOSS_ATOL, 'loss against float64')
    got_g = torch.autograd.grad((got * dev(up, cuda)).sum(), [t for t, nd in zip(ts, needs) if nd])
    plan = C.loss_plan(spec, 6, need=needs)
    live = [(t, p) for t, p in zip(spec, plan) if p[0] is not None or p[1] is not None]
    assert len(live) == 3 and plan[1] == (2, 0, False, True) and plan[3] == (2, None, True, False)
    rest = C.pair_loss_bwd(arrays, [t for t, _ in live], [p for _, p in live], alpha, 1., up,
                           {i: np.full((n, d), np.nan, F) for i in (0, 2)})
    for i, g in zip((0, 2), got_g[:2]):
        _assert_bits(g, rest[i], 'gradient of tensor %d' % i)
        _close(host(g), want_g[i], C.LOSS_G_RTOL, C.LOSS_G_ATOL, 'gradient %d against float64' % i)
    assert got_g[2].shape == (n, d) and not bool(got_g[2].any())
    same = autograd.PairLoss.apply(None, 0., ((0, 0, 1., 'mse', False, False),), ts[0])
    with pytest.raises(ValueError, match='two different tensors'):
        same.sum().backward()


class _Term(ctypes.Structure):
    _fields_ = [('a', ctypes.c_void_p), ('b', ctypes.c_void_p), ('ga', ctypes.c_void_p), ('gb', ctypes.c_void_p),
                ('d', ctypes.c_int), ('w', ctypes.c_float), ('kind', ctypes.c_int), ('flags', ctypes.c_int)]


def test_pair_loss_refusals_are_error_codes_and_nothing_is_launched(nfx_lib, cuda):
    lib = nfx_lib.lib
    n, d = 5, 3
    a, b, up = (torch.ones((n, d), device=cuda) for _ in range(3))
    ga, gb = torch.full((n, d), NAN, device=cuda), torch.full((n, d), NAN, device=cuda)
    loss = torch.full((n,), NAN, device=cuda)

    def term(**kw):
        f = dict(a=a.data_ptr(), b=b.data_ptr(), ga=ga.data_ptr(), gb=gb.data_ptr(), d=d, w=1., kind=0, flags=0)
        f.update(kw)
        return _Term(**f)

    def bwd(terms, n_terms, n_rays=n):
        table = (_Term * max(len(terms), 1))(*terms)
        return lib.nfx_pair_loss_bwd(table, n_terms, None, 0., n_rays, up.data_ptr(), _stream())

    def both(terms, n_terms, n_rays=n):
        table = (_Term * max(len(terms), 1))(*terms)
        return lib.nfx_pair_loss_fwd(table, n_terms, None, 0., n_rays, loss.data_ptr(), _stream()), bwd(terms, n_terms, n_rays)

    assert both([term()], 0) == (EINVAL, EINVAL)
    assert both([term()] * 9, 9) == (EINVAL, EINVAL)
    assert both([term(d=0)], 1) == (EINVAL, EINVAL)
    assert both([term(kind=2)], 1) == (EINVAL, EINVAL)
    assert both([term(a=None)], 1) == (EINVAL, EINVAL) and both([term(), term(b=None)], 2) == (EINVAL, EINVAL)
    assert both([term()], 1, n_rays=-1) == (EINVAL, EINVAL)
    assert bwd([term(ga=None, flags=4)], 1) == EINVAL and bwd([term(gb=None, flags=8)], 1) == EINVAL     # (the forward reads no flag)
    assert lib.nfx_pair_loss_fwd(None, 1, None, 0., n, loss.data_ptr(), _stream()) == EINVAL
    assert both([term()], 1, n_rays=0) == (0, 0)                 # n = 0: NFX_OK, nothing written
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (ga, gb, loss))


# ================================================================================================ l2_normalize_rows
def _norm_launch(lib, x, dy, eps, cuda):
    n, d = x.shape
    xd, dyd = dev(x, cuda), dev(dy, cuda)
    ybuf, y = _guarded((n, d), cuda)
    gbuf, g = _guarded((n, d), cuda)
    assert lib.nfx_l2_normalize_rows(xd.data_ptr(), y.data_ptr(), n, d, eps, _stream()) == 0
    assert lib.nfx_l2_normalize_rows_bwd(xd.data_ptr(), dyd.data_ptr(), g.data_ptr(), n, d, eps, _stream()) == 0
    torch.cuda.synchronize()
    _written(ybuf, 'y')
    _written(gbuf, 'dx')
    return host(y), host(g)


@pytest.mark.parametrize("n,d", C.NORM_SHAPES, ids=['n%d-d%d' % c for c in C.NORM_SHAPES])
def test_l2_normalize_rows_is_bit_equal_to_the_restatement(nfx_lib, cuda, n, d):
    for eps in C.NORM_EPS:
        x, dy = C.norm_case(n, d, eps)
        y, g = _norm_launch(nfx_lib.lib, x, dy, eps, cuda)
        _assert_bits(y, C.l2_normalize_rows(x, eps), 'y, eps %g' % eps)
        _assert_bits(g, C.l2_normalize_rows_bwd(x, dy, eps), 'dx, eps %g' % eps)
        yr, gr, scale = C.l2_normalize_float64(x, dy, eps)
        assert np.abs(y - yr).max() < C.NORM_TOL_Y and (np.abs(g - gr) / scale).max() < C.NORM_TOL_G
        for r in sorted(set(C.norm_rows(n).values()) | {0, n - 1}):       # a row alone gives the bits it gives in the batch
            y1, g1 = _norm_launch(nfx_lib.lib, x[r:r + 1], dy[r:r + 1], eps, cuda)
            _assert_bits(y1, y[r:r + 1], 'row %d alone' % r)
            _assert_bits(g1, g[r:r + 1], 'row %d alone, dx' % r)


def test_l2_normalize_rows_refusals_and_nothing(nfx_lib, cuda):
    lib = nfx_lib.lib
    x, out = torch.ones((4, 17), device=cuda), torch.full((4, 17), NAN, device=cuda)
    for d in (0, 17):
        assert lib.nfx_l2_normalize_rows(x.data_ptr(), out.data_ptr(), 4, d, 1e-6, _stream()) == EINVAL
        assert lib.nfx_l2_normalize_rows_bwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), 4, d, 1e-6, _stream()) == EINVAL
    assert lib.nfx_l2_normalize_rows(x.data_ptr(), out.data_ptr(), -1, 3, 1e-6, _stream()) == EINVAL
    assert lib.nfx_l2_normalize_rows(None, out.data_ptr(), 4, 3, 1e-6, _stream()) == EINVAL
    assert lib.nfx_l2_normalize_rows(x.data_ptr(), out.data_ptr(), 0, 3, 1e-6, _stream()) == 0
    assert lib.nfx_l2_normalize_rows_bwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), 0, 3, 1e-6, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ================================================================================================ light_smoothness
@pytest.mark.parametrize("h,w", C.LIGHT_SHAPES, ids=['%dx%d' % s for s in C.LIGHT_SHAPES])
def test_light_smoothness_is_bit_equal_to_the_restatement(nfx_lib, cuda, h, w):
    light = C.light_case(h, w)
    ld = dev(light, cuda)
    for tv, achro in C.LIGHT_WEIGHTS:
        gbuf, grad = _guarded((h, w, 3), cuda)
        lbuf, loss = _guarded((1,), cuda)
        assert nfx_lib.lib.nfx_light_smoothness(ld.data_ptr(), h, w, tv, achro, loss.data_ptr(), grad.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        _written(gbuf, 'grad')
        _written(lbuf, 'loss')
        want_loss, want_grad = C.light_smoothness(light, tv, achro)
        _assert_bits(loss, np.array([want_loss], F), 'loss (%g, %g)' % (tv, achro))
        _assert_bits(grad, want_grad, 'grad (%g, %g)' % (tv, achro))
        ref, gr = C.light_float64(light, tv, achro)
        assert abs(float(loss) - ref) <= C.LIGHT_TOL * abs(ref) + 1e-12
        assert np.abs(host(grad) - gr).max() <= C.LIGHT_TOL * np.abs(gr).max() + 1e-12


def test_light_smoothness_refusals(nfx_lib, cuda):
    lib = nfx_lib.lib
    light, loss, grad = torch.ones((4, 4, 3), device=cuda), torch.full((1,), NAN, device=cuda), torch.full((4, 4, 3), NAN, device=cuda)
    call = lambda h, w, lp=light.data_ptr(): lib.nfx_light_smoothness(lp, h, w, 1., 1., loss.data_ptr(), grad.data_ptr(), _stream())
    assert call(0, 4) == EINVAL and call(4, 0) == EINVAL and call(1 << 10, (1 << 10) + 1) == EINVAL and call(4, 4, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(grad).all())


# ================================================================================================ amsgrad
class _AdamState:
    """p, m, v, vhat with a guard element on each side of each."""

    def __init__(self, p0, cuda):
        n = p0.shape[0]
        self.bufs = [_guarded((n,), cuda)[0] for _ in range(4)]
        self.t = [b[1:n + 1] for b in self.bufs]
        self.t[0].copy_(dev(p0, cuda))
        for t in self.t[1:]:
            t.zero_()

    def check(self, want, what):
        for name, buf, t, w in zip(('p', 'm', 'v', 'vhat'), self.bufs, self.t, want):
            _guards_kept(buf, what + ' ' + name)
            _assert_bits(t, w, what + ' ' + name)


@pytest.mark.parametrize("n", C.ADAM_N)
def test_amsgrad_kernels_are_bit_equal_to_the_restatement_and_to_each_other(nfx_lib, cuda, n):
    from nerfactor_amd import ops
    p0, gs = C.adam_case(n)
    host_lr, dev_lr = _AdamState(p0, cuda), _AdamState(p0, cuda)
    word = torch.zeros(1, device=cuda)
    want = (p0.copy(), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F))
    ref = C.amsgrad_float64(p0, gs)
    keep = np.ones(n, bool)
    keep[[i for name, i in C.adam_rows(n).items() if name == 'underflow']] = False
    for step in range(1, C.ADAM_STEPS + 1):
        g = dev(gs[step - 1], cuda)
        lr_t = ops.amsgrad_step_size(C.ADAM_LR, step)
        assert C.same_bits(F(lr_t), C.amsgrad_step_size(C.ADAM_LR, C.ADAM_B1, C.ADAM_B2, step))
        ops.amsgrad_step(*host_lr.t[:1], g, *host_lr.t[1:], C.ADAM_LR, step)
        word.fill_(lr_t)
        ops.amsgrad_step_dev(*dev_lr.t[:1], g, *dev_lr.t[1:], word)
        want = C.amsgrad(want[0], gs[step - 1], want[1], want[2], want[3], C.amsgrad_step_size(C.ADAM_LR, C.ADAM_B1, C.ADAM_B2, step))
        host_lr.check(want, 'step %d, amsgrad_kernel' % step)
        dev_lr.check(want, 'step %d, amsgrad_dev_kernel' % step)
        _close(host(host_lr.t[0]), ref[step - 1][0], C.ADAM_P_RTOL, C.ADAM_P_ATOL, 'p against float64')
        _close(host(host_lr.t[3])[keep], ref[step - 1][1][keep], C.ADAM_VH_RTOL, 0., 'vhat against float64')


def test_amsgrad_element_alone_and_refusals(nfx_lib, cuda):
    from nerfactor_amd import ops
    n = 257
    p0, gs = C.adam_case(n)
    batch = _AdamState(p0, cuda)
    alone = {i: _AdamState(p0[i:i + 1], cuda) for i in list(C.adam_rows(n).values()) + [255, 256]}
    for step in range(1, C.ADAM_STEPS + 1):
        ops.amsgrad_step(*batch.t[:1], dev(gs[step - 1], cuda), *batch.t[1:], C.ADAM_LR, step)
        for i, st in alone.items():
            ops.amsgrad_step(*st.t[:1], dev(gs[step - 1, i:i + 1], cuda), *st.t[1:], C.ADAM_LR, step)
            st.check([host(t)[i:i + 1] for t in batch.t], 'element %d alone, step %d' % (i, step))
    before = [host(t).copy() for t in batch.t]
    lib, ptrs, g = nfx_lib.lib, [t.data_ptr() for t in batch.t], dev(gs[0], cuda)
    step_ = lambda n_, step: lib.nfx_amsgrad_step(ptrs[0], g.data_ptr(), ptrs[1], ptrs[2], ptrs[3], n_, C.ADAM_LR, C.ADAM_B1,
                                                  C.ADAM_B2, C.ADAM_EPS, step, _stream())
    assert step_(n, 0) == EINVAL and step_(n, -3) == EINVAL and step_(-1, 1) == EINVAL and step_(0, 1) == 0
    assert lib.nfx_amsgrad_step_dev(ptrs[0], g.data_ptr(), ptrs[1], ptrs[2], ptrs[3], n, None, C.ADAM_B1, C.ADAM_B2, C.ADAM_EPS,
                                    _stream()) == EINVAL
    torch.cuda.synchronize()
    batch.check(before, 'after the refusals')


# ================================================================================================ embed
def _embed_launch(mode, L, incl, x, dirs, z, per, col0, cuda):
    """The encoding written into columns col0 ... of a NaN-filled matrix with guard rows and EMBED_PAD columns behind it."""
    from nerfactor_amd import ops
    d = (3 if incl else 0) + 6 * L
    rows = (x if mode != 2 else dirs).shape[0] * per
    buf, out = _guarded((rows, col0 + d + C.EMBED_PAD), cuda)
    xd, dd, zd = dev(x, cuda), dev(dirs, cuda), dev(z, cuda)
    if mode == 0:
        ops.embed(L, incl, x=xd, per_ray=per, out=out, col0=col0)
    elif mode == 1:
        ops.embed(L, incl, rayo=xd, rayd=dd, z=zd, out=out, col0=col0)
    elif mode == 2:
        ops.embed(L, incl, rayd=dd, per_ray=per, out=out, col0=col0)
    else:
        ops.embed(L, incl, x=xd, lights=dd, out=out, col0=col0)
    torch.cuda.synchronize()
    _guards_kept(buf, 'embed')
    assert bool(torch.isnan(out[:, :col0]).all()) and bool(torch.isnan(out[:, col0 + d:]).all()), 'written beside its columns'
    assert not bool(torch.isnan(out[:, col0:col0 + d]).any()), 'a slot was never written'
    return host(out[:, col0:col0 + d])


EMBED_IDS = ['mode%d-L%d-in%d-n%d-per%d-col%d' % c for c in C.EMBED_CASES]


@pytest.mark.parametrize("mode,L,incl,n_src,per,col0", C.EMBED_CASES, ids=EMBED_IDS)
def test_embed_is_bit_equal_to_the_restatement(nfx_lib, cuda, mode, L, incl, n_src, per, col0):
    x, dirs, z = C.embed_inputs(mode, n_src, per)
    got = _embed_launch(mode, L, incl, x, dirs, z, per, col0, cuda)
    _assert_bits(got, C.embed(mode, L, incl, x, dirs, z, per), 'embed')
    assert np.abs(got - C.embed_float64(mode, L, incl, x, dirs, z, per)).max() < C.embed_tol(L)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_embed_vector_alone_equals_the_vector_in_the_batch(nfx_lib, cuda, mode):
    n_src, per, L = 13, 7, 10
    x, dirs, z = C.embed_inputs(mode, n_src, per)
    batch = _embed_launch(mode, L, True, x, dirs, z, per, 0, cuda)
    cut = lambda a, r: None if a is None else a[r:r + 1]
    for r in (0, 2, 12):
        one = _embed_launch(mode, L, True, cut(x, r), dirs if mode == 3 else cut(dirs, r), cut(z, r), per, 13, cuda)
        _assert_bits(one, batch[r * per:(r + 1) * per], 'vector %d alone' % r)
    if mode == 3:                                                # one light alone
        one = _embed_launch(3, L, True, x, dirs[3:4], None, 1, 0, cuda)
        _assert_bits(one, batch[3::per], 'light 3 alone')


def _embed_bwd_launch(lib, v, L, incl, d_out, col0, cuda):
    n = v.shape[0]
    vd, dd = dev(v, cuda), dev(d_out, cuda)
    buf, dv = _guarded((n, 3), cuda)
    assert lib.nfx_embed_bwd(vd.data_ptr(), n, L, int(incl), dd.data_ptr(), d_out.shape[1], col0, dv.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _written(buf, 'dv')
    return host(dv)


@pytest.mark.parametrize("L,incl,n,col0", C.EMBED_BWD_CASES, ids=['L%d-in%d-n%d-col%d' % c for c in C.EMBED_BWD_CASES])
def test_embed_bwd_is_bit_equal_to_the_restatement(nfx_lib, cuda, L, incl, n, col0):
    v, d_out = C.embed_bwd_case(L, incl, n, col0)
    got = _embed_bwd_launch(nfx_lib.lib, v, L, incl, d_out, col0, cuda)
    _assert_bits(got, C.embed_bwd(v, L, incl, d_out, col0), 'dv')
    want = C.embed_bwd_float64(v, L, incl, d_out, col0)
    assert np.abs(got - want).max() < C.EMBED_BWD_TOL * np.abs(want).max()
    for r in (0, n - 1):
        one = _embed_bwd_launch(nfx_lib.lib, v[r:r + 1], L, incl, d_out[r:r + 1], col0, cuda)
        _assert_bits(one, got[r:r + 1], 'row %d alone' % r)


def test_embed_refusals_are_error_codes_and_nothing_is_launched(nfx_lib, cuda):
    lib = nfx_lib.lib
    n = 4
    x, out = torch.ones((n, 3), device=cuda), torch.full((n, 40), NAN, device=cuda)
    fwd = lambda n_=n, per=1, mode=0, L=4, incl=1, ld=40, col0=0: lib.nfx_embed(x.data_ptr(), x.data_ptr(), x.data_ptr(), n_, per, mode, L,
                                                                               incl, out.data_ptr(), ld, col0, _stream())
    assert fwd(mode=4) == EINVAL and fwd(mode=-1) == EINVAL and fwd(L=0, incl=0) == EINVAL and fwd(L=17) == EINVAL
    assert fwd(ld=26) == EINVAL and fwd(col0=14) == EINVAL and fwd(col0=-1) == EINVAL and fwd(per=0) == EINVAL and fwd(n_=-1) == EINVAL
    assert lib.nfx_embed(None, None, None, n, 1, 0, 4, 1, out.data_ptr(), 40, 0, _stream()) == EINVAL
    bwd = lambda n_=n, L=4, incl=1, ld=40, col0=0: lib.nfx_embed_bwd(x.data_ptr(), n_, L, incl, out.data_ptr(), ld, col0, out.data_ptr(),
                                                                    _stream())
    assert bwd(L=0, incl=0) == EINVAL and bwd(ld=26) == EINVAL and bwd(col0=14) == EINVAL and bwd(n_=-1) == EINVAL
    assert fwd(n_=0) == 0 and bwd(n_=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
