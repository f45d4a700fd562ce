"""The NeRF point kernels, pinned to their points bit for bit.

Kernels: nerf_mlp_bf16_v6_kernel plain and fold:: (nerf_variant 6, 7, 8), nerf_mlp_bf16_kernel <2, 4> and <1, 8> plain and fold::
(nerf_variant 0, 1), nerf_mlp_x3_kernel (prec = 'fp32'); the density kernels nerf_sigma_v6_kernel and nerf_sigma_geo_kernel
(sigma_variant 1, 0), nerf_sigma_x3_pipe and nerf_sigma_x3_kernel<false> (sigma_x3_variant 1, 0); the density-gradient kernels
nerf_sigma_grad_kernel and nerf_sigma_x3_kernel<true>, over every sample and over the listed ones (sigma_grad_rows 0, 1).
Inputs: tests/nerf_point_cases.py, whose conditions tests/test_cpu_nerf_point_cases.py holds without a GPU.

(A) A point's value is a function of its own origin, direction and depth: a column of an MFMA block does not depend on its
neighbours and every launch runs the same arithmetic in the same order.  So whatever else is in the launch, however the 840
points are cut into rays (ray = m / n_samples: S = 105, 35, 21, 15, 7, 5, 3, 1 put a ray edge on every lane of every wave),
wherever the batch ends, in whatever order the points or the rays come, on however many workgroups and in whichever form of
the kernel: the same bits as the [840, 1] launch on the default grid.
(B) Every point against the oracle at the bounds the suite already has (tests/test_gpu_nerf.py).  (A) cannot see a defect
that is the same at every position; (B) holds those.

Lines that start with PTERR carry the measured worst errors (profiles/nerf_points/errors.txt)."""
import numpy as np
import pytest
import torch

from tests import common, nerf_point_cases as pc
from tests.test_gpu_poisoned_buffers import fresh_memory_holds

pytestmark = pytest.mark.gpu

GRIDS = (None, 1, 3)                      # nerf_blocks: the default (256: one tile per workgroup), one workgroup, three
VARIANTS = (7, 0, 1, 6, 8)
FORM_OPTIONS = ('nerf_variant', 'nerf_fold', 'sigma_variant', 'sigma_x3_variant', 'sigma_grad_rows')


def _form(kind, prec, **opts):
    return (kind, prec, tuple(sorted(opts.items())))


# ops.nerf_mlp_fwd: ten bf16 forms in two bit classes (folded, unfolded) and the fp32-class kernel
MLP_BF16 = [_form('mlp', 'bf16', nerf_variant=v, nerf_fold=f) for f in (1, 0) for v in VARIANTS]
MLP_FP32 = _form('mlp', 'fp32')
MLP_FORMS = MLP_BF16 + [MLP_FP32]
DEFAULT_FORM = _form('mlp', 'bf16', nerf_variant=7, nerf_fold=1)
ALL_POINT_FORMS = (DEFAULT_FORM, MLP_FP32)                        # every point launched alone
SIGMA_FORMS = [_form('sigma', 'bf16', sigma_variant=v) for v in (1, 0)] + [_form('sigma', 'fp32', sigma_x3_variant=v) for v in (1, 0)]
GRAD_FORMS = [_form('grad', p, sigma_grad_rows=r) for p in ('bf16', 'fp32') for r in (1, 0)]
ALL_FORMS = MLP_FORMS + SIGMA_FORMS + GRAD_FORMS
PREFIX_FORMS = [DEFAULT_FORM, _form('mlp', 'bf16', nerf_variant=7, nerf_fold=0), _form('mlp', 'bf16', nerf_variant=1, nerf_fold=1),
                _form('mlp', 'bf16', nerf_variant=0, nerf_fold=0), MLP_FP32] + SIGMA_FORMS + GRAD_FORMS


def form_id(form):
    kind, prec, opts = form
    return '_'.join([kind, prec] + ['%s%d' % (k.split('_')[-1], v) for k, v in opts])


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def on_dev(ps, s, cuda):
    """(rayo, rayd, z) of the layout s on the device"""
    return cached(('layout', ps.name, s), lambda: tuple(dev(a, cuda) for a in ps.layout(s)))


def blob_of(ps, which, prec, cuda):
    from nerfactor_amd import ops
    pack = ops.pack_nerf_weights if which == 'full' else ops.pack_nerf_geom_weights
    return cached(('blob', ps.name, which, prec), lambda: pack(*common.nerf_layers(ps.net), prec=prec).to(cuda))


def options(nfx_opt, **kw):
    for k, v in kw.items():
        if v is None:
            nfx_opt.unset(k)
        else:
            nfx_opt.set(k, v)


def runner(nfx_opt, cuda, ps, form):
    """run(rayo, rayd, z) -> [points, 4] (rgb logits, density | normal, density) or [points, 1] (density) of one form; sets the
    form's options and unsets every other form option"""
    from nerfactor_amd import ops
    kind, prec, opts = form
    options(nfx_opt, **{k: dict(opts).get(k) for k in FORM_OPTIONS})
    blob = blob_of(ps, 'full' if kind == 'mlp' else 'geom', prec, cuda)
    if kind == 'mlp':
        return lambda o, d, z: ops.nerf_mlp_fwd(o, d, z, blob, prec).reshape(-1, 4)
    if kind == 'sigma':
        return lambda o, d, z: ops.nerf_sigma_fwd(o, d, z, blob, prec).reshape(-1, 1)

    def grad(o, d, z):
        normal, sigma = ops.nerf_sigma_grad(o, d, z, blob, prec)
        return torch.cat((normal, sigma[..., None]), -1).reshape(-1, 4)
    return grad


def same(form, want, got, what):
    """bit for bit; of the gradient kernels the density of every row and the normal of the rows with a positive density, the
    other rows' normals as numbers: the every-sample kernel writes g * 0 there with g's sign, the list form -0
    (test_sigma_gradient_over_the_samples_with_a_density_equals_every_sample)"""
    what = '%s: %s' % (form_id(form), what)
    if form[0] != 'grad':
        return common.assert_same_bits(want, got, what)
    common.assert_same_bits(want[:, 3:], got[:, 3:], what + ' (density)')
    on = want[:, 3] > 0
    common.assert_same_bits(want[on], got[on], what + ' (rows with a density)')
    assert torch.equal(want[~on], got[~on]), what + ' (rows without a density, as numbers)'
    assert not bool(got[~on][:, :3].any())


def base_of(nfx_opt, cuda, ps, form):
    """the [840, 1] launch on the default grid: what everything else is compared with"""
    run = runner(nfx_opt, cuda, ps, form)
    options(nfx_opt, nerf_blocks=None)
    base = cached(('base', ps.name, form), lambda: run(*on_dev(ps, 1, cuda)))
    assert base.shape[0] == pc.N and bool(torch.isfinite(base).all())
    return run, base


def alone(run, flat, points):
    """every one of `points` launched alone, put together"""
    o, d, z = flat
    return torch.cat([run(o[i:i + 1], d[i:i + 1], z[i:i + 1]) for i in points])


def index(idx, cuda):
    return torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)


SETS_FORMS = [pytest.param(s, f, id='%s-%s' % (s, form_id(f))) for s in pc.SETS for f in ALL_FORMS]


# ========================================================================================================= (A) identities
@pytest.mark.parametrize('name,form', SETS_FORMS)
def test_a_point_s_value_is_its_own(nfx_lib, cuda, nfx_opt, name, form):
    """Every form: all eight layouts on the default grid, one workgroup and three; chunks cut inside column tiles; points launched
    alone (every point for the default render form and the fp32-class kernel, sampled_points() for the others); the points
    reversed and in a random order, the base rays reversed and in a random order, a random sample order inside every ray."""
    ps = pc.point_set(name)
    run, base = base_of(nfx_opt, cuda, ps, form)
    flat = on_dev(ps, 1, cuda)
    for blocks in GRIDS:
        options(nfx_opt, nerf_blocks=blocks)
        for s in pc.LAYOUTS:
            same(form, base, run(*on_dev(ps, s, cuda)), 'layout [%d, %d], nerf_blocks %s against [840, 1]' % (pc.N // s, s, blocks))
    options(nfx_opt, nerf_blocks=None)
    for a, b in pc.chunks():
        same(form, base[a:b], run(*(t[a:b] for t in flat)), 'points [%d, %d) alone against the batch' % (a, b))
    points = list(range(pc.N)) if form in ALL_POINT_FORMS else pc.sampled_points()
    got = alone(run, flat, points)
    if form[0] == 'grad' or not torch.equal(base[index(np.array(points), cuda)], got):
        for k, i in enumerate(points):           # (one comparison per point: the message names it)
            same(form, base[i:i + 1], got[k:k + 1], 'point %d (lane %d of wave %d of tile %d) alone against the batch' % (
                i, i % pc.WAVE, i % pc.TILE // pc.WAVE, i // pc.TILE))
    rng = np.random.default_rng(11)
    for what, idx in (('reversed', np.arange(pc.N)[::-1]), ('in a random order', rng.permutation(pc.N))):
        ix = index(idx, cuda)
        same(form, base[ix], run(*(t[ix].contiguous() for t in flat)), 'the points %s on [840, 1]' % what)
    for what, order in (('reversed', np.arange(pc.N_RAYS)[::-1]), ('in a random order', rng.permutation(pc.N_RAYS))):
        o, d, z, idx = ps.base_ray_order(order)
        same(form, base[index(idx, cuda)], run(dev(o, cuda), dev(d, cuda), dev(z, cuda)), 'the base rays %s on [8, 105]' % what)
    for s, seed in ((105, 12), (7, 13)):
        o, d, z, idx = ps.sample_order(s, seed)
        same(form, base[index(idx, cuda)], run(dev(o, cuda), dev(d, cuda), dev(z, cuda)), 'a random sample order inside every ray of [%d, %d]' % (pc.N // s, s))


@pytest.mark.parametrize('name,form', [pytest.param(s, f, id='%s-%s' % (s, form_id(f))) for s in pc.SETS for f in PREFIX_FORMS])
def test_where_the_batch_ends_changes_no_point(nfx_lib, cuda, nfx_opt, name, form):
    """Every prefixes() count on [P, 1] and the first 1 .. 8 base rays on [k, 105], on the default grid, one workgroup (it walks
    four 256-point or seven 128-point tiles; the 78- or 70-chunk weight stream of the render kernels wraps three times) and three."""
    ps = pc.point_set(name)
    run, base = base_of(nfx_opt, cuda, ps, form)
    flat, rays = on_dev(ps, 1, cuda), on_dev(ps, 105, cuda)
    for blocks in GRIDS:
        options(nfx_opt, nerf_blocks=blocks)
        for k in pc.prefixes():
            same(form, base[:k], run(*(t[:k] for t in flat)), 'the first %d points on [P, 1], nerf_blocks %s against the batch' % (k, blocks))
        for k in pc.ray_prefixes():
            same(form, base[:k * 105], run(*(t[:k] for t in rays)), 'the first %d base rays on [k, 105], nerf_blocks %s against the batch' % (k, blocks))


@pytest.mark.parametrize('name', pc.SETS)
def test_the_forms_agree_with_each_other(nfx_lib, cuda, nfx_opt, name):
    """All five variants agree within each `fold` setting; the density is the same folded and unfolded, and it is what
    nerf_sigma_fwd gives from the geom blob under both sigma_variants, in every layout; the density of the fp32-class kernel is
    nerf_sigma_fwd(..., 'fp32') under both sigma_x3_variants (nerf_mlp_x3_kernel and nerf_sigma_x3_kernel run x3::tile<16, 0, .>
    over the same 16 k-steps of the same activation pairs against the same fragments: the geom blob's sigma tile is a copy of
    chunk 72 of the full blob, pack_nets.cpp:pack_geom_fragments; both round the encoder's activations with acc_to_pair<true>); the
    gradient kernels' density is nerf_sigma_fwd's and both sigma_grad_rows settings agree."""
    ps = pc.point_set(name)
    bases = {form: base_of(nfx_opt, cuda, ps, form)[1] for form in ALL_FORMS}
    by_fold = {f: bases[_form('mlp', 'bf16', nerf_variant=7, nerf_fold=f)] for f in (1, 0)}
    for form in MLP_BF16:
        same(form, by_fold[dict(form[2])['nerf_fold']], bases[form], 'against variant 7')
    common.assert_same_bits(by_fold[0][:, 3], by_fold[1][:, 3], '%s: density folded against unfolded' % name)
    assert not torch.equal(by_fold[0][:, :3], by_fold[1][:, :3])
    density = {'bf16': by_fold[1][:, 3:], 'fp32': bases[MLP_FP32][:, 3:]}
    for form in SIGMA_FORMS:
        run = runner(nfx_opt, cuda, ps, form)
        for s in pc.LAYOUTS:
            same(form, density[form[1]], run(*on_dev(ps, s, cuda)), 'layout [%d, %d] against the density of nerf_mlp_fwd' % (pc.N // s, s))
    for form in GRAD_FORMS:
        same(form, bases[_form('grad', form[1], sigma_grad_rows=0)], bases[form], 'against sigma_grad_rows 0')
        common.assert_same_bits(density[form[1]], bases[form][:, 3:], '%s: density against nerf_mlp_fwd' % form_id(form))
        on = bases[form][:, 3] > 0
        assert 0.1 * pc.N < int(on.sum()) < 0.9 * pc.N
        norm = bases[form][:, :3].norm(dim=1)
        assert bool((norm[on] - 1).abs().max() < 1e-5) and bool((norm[~on] == 0).all())


@pytest.mark.parametrize('name', pc.SETS)
def test_the_output_does_not_depend_on_what_its_buffer_held(nfx_lib, cuda, nfx_opt, name):
    """nerf_mlp_fwd (folded, unfolded, fp32) and nerf_sigma_fwd (bf16, fp32) at 840 and at 833 points (the last wave holds 8 points
    and one) with fresh memory 0x00 and 0xFF: the same bits as the batch, every element finite."""
    ps = pc.point_set(name)
    flat = on_dev(ps, 1, cuda)
    for form in (DEFAULT_FORM, _form('mlp', 'bf16', nerf_variant=7, nerf_fold=0), MLP_FP32, SIGMA_FORMS[0], SIGMA_FORMS[2]):
        run, base = base_of(nfx_opt, cuda, ps, form)
        for k in (840, 833):
            for byte in (0x00, 0xFF):
                with fresh_memory_holds(byte) as px:
                    got = run(*(t[:k] for t in flat))
                    torch.cuda.synchronize()
                assert px.filled >= 1 and bool(torch.isfinite(got).all())
                same(form, base[:k], got, '%d points, fresh memory 0x%02X against the batch' % (k, byte))


# ============================================================================================================ (B) the oracle
@pytest.mark.parametrize('name,form', SETS_FORMS)
def test_every_point_against_the_oracle(nfx_lib, cuda, nfx_opt, name, form):
    """bf16 forms: < 4e-3 max(1, max |want_q|) of the oracle with the same operand rounding, and (glorot set) < 0.2 of the float32
    oracle (test_nerf_mlp_bf16_vs_oracle); fp32-class forms: < 2e-4 max(1, max |want|) of the float64 oracle
    (test_nerf_mlp_fp32_vs_oracle).  The density forms are held to the same bounds on their one channel.  The fitted set's distance to
    the float32 oracle is printed only: the reference's own bf16 rounding moves it by 0.25 at logits up to 131."""
    ps = pc.point_set(name)
    kind, prec, _ = form
    cols = slice(0, 4) if kind == 'mlp' else slice(3, 4)
    got = base_of(nfx_opt, cuda, ps, form)[1].cpu().numpy()
    got = got if kind != 'grad' else got[:, 3:]
    assert np.isfinite(got).all()
    if prec == 'bf16':
        want_q, want = ps.want('q'), ps.want('f32')
        eq, e = np.abs(got - want_q[:, cols]).max(), np.abs(got - want[:, cols]).max()
        bound = 4e-3 * max(1., np.abs(want_q).max())
        print('PTERR %-6s %-26s vs same-rounding oracle %.3e (bound %.3e)  vs float32 oracle %.3e (%s)  oracle rounding alone %.3e' % (
            name, form_id(form), eq, bound, e, 'bound 0.2' if name == 'glorot' else 'no bound', np.abs(want_q - want)[:, cols].max()))
        assert eq < bound, (name, form_id(form), eq)
        assert name != 'glorot' or e < 0.2, (name, form_id(form), e)
    else:
        want = ps.want('f64')
        e, bound = np.abs(got - want[:, cols]).max(), 2e-4 * max(1., np.abs(want).max())
        print('PTERR %-6s %-26s vs float64 oracle %.3e (bound %.3e)' % (name, form_id(form), e, bound))
        assert e < bound, (name, form_id(form), e)
