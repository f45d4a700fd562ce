"""The shading kernels of csrc/shade.hip (shade_kernel, shade_olat_kernel, shade_bwd_kernel) through nerfactor_amd.ops at
every light count and launch shape they branch on, against the float64 references of tests/shade_cases.py.

  light loop   a lane keeps 8 lights, a pass covers 512: L = 1 ... 2048 on both sides of 64, 512 and 576, with one-hot
               probes / OLAT columns at the lights next to every boundary (a lost or shifted light is the whole value)
  grid stride  shade_kernel caps its grid at 512 workgroups of 8 waves, the OLAT kernel and the backward at 2048: 4096 + 13
               and 16384 + 13 points take the second trip of the loop with the prefetched rows
  rows         lvis_row / out_row into full buffers of 2 n rows in shuffled order; rows nobody owns keep a sentinel
  probe split  ops.shade_fwd splits the probes that do not fit 160 KiB of LDS together

Bound against float64 (shade_cases.bound): 8 x max(d_ref, 1e-6), d_ref = max |fp32 oracle - float64 oracle| over the outputs
where that distance is <= 1e-5 (shade_cases.compared_set; tests/test_cpu_shade_cases.py holds the share of the others below
1 %).  The outputs left out are the ill-conditioned ones the bound of tests/test_gpu_nerfactor.py was made for, and are held
to that bound: 1e-3 against float64.  Every comparison prints `shade_shapes: ...` with the measured ratio
(profiles/shade_shapes/errors.txt).  Identities that involve no rounding (chunked runs, one probe per call, rows against the
compact run) are held with torch.equal.  The backward is held to float64 autograd with the bounds of
tests/test_gpu_train.py::test_shade_backward_vs_autograd, and single columns of d_lvis / d_spec / rows of d_light to 1e-3.
"""
import numpy as np
import pytest
import torch

from tests import shade_cases as S

pytestmark = pytest.mark.gpu

LOOSE = 1e-3            # tests/test_gpu_nerfactor.py::test_shade_microfacet_vs_oracle, against float64
SENTINEL = 0x7FC5A5A5   # a quiet NaN with a payload no kernel produces


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def geometry(c, cuda, sel=slice(None), lvis=None):
    """The positional arguments of ops.shade_fwd / shade_olat_fwd / shade_bwd up to `lareas`."""
    return (dev(c.xyz[sel], cuda), dev(c.cam[sel], cuda), dev(c.normal[sel], cuda), dev(c.albedo[sel], cuda),
            dev(c.lvis[sel], cuda) if lvis is None else lvis, dev(c.lxyz, cuda), dev(c.lareas, cuda))


def brdf(c, kind, cuda, sel=slice(None)):
    if kind == 'microfacet':
        return dict(rough=dev(c.rough[sel], cuda), f0=S.F0)
    return dict(spec=dev(c.spec[sel], cuda), spec_scale=S.SPEC_SCALE)


def shade(c, kind, to_srgb, cuda, probes=None, sel=slice(None), **kw):
    from nerfactor_amd import ops
    probes = c.probes if probes is None else probes
    return ops.shade_fwd(*geometry(c, cuda, sel, kw.pop('lvis', None)), dev(probes, cuda), linear2srgb=to_srgb,
                         **brdf(c, kind, cuda, sel), **kw)


def olat(c, kind, ambient, to_srgb, cuda, sel=slice(None), **kw):
    from nerfactor_amd import ops
    return ops.shade_olat_fwd(*geometry(c, cuda, sel, kw.pop('lvis', None)), c.olat_inten, ambient, linear2srgb=to_srgb,
                              **brdf(c, kind, cuda, sel), **kw)


def hold(got, ref32, ref64, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    mask, d_ref, left_out = S.compared_set(ref32, ref64)
    err = np.abs(got - ref64)
    tight, loose = float(err[mask].max()), float(err[~mask].max()) if (~mask).any() else 0.
    tol = S.bound(d_ref)
    print('shade_shapes: %-58s err %.2e  d_ref %.2e  err/max(d_ref,1e-6) %5.2f  (bound 8)  left out %d of %d, err there %.1e'
          % (what, tight, d_ref, tight / max(d_ref, S.BOUND_FLOOR), int((~mask).sum()), mask.size, loose))
    assert np.isfinite(got).all(), what
    assert tight <= tol, (what, tight, tol)
    assert loose <= LOOSE, (what, loose)


def hold_fwd(got, c, kind, to_srgb, what, probes=None):
    hold(got, S.forward_ref(c, kind, to_srgb, np.float32, probes), S.forward_ref(c, kind, to_srgb, np.float64, probes),
         '%s %r %s srgb=%d' % (what, c, kind, to_srgb))


def hold_olat(got, c, kind, ambient, to_srgb, what):
    hold(got, S.olat_ref(c, kind, ambient, to_srgb, np.float32), S.olat_ref(c, kind, ambient, to_srgb),
         '%s %r %s srgb=%d ambient=%g' % (what, c, kind, to_srgb, ambient))


# --------------------------------------------------------------------------------------------------- light counts
@pytest.mark.parametrize("to_srgb", [True, False])
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("L", S.FWD_LIGHTS)
def test_shade_fwd_at_every_light_count(nfx_lib, cuda, L, kind, to_srgb):
    c = S.case(L, S.N_SMALL)
    hold_fwd(shade(c, kind, to_srgb, cuda), c, kind, to_srgb, 'fwd')


@pytest.mark.parametrize("ambient", S.OLAT_AMBIENTS)
@pytest.mark.parametrize("kind,to_srgb", S.OLAT_COMBOS)
@pytest.mark.parametrize("L", S.FWD_LIGHTS)
def test_shade_olat_fwd_at_every_light_count(nfx_lib, cuda, L, kind, to_srgb, ambient):
    c = S.case(L, S.N_SMALL)
    hold_olat(olat(c, kind, ambient, to_srgb, cuda), c, kind, ambient, to_srgb, 'olat')


# --------------------------------------------------------------------------------------------------- point counts
@pytest.mark.parametrize("n", S.SMALL_NS)
def test_fewer_points_than_a_workgroup_and_one_more(nfx_lib, cuda, n):
    c = S.case(65, n)
    for kind in S.KINDS:
        hold_fwd(shade(c, kind, True, cuda), c, kind, True, 'fwd')
    for kind, to_srgb in S.OLAT_COMBOS:
        hold_olat(olat(c, kind, 0.05, to_srgb, cuda), c, kind, 0.05, to_srgb, 'olat')


def chunks(n, size):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


@pytest.mark.parametrize("kind", S.KINDS)
def test_shade_fwd_grid_stride_loop(nfx_lib, cuda, kind):
    """4096 + 13 points: 13 waves take a second point, whose rows they prefetched while shading the first.  The run equals
    (bit for bit) the runs over chunks in which every wave shades one point."""
    c = S.case(S.L_STRIDE_FWD, S.N_STRIDE_FWD)
    assert c.probes.shape[0] == 2
    got = shade(c, kind, True, cuda)
    hold_fwd(got, c, kind, True, 'fwd grid-stride')
    for size in (4096, 1500):
        assert torch.equal(got, torch.cat([shade(c, kind, True, cuda, sel=s) for s in chunks(c.n, size)])), size


@pytest.mark.parametrize("kind,to_srgb", S.OLAT_COMBOS[:2])
def test_shade_olat_fwd_grid_stride_loop(nfx_lib, cuda, kind, to_srgb):
    c = S.case(S.L_STRIDE_BIG, S.N_STRIDE_BIG)
    got = olat(c, kind, 0.05, to_srgb, cuda)
    hold_olat(got, c, kind, 0.05, to_srgb, 'olat grid-stride')
    for size in (16384, 6000):
        assert torch.equal(got, torch.cat([olat(c, kind, 0.05, to_srgb, cuda, sel=s) for s in chunks(c.n, size)])), size


# ------------------------------------------------------------------------------------------------------------ rows
def shuffled_rows(c, cuda, seed):
    """(row [n] int32 into a buffer of 2 n rows, in shuffled order; lvis [2 n, L] with NaN in the rows nobody owns)."""
    row = np.random.default_rng(seed).permutation(2 * c.n)[:c.n].astype(np.int32)
    full = np.full((2 * c.n, c.L), np.nan, np.float32)
    full[row] = c.lvis
    return torch.from_numpy(row).to(cuda), dev(full, cuda)


@pytest.mark.parametrize("kind", S.KINDS)
def test_shade_fwd_reads_its_visibilities_through_lvis_row(nfx_lib, cuda, kind):
    """L = 577: the lights of the second pass re-read `lvis` through lvis_row (light_transport); the first 512 come from the
    prefetch.  Any other row of the full buffer holds NaN, which the front-lit mask lets through."""
    c = S.case(S.L_ROWS, S.N_SMALL)
    row, full = shuffled_rows(c, cuda, 1)
    compact = shade(c, kind, True, cuda)
    hold_fwd(compact, c, kind, True, 'fwd (compact run of the rows test)')
    assert torch.equal(shade(c, kind, True, cuda, lvis=full, lvis_row=row), compact)


@pytest.mark.parametrize("kind,to_srgb", S.OLAT_COMBOS[:2])
def test_shade_olat_fwd_rows_in_and_out(nfx_lib, cuda, kind, to_srgb):
    c = S.case(S.L_ROWS, S.N_SMALL)
    row, full = shuffled_rows(c, cuda, 2)
    out_row = torch.from_numpy(np.random.default_rng(3).permutation(2 * c.n)[:c.n].astype(np.int32)).to(cuda)
    compact = olat(c, kind, 0.05, to_srgb, cuda)
    hold_olat(compact, c, kind, 0.05, to_srgb, 'olat (compact run of the rows test)')
    assert torch.equal(olat(c, kind, 0.05, to_srgb, cuda, lvis=full, lvis_row=row), compact)
    out = torch.full((2 * c.n, c.L, 3), SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)
    back = olat(c, kind, 0.05, to_srgb, cuda, lvis=full, lvis_row=row, out=out, out_row=out_row)
    assert back.data_ptr() == out.data_ptr()
    assert torch.equal(out[out_row.long()], compact)
    free = torch.ones(2 * c.n, dtype=torch.bool, device=cuda)
    free[out_row.long()] = False
    assert int(free.sum()) == c.n and bool((out.view(torch.int32)[free] == SENTINEL).all())


def test_shade_olat_fwd_nan_flag(nfx_lib, cuda):
    """A NaN visibility of a front-lit light is a NaN radiance before the clip (which drops it): the flag says so."""
    c = S.case(S.L_ROWS, S.N_SMALL)
    cos = S.light_cosines(c)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    clean = olat(c, 'microfacet', 0., True, cuda, nan_flag=flag)
    assert int(flag.item()) == 0
    for light in (3, 520):      # the lights kept in registers | the tail loop past 512
        lvis = c.lvis.copy()
        pt = int(np.argmax(cos[:, light]))
        lvis[pt, light] = np.nan
        flag.zero_()
        got = olat(c, 'microfacet', 0., True, cuda, lvis=dev(lvis, cuda), nan_flag=flag)
        assert int(flag.item()) == 1, light
        assert bool(torch.isfinite(got).all())
        others = torch.arange(c.n, device=cuda) != pt
        assert torch.equal(got[others], clean[others]), light
        # the same NaN behind the front-lit mask is no radiance at all
        lvis = c.lvis.copy()
        lvis[int(np.argmin(cos[:, light])), light] = np.nan
        flag.zero_()
        assert torch.equal(olat(c, 'microfacet', 0., True, cuda, lvis=dev(lvis, cuda), nan_flag=flag), clean)
        assert int(flag.item()) == 0, light


# ---------------------------------------------------------------------------------------------------------- probes
@pytest.mark.parametrize("kind", S.KINDS)
def test_probes_of_one_call_equal_one_call_per_probe(nfx_lib, cuda, kind):
    c = S.case(S.L_ROWS, S.N_SMALL)
    got = shade(c, kind, True, cuda)
    for p in range(c.probes.shape[0]):
        assert torch.equal(got[:, p:p + 1], shade(c, kind, True, cuda, probes=c.probes[p:p + 1])), p


def test_ops_shade_fwd_splits_probes_that_do_not_fit_the_lds(nfx_lib, cuda):
    """2048 lights x 6 probes need 180 800 B of LDS: ops.shade_fwd runs 5 probes (156 128 B) and then 1."""
    from nerfactor_amd.ops import lib
    assert lib.nfx_shade_lds_bytes(2048, 6) == 180800 > 160 * 1024 >= lib.nfx_shade_lds_bytes(2048, 5) == 156128
    c = S.case(2048, S.N_SMALL)
    probes = c.probes[[0, 1, 2, 5, 8, 9]]       # natural, natural, one-hot at 0, 511, 576, 2047
    got = shade(c, 'microfacet', True, cuda, probes=probes)
    hold_fwd(got, c, 'microfacet', True, 'fwd 6 probes (split 5 + 1)', probes=probes)
    for p in range(6):
        assert torch.equal(got[:, p:p + 1], shade(c, 'microfacet', True, cuda, probes=probes[p:p + 1])), p


# -------------------------------------------------------------------------------------------------------- backward
def backward(c, kind, to_srgb, cuda, sel=slice(None), d_light=None):
    from nerfactor_amd import ops
    return ops.shade_bwd(*geometry(c, cuda, sel), dev(c.light, cuda), dev(c.drgb[sel], cuda), d_light, linear2srgb=to_srgb,
                         **brdf(c, kind, cuda, sel))


def hold_backward(c, kind, to_srgb, cuda, what):
    ref = S.backward_ref(c, kind, to_srgb)
    inside = ref['inside']
    assert inside.mean() >= 0.5
    d_light = torch.zeros(c.L, 3, device=cuda)
    got = backward(c, kind, to_srgb, cuda, d_light=d_light)
    front = S.front_lit(c)

    def rel(g, w, rows=inside):
        g, w = g.double().cpu().numpy()[rows], w[rows]
        return float(np.linalg.norm(g - w) / (np.linalg.norm(w) + 1e-30))
    e = {'d_albedo': rel(got[0], ref['d_albedo']), 'd_normal': rel(got[1], ref['d_normal']),
         'd_lvis': rel(got[2], ref['d_lvis']), ('d_rough' if kind == 'microfacet' else 'd_spec'): rel(got[3], ref['d_param'])}
    # d light: summed over the points inside the clip range only -> a second call with those points
    idx = np.nonzero(inside)[0]
    d_light2 = torch.zeros(c.L, 3, device=cuda)
    backward(c, kind, to_srgb, cuda, sel=idx, d_light=d_light2)
    e['d_light'] = rel(d_light2, ref['d_light_inside'], slice(None))
    # single lights: a lost or shifted light is a relative error of 1 there, not of 1 / L
    cols = {}
    for l in S.bwd_columns(c.L):
        rows = inside & front[:, l]
        cols[l] = [rel(got[2][:, l], ref['d_lvis'][:, l], rows), rel(d_light2[l], ref['d_light_inside'][l], slice(None))]
        if kind == 'spec':
            cols[l].append(rel(got[3][:, l], ref['d_param'][:, l], rows))
        assert rows.any() and bool((got[2][:, l].cpu().numpy()[~front[:, l]] == 0).all())
    print('shade_shapes: %-40s rel. Frobenius %s | worst single column d_lvis %.1e d_light %.1e%s'
          % ('%s %r %s srgb=%d' % (what, c, kind, to_srgb), ' '.join('%s %.1e' % kv for kv in e.items()),
             max(v[0] for v in cols.values()), max(v[1] for v in cols.values()),
             ' d_spec %.1e' % max(v[2] for v in cols.values()) if kind == 'spec' else ''))
    for name, v in e.items():
        assert v <= (2e-2 if name in ('d_rough', 'd_normal') else 1e-3), (what, name, v)
    for l, v in cols.items():
        assert max(v) <= 1e-3, (what, l, v)
    return got


@pytest.mark.parametrize("to_srgb", [True, False])
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("L", S.BWD_LIGHTS)
def test_shade_bwd_at_every_light_count(nfx_lib, cuda, L, kind, to_srgb):
    hold_backward(S.case(L, S.N_SMALL), kind, to_srgb, cuda, 'bwd')


@pytest.mark.parametrize("kind", S.KINDS)
def test_shade_bwd_grid_stride_loop(nfx_lib, cuda, kind):
    c = S.case(S.L_STRIDE_BIG, S.N_STRIDE_BIG)
    got = hold_backward(c, kind, True, cuda, 'bwd grid-stride')
    parts = [backward(c, kind, True, cuda, sel=s) for s in chunks(c.n, 16384)]
    for i, g in enumerate(got):
        assert torch.equal(g, torch.cat([p[i] for p in parts])), i


@pytest.mark.parametrize("kind", S.KINDS)
def test_shade_bwd_adds_to_d_light(nfx_lib, cuda, kind):
    """d_light accumulates: the fixed-point sum is converted once and added, so a pre-filled d_light ends as the float sum
    of the pre-fill and the gradient of a call into zeros — exactly, the sum being order-independent."""
    c = S.case(S.L_ROWS, S.N_SMALL)
    grad = torch.zeros(c.L, 3, device=cuda)
    backward(c, kind, True, cuda, d_light=grad)
    assert float(grad.abs().max()) > 0
    pre = dev(np.random.default_rng(4).normal(size=(c.L, 3)), cuda)
    acc = pre.clone()
    backward(c, kind, True, cuda, d_light=acc)
    assert torch.equal(acc, pre + grad)


# -------------------------------------------------------------------------------------------------------- refusals
def zeros_call(cuda, L, n=4):
    z = lambda *s: torch.zeros(s, device=cuda)
    return (z(n, 3), z(n, 3), z(n, 3), z(n, 3), z(n, L), z(L, 3), z(L))


def test_light_counts_past_the_lds_are_refused_by_the_argument_checks(nfx_lib, cuda):
    from nerfactor_amd import ops
    with pytest.raises(nfx_lib.NfxError, match=r"8192 lights do not fit"):
        ops.shade_fwd(*zeros_call(cuda, 8192), torch.zeros(1, 8192, 3, device=cuda), rough=torch.zeros(4, device=cuda))
    with pytest.raises(nfx_lib.NfxError, match=r"too many lights \(10241\)"):      # 16 bytes of LDS per light: 10240 fit
        ops.shade_olat_fwd(*zeros_call(cuda, 10241), 1., 0., rough=torch.zeros(4, device=cuda))
    torch.cuda.synchronize()


def test_shade_bwd_counts_the_light_gradient_in_its_lds_check(nfx_lib, cuda):
    """28 bytes of LDS per light, 52 with a light gradient: 4608 lights (light_h = 48) fit without d_light and not with it.
    The refusal is the argument check's, naming the lights — not a HIP error out of the launcher."""
    c = S.case(4608, 9)
    with pytest.raises(nfx_lib.NfxError, match=r"too many lights \(4608\)"):
        backward(c, 'microfacet', True, cuda, d_light=torch.zeros(c.L, 3, device=cuda))
    torch.cuda.synchronize()          # nothing was launched, nothing is pending
    ref = S.backward_ref(c, 'microfacet', True)
    inside = ref['inside']
    assert inside.any()
    got = backward(c, 'microfacet', True, cuda)
    for g, w in ((got[0], ref['d_albedo']), (got[2], ref['d_lvis'])):
        g, w = g.double().cpu().numpy()[inside], w[inside]
        assert np.linalg.norm(g - w) <= 1e-3 * np.linalg.norm(w)
