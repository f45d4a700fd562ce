"""The ray-march kernels of csrc/raymarch.hip (gen_z, l2_normalize3, composite, composite_bwd, sample_fine) at the shape edges
of tests/raymarch_cases.py: a partly filled last 64-sample chunk behind the running product's carry, S = 1 and 2, the
large-LDS backward launch above S = 2048, ray counts that leave waves of the last workgroup idle, both sides of every
64-bin segment of sample_fine and the limits of its API.

Tolerances: each is the figure of a test the project already has (raymarch_cases.TOL_*), or bit equality; tests/
test_cpu_raymarch_cases.py shows that each leaves the reference alone a factor of two.  Why the bit equalities must hold:
  * sample_fine, gen_z: raymarch.hip is compiled with -ffp-contract=off and IEEE division (it is not in build.py's FAST_DIV
    list), every expression is written in the oracle's order, both running sums of sample_fine are sequential in the oracle's
    order, and the oracle sorts values (the kernel scatters them by rank);
  * disp: one IEEE division of the kernel's own depth;
  * a ray alone against the same ray in a batch, want_weights on / off, surface_kernel against composite_kernel: the same
    instructions on the same numbers.
Outputs are allocated by ops.py with torch.empty: the tests that look for slots never written (or written outside the
output) call the C-ABI on a slice of a NaN-filled tensor with a guard row on each side.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import raymarch_cases as C

pytestmark = pytest.mark.gpu

ids2 = lambda cases: ['n%d-S%d' % c for c in cases]
ids3 = lambda cases: ['n%d-nc%d-nf%d' % c for c in cases]
FWD_COMBOS = ((True, False), (False, True))       # (white_bg, use_noise): white without noise, black with
NAMES = ('rgb', 'occu', 'depth', 'disp', 'weights')


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(cuda)     # (a copy: the cases are read-only)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, row_shape, cuda):
    """(buffer [n + 2, *row_shape] full of NaN, its rows 1 .. n as the output the kernel gets)."""
    buf = torch.full((n + 2,) + tuple(row_shape), float('nan'), dtype=torch.float32, device=cuda)
    return buf, buf[1:n + 1]


def _check_guards(buf, what):
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), what + ': written outside the output'
    assert not bool(torch.isnan(buf[1:-1]).any()), what + ': a slot was never written'


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _composite(case, white_bg, use_noise, cuda, want_weights=True, rows=slice(None)):
    from nerfactor_amd import ops
    rgbs, z, rayd, noise, _ = C.edge_rays(*case)
    return ops.composite_fwd(dev(rgbs[rows], cuda), dev(z[rows], cuda), dev(rayd[rows], cuda), white_bg=white_bg,
                             noise=dev(noise[rows], cuda) if use_noise else None, want_weights=want_weights)


def _composite_bwd(case, white_bg, use_noise, cuda, rows=slice(None)):
    from nerfactor_amd import ops
    rgbs, z, rayd, noise, g = C.edge_rays(*case)
    return ops.composite_bwd(dev(rgbs[rows], cuda), dev(z[rows], cuda), dev(rayd[rows], cuda), dev(g[rows], cuda),
                             white_bg=white_bg, noise=dev(noise[rows], cuda) if use_noise else None)


def _float64_forward(case, white_bg, use_noise):
    rgbs, z, rayd, noise, _ = C.edge_rays(*case)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    return [v.numpy() for v in C.torch_composite_all(t(rgbs), t(z), t(rayd), white_bg, t(noise) if use_noise else None)]


def _disp_of(depth):
    """1 / clamp(depth, min=1e-10) in float32 on the host: one IEEE division."""
    return torch.tensor(1., dtype=torch.float32) / torch.clamp(depth.cpu(), min=1e-10)


# ================================================================================================ sample_fine
def _fine_u(n, nf, seed):
    return np.random.default_rng(seed).uniform(size=(n, nf)).astype(np.float32)


@pytest.mark.parametrize("n,nc,nf", C.FINE_CASES, ids=ids3(C.FINE_CASES))
def test_sample_fine_is_bit_equal_to_the_oracle(nfx_lib, cuda, n, nc, nf):
    from nerfactor_amd import ops
    z, w = C.fine_cases(nc, nf, n=n)
    for u in (None, _fine_u(n, nf, nc + nf)):
        got = ops.sample_fine(dev(z, cuda), dev(w, cuda), nf, u=dev(u, cuda)).cpu().numpy()
        want = nerf_ref.gen_z_fine(z, w, nf, u=u)
        assert got.shape == (n, nc + nf)
        differ = np.argwhere(got != want)
        assert np.array_equal(got, want), ('u given' if u is not None else 'u = None', len(differ), differ[:4].tolist(),
                                           float(np.abs(got - want).max()))


@pytest.mark.parametrize("n,nc,nf", C.FINE_CASES, ids=ids3(C.FINE_CASES))
def test_sample_fine_ranking_paths_agree(nfx_lib, cuda, n, nc, nf):
    """u = None ranks by two binary searches in two sorted lists, a given u by all pairs: given the u that u = None stands
    for, the two must return the same bits on every ray, the tie-heavy ones included."""
    from nerfactor_amd import ops
    z, w = C.fine_cases(nc, nf, n=n)
    by_lists = ops.sample_fine(dev(z, cuda), dev(w, cuda), nf)
    by_pairs = ops.sample_fine(dev(z, cuda), dev(w, cuda), nf, u=dev(C.linspace_u(n, nf), cuda))
    assert _same_bits(by_lists, by_pairs), torch.nonzero(by_lists != by_pairs)[:4].tolist()


def test_sample_fine_at_chosen_u(nfx_lib, cuda):
    """u on the cdf entries of a ray with four equal bins, one float to either side of them, 0 and the float below 1: the
    oracle's `<=` search decides the bin."""
    from nerfactor_amd import ops
    z, w, u, row = C.chosen_u_case()
    got = ops.sample_fine(dev(z, cuda), dev(w, cuda), u.shape[1], u=dev(u, cuda)).cpu().numpy()
    want = nerf_ref.gen_z_fine(z, w, u.shape[1], u=u)
    assert np.array_equal(got[row], want[row]), (got[row], want[row])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,nc,nf", C.FINE_CASES, ids=ids3(C.FINE_CASES))
def test_sample_fine_writes_every_slot_once_and_nothing_else(nfx_lib, cuda, n, nc, nf):
    z, w = C.fine_cases(nc, nf, n=n)
    zd, wd = dev(z, cuda), dev(w, cuda)
    for u in (None, _fine_u(n, nf, 7 + nc)):
        ud = dev(u, cuda)
        buf, out = _guarded(n, (nc + nf,), cuda)
        nfx_lib.check(nfx_lib.lib.nfx_sample_fine(zd.data_ptr(), wd.data_ptr(), n, nc, nf, _ptr(ud), out.data_ptr(), _stream()),
                      'nfx_sample_fine')
        torch.cuda.synchronize()
        _check_guards(buf, 'z_all')
        got = out.cpu().numpy()
        assert np.all(np.diff(got, axis=1) >= 0)
        both = np.concatenate((z, C.fine_samples(z, w, nf, u=u)), 1)
        assert np.array_equal(got, np.sort(both, 1))          # a permutation of concat(z, z_fine): sorted rows compare as sets


@pytest.mark.parametrize("nc,nf", C.FINE_SHAPES, ids=['nc%d-nf%d' % c for c in C.FINE_SHAPES])
def test_sample_fine_rays_do_not_see_each_other(nfx_lib, cuda, nc, nf):
    from nerfactor_amd import ops
    n = C.N_ALL
    z, w = C.fine_cases(nc, nf)
    zd, wd = dev(z, cuda), dev(w, cuda)
    for u in (None, _fine_u(n, nf, 9 + nc)):
        ud = dev(u, cuda)
        batch = ops.sample_fine(zd, wd, nf, u=ud)
        for r in range(n):
            alone = ops.sample_fine(zd[r:r + 1], wd[r:r + 1], nf, u=None if ud is None else ud[r:r + 1])
            assert _same_bits(alone[0], batch[r]), (r, u is not None)


def test_sample_fine_refuses_bad_shapes(nfx_lib, cuda):
    from nerfactor_amd import ops
    mk = lambda nc: (torch.linspace(2., 6., nc, device=cuda).repeat(3, 1), torch.ones((3, nc), device=cuda))
    for nc, nf in ((2, 8), (259, 8), (16, 1), (258, 3400)):       # (258, 3400): 16 (3 nc - 2 + nf) bytes of LDS > 64 KiB
        with pytest.raises(nfx_lib.NfxError):
            ops.sample_fine(*mk(nc), nf)
    assert ops.sample_fine(*mk(258), 320).shape == (3, 578)


# ================================================================================================ composite_fwd
@pytest.mark.parametrize("n,s", C.COMPOSITE_CASES, ids=ids2(C.COMPOSITE_CASES))
def test_composite_at_the_shape_edges_vs_oracle(nfx_lib, cuda, n, s):
    """Against nerf_ref.accumulate in float32; S = 1, where the oracle's dist[:, :1] is empty, against the float64 torch
    formula.  disp is one IEEE division of the kernel's own depth."""
    rgbs, z, rayd, noise, _ = C.edge_rays(n, s)
    for white_bg, use_noise in FWD_COMBOS:
        got = _composite((n, s), white_bg, use_noise, cuda)
        if s >= 2:
            rgb, occu, depth, _, w = nerf_ref.accumulate(rgbs, z, rayd, white_bg=white_bg, noise=noise if use_noise else None)
        else:
            rgb, occu, depth, w = _float64_forward((n, s), white_bg, use_noise)
        want = dict(rgb=rgb, occu=occu, depth=depth, weights=w)
        for name, g in zip(NAMES, got):
            assert bool(torch.isfinite(g).all()), name
            if name == 'disp':
                assert _same_bits(g.cpu(), _disp_of(got[2])), 'disp'
                continue
            assert g.shape == want[name].shape, name
            err = float(np.abs(g.cpu().numpy().astype(np.float64) - want[name]).max())
            print('n %d S %d white %d noise %d: %s off by %.2e' % (n, s, white_bg, use_noise, name, err))
            assert err <= (C.TOL_DEPTH if name == 'depth' else C.TOL_FWD), (name, white_bg, use_noise, err)


EXACT_CASES = tuple(c for c in C.COMPOSITE_CASES if C.edge_rows(*c))


@pytest.mark.parametrize("n,s", EXACT_CASES, ids=ids2(EXACT_CASES))
def test_composite_exact_values_of_empty_and_opaque_rays(nfx_lib, cuda, n, s):
    rows = C.edge_rows(n, s)
    for white_bg in (True, False):
        rgb, occu, depth, disp, w = (t.cpu().numpy() for t in _composite((n, s), white_bg, False, cuda))
        for name in ('empty', 'zero', 'negzero'):
            if name not in rows:
                continue
            r = rows[name]
            assert occu[r] == 0 and depth[r] == 0 and np.all(w[r] == 0), (name, occu[r], depth[r])
            assert disp[r] == np.float32(1e10) and np.all(rgb[r] == (1. if white_bg else 0.)), (name, disp[r], rgb[r])
        if 'opaque_first' in rows:
            assert abs(float(w[rows['opaque_first'], 0]) - 1.) <= 1e-6


@pytest.mark.parametrize("n,s", C.COMPOSITE_CASES, ids=ids2(C.COMPOSITE_CASES))
def test_composite_without_the_weights_gives_the_same_bits(nfx_lib, cuda, n, s):
    for white_bg, use_noise in FWD_COMBOS:
        full = _composite((n, s), white_bg, use_noise, cuda)
        lean = _composite((n, s), white_bg, use_noise, cuda, want_weights=False)
        assert lean[4] is None
        for name, a, b in zip(NAMES[:4], full, lean):
            assert _same_bits(a, b), name


@pytest.mark.parametrize("s", C.COMPOSITE_S)
def test_composite_rays_do_not_see_each_other(nfx_lib, cuda, s):
    n = C.N_ALL
    for white_bg, use_noise in FWD_COMBOS:
        batch = _composite((n, s), white_bg, use_noise, cuda)
        for r in range(n):
            alone = _composite((n, s), white_bg, use_noise, cuda, rows=slice(r, r + 1))
            for name, a, b in zip(NAMES, alone, batch):
                assert _same_bits(a[0], b[r]), (name, r)


@pytest.mark.parametrize("s", [1, 65, 257])
def test_composite_and_surface_kernel_share_their_scan(nfx_lib, cuda, s):
    """surface_kernel was copied from composite_kernel's scan: on the same densities, depths and (unit) directions its
    occupancy and expected depth are composite's, bit for bit."""
    from nerfactor_amd import ops
    n = C.N_ALL
    rgbs, z, rayd, _, _ = C.edge_rays(n, s)
    unit = nerf_ref.l2_normalize(rayd, 1, 1e-12)
    rayo = np.random.default_rng(s).uniform(-1, 1, size=(n, 3)).astype(np.float32)
    _, occu, depth, _, _ = ops.composite_fwd(dev(rgbs, cuda), dev(z, cuda), dev(unit, cuda), white_bg=True)
    _, _, s_depth, s_occu = ops.nerf_surface(dev(rgbs[..., 3], cuda), dev(z, cuda), dev(rayo, cuda), dev(unit, cuda),
                                             want_occu=True)
    assert _same_bits(s_occu, occu) and _same_bits(s_depth, depth)
    assert float(occu.max()) > 0.5


@pytest.mark.parametrize("n,s", C.COMPOSITE_CASES, ids=ids2(C.COMPOSITE_CASES))
def test_composite_writes_every_slot_and_nothing_else(nfx_lib, cuda, n, s):
    rgbs, z, rayd, noise, _ = (dev(a, cuda) for a in C.edge_rays(n, s))
    for want_weights in (True, False):
        bufs = [_guarded(n, shp, cuda) for shp in ((3,), (), (), (), (s,))]
        outs = [o for _, o in bufs]
        nfx_lib.check(nfx_lib.lib.nfx_composite_fwd(rgbs.data_ptr(), z.data_ptr(), rayd.data_ptr(), noise.data_ptr(), n, s, 0,
                                                    outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                    outs[3].data_ptr(), outs[4].data_ptr() if want_weights else None,
                                                    _stream()), 'nfx_composite_fwd')
        torch.cuda.synchronize()
        for name, (buf, _) in zip(NAMES, bufs):
            if name == 'weights' and not want_weights:
                assert bool(torch.isnan(buf).all())
            else:
                _check_guards(buf, name)
        ref = _composite((n, s), False, True, cuda)
        for name, a, b in zip(NAMES[:4 + want_weights], outs, ref):
            assert _same_bits(a, b), name


# ================================================================================================ composite_bwd
@pytest.mark.parametrize("n,s", C.BWD_CASES, ids=ids2(C.BWD_CASES))
def test_composite_backward_at_the_shape_edges_vs_autograd(nfx_lib, cuda, n, s):
    """Against float64 autograd, with and without noise, on both backgrounds; the gradient is exactly zero where the formula
    says so: the density of a sample with sigma + noise <= 0, the colours of an empty ray.  S > 2048 takes the launch with
    more than 64 KiB of LDS."""
    rgbs, z, rayd, noise, _ = C.edge_rays(n, s)
    rows = C.edge_rows(n, s)
    for white_bg, use_noise in C.BWD_COMBOS:
        got = _composite_bwd((n, s), white_bg, use_noise, cuda).cpu().numpy()
        want = C.backward_ref(n, s, white_bg, use_noise)[0]
        assert got.shape == (n, s, 4) and np.isfinite(got).all()
        print('n %d S %d white %d noise %d: error / tolerance %.3f' % (n, s, white_bg, use_noise, C.bwd_error_ratio(got, want)))
        np.testing.assert_allclose(got, want, rtol=C.BWD_RTOL, atol=C.BWD_ATOL * np.abs(want).max())
        sg = rgbs[..., 3] + noise if use_noise else rgbs[..., 3]          # in float32, as the kernel adds them
        assert np.all(got[..., 3][sg <= 0] == 0)
        if not use_noise:
            for name in ('empty', 'zero', 'negzero'):
                if name in rows:
                    assert np.all(got[rows[name]] == 0), name


@pytest.mark.parametrize("n,s", C.COMPOSITE_CASES, ids=ids2(C.COMPOSITE_CASES))
def test_composite_backward_recomputes_the_forward_kernel_s_forward(nfx_lib, cuda, n, s):
    """As tests/test_gpu_train.py::test_composite_backward_vs_autograd asserts it: the forward kernel's colour against the
    float64 output the backward reference was differentiated from (raymarch_cases.forward_compared_rays: which rays, and
    why not all of them at S >= 200)."""
    for white_bg, use_noise in C.BWD_COMBOS:
        rgb = _composite((n, s), white_bg, use_noise, cuda)[0].cpu().numpy()
        rays = C.forward_compared_rays(n, s, white_bg, use_noise)
        assert rays.sum() >= n - 3
        np.testing.assert_allclose(rgb[rays], C.backward_ref(n, s, white_bg, use_noise)[1][rays], atol=C.TOL_FWD)


BWD_ALONE = tuple(c for c in C.BWD_CASES if 2 <= c[0] <= C.N_ALL)


@pytest.mark.parametrize("n,s", BWD_ALONE, ids=ids2(BWD_ALONE))
def test_composite_backward_rays_do_not_see_each_other(nfx_lib, cuda, n, s):
    for white_bg, use_noise in FWD_COMBOS:
        batch = _composite_bwd((n, s), white_bg, use_noise, cuda)
        for r in range(n):
            alone = _composite_bwd((n, s), white_bg, use_noise, cuda, rows=slice(r, r + 1))
            assert _same_bits(alone[0], batch[r]), r


@pytest.mark.parametrize("n,s", C.BWD_CASES, ids=ids2(C.BWD_CASES))
def test_composite_backward_writes_every_slot_and_nothing_else(nfx_lib, cuda, n, s):
    rgbs, z, rayd, noise, g = (dev(a, cuda) for a in C.edge_rays(n, s))
    buf, out = _guarded(n, (s, 4), cuda)
    nfx_lib.check(nfx_lib.lib.nfx_composite_bwd(rgbs.data_ptr(), z.data_ptr(), rayd.data_ptr(), noise.data_ptr(), n, s, 1,
                                                g.data_ptr(), out.data_ptr(), _stream()), 'nfx_composite_bwd')
    torch.cuda.synchronize()
    _check_guards(buf, 'd_rgbs')
    assert _same_bits(out, _composite_bwd((n, s), True, True, cuda))


def test_composite_backward_refuses_more_than_4096_samples(nfx_lib, cuda):
    from nerfactor_amd import ops
    n, s = 2, 4097
    z = torch.linspace(2., 6., s, device=cuda).repeat(n, 1)
    with pytest.raises(nfx_lib.NfxError):
        ops.composite_bwd(torch.zeros((n, s, 4), device=cuda), z, torch.ones((n, 3), device=cuda), torch.ones((n, 3), device=cuda))


# ================================================================================================ gen_z, l2_normalize3
@pytest.mark.parametrize("lin_in_disp", [False, True])
@pytest.mark.parametrize("n_samples", [2, 3, 64, 65])
def test_gen_z_is_bit_equal_to_the_oracle(nfx_lib, cuda, n_samples, lin_in_disp):
    """z_of_t, the midpoints and the jitter are written in the oracle's order and nothing is contracted."""
    from nerfactor_amd import ops
    for n_rays in (1, 5, 300):
        rng = np.random.default_rng(1000 * n_samples + n_rays)
        edges = rng.uniform(size=(n_rays, n_samples)).astype(np.float32)
        edges[:, ::2] = 0.
        edges[:, 1::3] = np.nextafter(np.float32(1), np.float32(0))
        for u in (None, edges, rng.uniform(size=(n_rays, n_samples)).astype(np.float32)):
            got = ops.gen_z(C.NEAR, C.FAR, n_samples, n_rays, lin_in_disp=lin_in_disp, u=dev(u, cuda), device=cuda).cpu().numpy()
            want = nerf_ref.gen_z(C.NEAR, C.FAR, n_samples, n_rays, lin_in_disp, u=u)
            assert got.shape == (n_rays, n_samples)
            assert np.array_equal(got, want), (n_rays, u is not None, np.argwhere(got != want)[:4].tolist(),
                                               float(np.abs(got - want).max()))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_l2_normalize3_at_the_block_edges(nfx_lib, cuda, n):
    """1 / sqrtf is two roundings against the oracle's form: the existing 2e-7, on a NaN-filled output with guard rows."""
    rng = np.random.default_rng(n)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[n // 2] = 0                                   # the zero vector: eps guards the square root
    x = dev(d, cuda)
    buf, out = _guarded(n, (3,), cuda)
    nfx_lib.check(nfx_lib.lib.nfx_l2_normalize3(x.data_ptr(), out.data_ptr(), n, 1e-12, _stream()), 'nfx_l2_normalize3')
    torch.cuda.synchronize()
    _check_guards(buf, 'out')
    got = out.cpu().numpy()
    np.testing.assert_allclose(got, nerf_ref.l2_normalize(d, 1, 1e-12), atol=C.TOL_NORMALIZE, rtol=0)
    assert np.all(got[n // 2] == 0)
