"""Marching tetrahedra on the GPU (csrc/isosurface.hip): ops.isosurface against the NumPy
restatement (tests/isosurface_ref.py) array for array — faces equal, vertices bit for bit — on every small shape at which
the kernels take another path; poisoned buffers; the refusals; and the mesh of the NeRF fitted to a unit sphere."""
import numpy as np
import pytest
import torch

from tests import isosurface_ref as ref
from tests.golden import golden_inputs as gi
from tests.test_gpu_render_from_nerf import fill_nerf

pytestmark = pytest.mark.gpu
BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
RES = 24


def _check(ops, cuda, field, iso, origin=(0., 0., 0.), spacing=(1., 1., 1.)):
    """ops.isosurface == the restatement; returns the restatement's arrays."""
    field = np.ascontiguousarray(field, dtype=np.float32)
    v, f = ops.isosurface(torch.from_numpy(field).to(cuda), iso, origin, spacing)
    want_v, want_f = ref.extract(field, iso, origin, spacing)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == want_v.shape and tuple(f.shape) == want_f.shape, (tuple(v.shape), want_v.shape, tuple(f.shape), want_f.shape)
    assert np.array_equal(f.cpu().numpy(), want_f)
    assert np.array_equal(v.cpu().numpy().view(np.int32), want_v.view(np.int32)), "vertices differ in their bits"
    return want_v, want_f


def test_all_256_sign_patterns_of_one_cell(nfx_lib, cuda):
    from nerfactor_amd import ops
    rng = np.random.default_rng(11)
    n_faces = 0
    for pattern in range(256):
        sign = np.array([1. if (pattern >> k) & 1 else -1. for k in range(8)]).reshape(2, 2, 2)
        _, f = _check(ops, cuda, sign * rng.uniform(0.05, 2., (2, 2, 2)), 0.)
        n_faces += f.shape[0]
    assert n_faces > 1000


@pytest.mark.parametrize('shape', [(3, 2, 2), (2, 5, 3), (7, 4, 9), (33, 17, 5), (65, 3, 3)])
def test_random_fields(nfx_lib, cuda, shape):
    from nerfactor_amd import ops
    rng = np.random.default_rng(sum(shape))
    v, f = _check(ops, cuda, rng.standard_normal(shape), 0.1)
    assert f.shape[0] > 0


# the block scan sums 1024 points per block (rowsel) and 1024 block sums per pass of its one workgroup: lattices of one point
# fewer than, exactly and one more than a multiple of 1024, and around multiples of 1024 * 1024 = 2^20.  2^20 + 1 = 17 * 61681
# has no three factors >= 2, so the lattice just above a multiple is 2^21 + 1 = 9 * 43 * 5419.
@pytest.mark.parametrize('shape', [(3, 11, 31), (8, 8, 16), (5, 5, 41), (9, 35, 13), (16, 16, 16), (3, 3, 569)])
def test_lattices_around_the_scan_block(nfx_lib, cuda, shape):
    from nerfactor_amd import ops
    assert np.prod(shape) in (1023, 1024, 1025, 4095, 4096, 5121)
    rng = np.random.default_rng(int(np.prod(shape)))
    _check(ops, cuda, rng.standard_normal(shape), -0.2)


@pytest.mark.parametrize('shape', [(75, 341, 41), (128, 128, 64), (9, 43, 5419)])
def test_lattices_around_the_second_level_of_the_scan(nfx_lib, cuda, shape):
    """A wavy sheet across the middle axis: it passes through every x slab, so vertices and triangles lie on both sides
    of every 2^20-point boundary, and the restatement stays quick (tens of thousands of cells on the surface)."""
    from nerfactor_amd import ops
    assert np.prod(shape) in (2 ** 20 - 1, 2 ** 20, 2 ** 21 + 1)
    a, b, c = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing='ij')
    field = (b - shape[1] / 2.) * 0.21 + np.sin(0.9 * a + 0.3) + np.sin(0.05 * c)
    v, f = _check(ops, cuda, field, 0.05)
    flat = (np.round(v[:, 0]) * shape[1] + np.round(v[:, 1])) * shape[2]
    assert flat.min() < 2 ** 19 and flat.max() > np.prod(shape) - 2 ** 19 and f.shape[0] > 5000


def test_anisotropic_lattice_with_a_negative_origin(nfx_lib, cuda):
    from nerfactor_amd import ops
    rng = np.random.default_rng(3)
    origin, spacing = (-3.25, -4.7, 0.3), (0.5, 1., 2.)
    _check(ops, cuda, rng.standard_normal((9, 7, 6)), 0., origin, spacing)
    idx = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(6), indexing='ij'), -1)
    grad = np.array([0.7, -1.3, 0.45])
    v, f = _check(ops, cuda, (np.array(origin) + idx * np.array(spacing)) @ grad + 1.234, 0.25, origin, spacing)
    assert ((ref.face_normals(v, f) @ -grad) > 0).all()


def test_corners_exactly_at_iso(nfx_lib, cuda):
    from nerfactor_amd import ops
    rng = np.random.default_rng(6)
    for iso in (-1., 0., 1.):
        v, f = _check(ops, cuda, rng.integers(-2, 3, (6, 5, 7)), iso)
        assert f.shape[0] > 0 and np.isfinite(v).all()


@pytest.mark.parametrize('value', [1., -1.])
def test_no_surface(nfx_lib, cuda, value):
    from nerfactor_amd import ops
    v, f = ops.isosurface(torch.full((5, 4, 3), value, device=cuda), 0.)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32


def test_poisoned_buffers_give_the_same_bits(nfx_lib, cuda):
    from nerfactor_amd import ops
    rng = np.random.default_rng(21)
    field = torch.from_numpy(rng.standard_normal((33, 17, 5)).astype(np.float32)).to(cuda)
    origin, spacing = (0.5, -1., 2.), (0.25, 0.5, 1.)
    got = []
    for ws_fill, v_fill, f_fill in ((0, 0., 0), (-1, float('nan'), -1)):
        ws = ops.isosurface_workspace(field.shape, cuda).fill_(ws_fill)
        ops.isosurface_count(field, 0.1, ws)
        nv, nf, overflow = ws[:3].tolist()
        assert overflow == 0 and nv > 0 and nf > 0
        v = torch.full((nv, 3), v_fill, device=cuda)
        f = torch.full((nf, 3), f_fill, dtype=torch.int32, device=cuda)
        ops.isosurface_emit(field, 0.1, origin, spacing, ws, nv, nf, v, f)
        got.append((v.cpu().numpy().view(np.int32), f.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want_v, want_f = ref.extract(field.cpu().numpy(), 0.1, origin, spacing)
    assert np.array_equal(got[1][0], want_v.view(np.int32)) and np.array_equal(got[1][1], want_f)


def test_refusals(nfx_lib, cuda):
    from nerfactor_amd import ops
    good = torch.zeros((4, 5, 6), device=cuda)
    with pytest.raises(nfx_lib.NfxError, match=r'contiguous.*strides \(1, 6, 30\) of shape \(6, 5, 4\)'):
        ops.isosurface(good.permute(2, 1, 0), 0.)
    with pytest.raises(nfx_lib.NfxError, match='float32, got torch.float64'):
        ops.isosurface(good.double(), 0.)
    with pytest.raises(nfx_lib.NfxError, match='CUDA/ROCm tensor'):
        ops.isosurface(good.cpu(), 0.)
    with pytest.raises(nfx_lib.NfxError, match=r'shape \(20, 6\)'):
        ops.isosurface(good.view(20, 6), 0.)
    with pytest.raises(nfx_lib.NfxError, match='4 x 1 x 6 lattice'):
        ops.isosurface(torch.zeros((4, 1, 6), device=cuda), 0.)
    with pytest.raises(nfx_lib.NfxError, match=r'spacing = \[1.0, 0.0, 1.0\]'):
        ops.isosurface(good, 0., spacing=(1., 0., 1.))
    with pytest.raises(nfx_lib.NfxError, match=r'spacing = \[1.0, 1.0, -0.5\]'):
        ops.isosurface(good, 0., spacing=(1., 1., -.5))
    for bad in (float('nan'), float('inf')):
        field = good.clone()
        field[3, 4, 5] = bad
        with pytest.raises(nfx_lib.NfxError, match=r'\(4, 5, 6\) field holds Inf or NaN'):
            ops.isosurface(field, 0.)
    # the limits on the counts and on the lattice, with their numbers
    ws = ops.isosurface_workspace(good.shape, cuda)
    ops.isosurface_count(good, 0., ws)
    with pytest.raises(nfx_lib.NfxError, match='nv = 2147483648'):
        ops.isosurface_emit(good, 0., (0., 0., 0.), (1., 1., 1.), ws, 2 ** 31, 0)
    with pytest.raises(nfx_lib.NfxError, match='3 nf = 2147483649'):
        ops.isosurface_emit(good, 0., (0., 0., 0.), (1., 1., 1.), ws, 0, (2 ** 31 + 1) // 3)
    assert nfx_lib.lib.nfx_isosurface_workspace_bytes(2048, 1024, 1024) == 0      # 2^31 points
    assert nfx_lib.lib.nfx_isosurface_workspace_bytes(1, 4, 4) == 0
    rc = nfx_lib.lib.nfx_isosurface_count(good.data_ptr(), 2048, 1024, 1024, 0., ws.data_ptr(), ws.numel() * 4, None)
    assert rc != 0 and '2048 x 1024 x 1024 = 2147483648 lattice points' in nfx_lib.last_error()


# ------------------------------------------------------------------------------------------------ the fitted NeRF
@pytest.fixture(scope='module', params=['fp32', 'bf16'])
def fitted(request, nfx_lib, cuda):
    """(model, the RES^3 lattice of its fine network's raw density, extract's output at iso = 0).  iso = 0 and not the
    driver's default 10: the fixture's raw density peaks at 13.5, and its level-10 set is not a sphere (V - E + F = -16)."""
    from nerfactor_amd.nerfactor import mesh_from_nerf
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    torch.manual_seed(0)
    model = get_model_class('nerf')(make_config('nerf', precision=request.param))
    fill_nerf(model, gi.trained_nerf_nets())
    model = model.to(cuda)
    field = mesh_from_nerf.eval_lattice(model, BOX, RES, 'fine')
    return model, field, mesh_from_nerf.extract(model, BOX, RES, iso=0., network='fine')


@pytest.fixture(scope='module')
def oracle_mesh():
    """The restatement's mesh of the oracle's fp32 density on the same lattice."""
    from oracle import nerf_ref
    t = (np.arange(RES, dtype=np.float64) + 0.5) / RES
    axes = [(BOX[2 * k] + t * (BOX[2 * k + 1] - BOX[2 * k])).astype(np.float32) for k in range(3)]
    pts = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 1, 3)
    sigma = nerf_ref.eval_nerf_at(pts, np.zeros_like(pts), gi.trained_nerf_nets()[1])[..., 3]
    from nerfactor_amd.nerfactor import mesh_from_nerf
    return ref.extract(sigma.reshape(RES, RES, RES).astype(np.float32), 0., *mesh_from_nerf.lattice_frame(BOX, RES))


# |V_gpu - V_oracle| measured once on the MI355X at precision = fp32: 2.548e-6 of 3.949; four times that
VOLUME_TOL = 4 * 2.548e-6


def test_fitted_nerf_mesh(fitted, oracle_mesh):
    from nerfactor_amd.nerfactor import mesh_from_nerf
    model, field, (v, f, n) = fitted
    want_v, want_f = ref.extract(field.cpu().numpy(), 0., *mesh_from_nerf.lattice_frame(BOX, RES))
    assert np.array_equal(f, want_f) and np.array_equal(v.view(np.int32), want_v.view(np.int32))
    assert f.shape[0] > 1000 and ref.unpaired_edges(f).shape[0] == 0, "the mesh is closed"
    volume, want_volume = ref.signed_volume(v, f), ref.signed_volume(*oracle_mesh)
    print("fitted NeRF (%s): %d vertices, %d triangles, V - E + F = %d, volume %.6f, oracle lattice %.6f, difference %.3e"
          % (model.precision, v.shape[0], f.shape[0], ref.euler_characteristic(v, f), volume, want_volume, abs(volume - want_volume)))
    if model.precision == 'fp32':
        assert ref.euler_characteristic(v, f) == 2
        assert ref.euler_characteristic(*oracle_mesh) == 2 and 3.9 < want_volume < 4.0
        assert abs(volume - want_volume) <= VOLUME_TOL, (volume, want_volume)


def test_fitted_nerf_normals(fitted):
    from nerfactor_amd import ops
    model, _, (v, f, n) = fitted
    p = torch.from_numpy(v).to(next(model.parameters()).device)
    z = torch.zeros((p.shape[0], 1), device=p.device)
    want = ops.nerf_sigma_grad(p, torch.zeros_like(p), z, model._nerf_geom_blob('fine_'), model.precision)[0][:, 0]
    want = torch.nn.functional.normalize(want, dim=1, eps=1e-12).cpu().numpy()      # -normalize(grad sigma); 0 where sigma <= 0
    have = (want != 0).any(1)
    assert 0.05 * len(v) < have.sum(), "the gradient normal of a fair share of the vertices"
    assert np.abs(n[have] - want[have]).max() <= 1e-6
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.).max() < 1e-5
    # the others: the normalised sum of the adjacent face normals, which leave the sphere
    fn = ref.face_normals(v, f)
    length = np.linalg.norm(fn, axis=1, keepdims=True)
    fn = np.divide(fn, length, out=np.zeros_like(fn), where=length > 0)
    total = np.zeros((len(v), 3))
    np.add.at(total, f.reshape(-1), np.repeat(fn, 3, axis=0))
    total /= np.linalg.norm(total, axis=1, keepdims=True)
    assert np.abs(n[~have] - total[~have]).max() < 1e-5
    # the summed face normals leave the fitted sphere everywhere.  The network's own pointwise gradient does not: with
    # frequencies up to 2^9 in its encoding it is radial neither at every vertex nor on average on this fixture (measured
    # at precision = fp32: radial component min -0.999, mean 0.064 over 2259 vertices), so nothing is asserted of it but
    # that it is the kernel's
    radial = (n * v).sum(1) / np.linalg.norm(v, axis=1)
    print("normals (%s): %d of %d from the gradient, radial component min %.3f mean %.3f (gradient), min %.3f (faces)"
          % (model.precision, have.sum(), len(v), radial[have].min(), radial[have].mean(), radial[~have].min()))
    assert (radial[~have] > 0).all(), "summed face normals point away from the sphere's centre"
