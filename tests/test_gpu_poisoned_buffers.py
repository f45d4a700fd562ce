"""Results do not depend on what freshly allocated memory held.

ops.py allocates every workspace and output with torch.empty / torch.empty_like; the kernels rely on contracts that only
comments state (pad rows of the last tile hold exact zeros in every dZ, the odd half of the last feature pair is zeroed while
staging, a slab past the counted rows is written as zeros, integer accumulators are zeroed in front of their atomics).  In
a test process the allocator hands back mostly fresh memory; in a long training run it hands back whatever the previous
step left there.  Each case below runs one op twice on the same inputs — once with every such allocation filled with byte
0x00, once with 0xFF (NaN as bf16 and fp32, -1 as int32 and int64) — and asserts that every returned tensor and every
gradient buffer the op accumulates into has the same bits both times and is finite.

Left out of the comparison, and nothing else:
  * the workspace tensor that mlp128_bwd, mlp128_bwd_heads and nerf_mlp_bwd return (it is the workspace itself);
  * of occgrid_select's list, a view of its workspace, the entries past the count (nfx.h: not written).
occgrid_select is given its `out`: the samples it lists are left for the density kernel to fill, by contract.

These are ordinary calls with ordinary inputs: the kernels read counts and lists only after the same call wrote them."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

from tests import common
from tests.conftest import ROOT
from tests.test_gpu_nerfactor import dev, net128, scene

pytestmark = pytest.mark.gpu


class _TorchProxy:
    """Stands in for the `torch` name of nerfactor_amd.ops: empty / empty_like return buffers filled with one byte value,
    everything else is torch's.  `filled` counts the allocations it filled."""

    def __init__(self, byte):
        self.byte, self.filled = byte, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _fill(self, t):
        if t.numel():
            # (every element of a dense tensor, whatever its strides)
            torch.as_strided(t, (t.numel(),), (1,)).view(torch.uint8).fill_(self.byte)
            self.filled += 1
        return t

    def empty(self, *args, **kw):
        return self._fill(torch.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._fill(torch.empty_like(*args, **kw))


@contextlib.contextmanager
def fresh_memory_holds(byte):
    from nerfactor_amd import ops
    proxy, real = _TorchProxy(byte), ops.torch
    ops.torch = proxy
    try:
        yield proxy
    finally:
        ops.torch = real


def test_the_proxy_covers_how_ops_allocates():
    """ops.py allocates uninitialised memory through torch.empty and torch.empty_like only (no Tensor.new_empty,
    empty_strided, resize_ ...): what the proxy above intercepts is all there is."""
    src = open(os.path.join(ROOT, 'nerfactor_amd', 'ops.py')).read()
    assert len(re.findall(r'\btorch\.empty(?:_like)?\(', src)) >= 60
    assert not re.findall(r'new_empty|empty_strided|empty_permuted|empty_quantized|\.resize_\(|\.new\(', src)
    with fresh_memory_holds(0xFF) as px:
        from nerfactor_amd import ops
        a = ops.torch.empty((3, 5), dtype=torch.float32)
        b = ops.torch.empty_like(a.t())
        assert px.filled == 2 and bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and ops.torch.float32 is torch.float32
    assert ops.torch is torch


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def check(run):
    """run() -> {name: tensor} of everything the op returned or accumulated into; called once per fill byte."""
    outs = []
    for byte in (0x00, 0xFF):
        with fresh_memory_holds(byte) as px:
            out = run()
            torch.cuda.synchronize()
        assert px.filled >= 1, "the op allocated nothing through torch.empty: the case is blind"
        outs.append(out)
    assert outs[0].keys() == outs[1].keys() and outs[0]
    for name in outs[0]:
        a, b = outs[0][name], outs[1][name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), '%s is not finite' % name
        if not torch.equal(_bits(a), _bits(b)):
            common.assert_same_bits(a, b, '%s: fresh memory 0x00 vs 0xFF' % name)
            raise AssertionError('%s: differs in the sign of a zero or a NaN payload between fresh memory 0x00 and 0xFF' % name)
    return outs[0]


def _grad_buffers(ks, bs, cuda):
    """the buffers a backward op accumulates into: a non-zero start, the same for both runs"""
    return ([torch.full(tuple(k.shape), 0.25, device=cuda) for k in ks], [torch.full(tuple(b.shape), -0.5, device=cuda) for b in bs])


def _named(prefix, tensors):
    return {'%s%d' % (prefix, i): t for i, t in enumerate(tensors)}


def _kb(layers, out):
    return [k for k, _ in layers] + [out[0][0]], [b for _, b in layers] + [out[0][1]]


# ---------------------------------------------------------------------------------------------------- training ops
@pytest.mark.parametrize('wgrad_lds', [0, 1])
@pytest.mark.parametrize('rows', [0, 1])
def test_nerf_mlp_bwd(nfx_lib, cuda, nfx_opt, rows, wgrad_lds):
    """40 rays x 7 samples = 280 points (not a multiple of 16); about half of d_rgbs is four zeros, so the listed count is
    not one either."""
    from nerfactor_amd import ops
    nfx_opt.set('nerf_bwd_rows', rows)
    nfx_opt.set('wgrad_lds', wgrad_lds)
    ks, bs = common.nerf_layers(common.nerf_nets(seed=5, opaque=False)[0])
    rng = np.random.default_rng(317)
    n, s = 40, 7
    rayo = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    rayd = rng.normal(size=(n, 3)).astype(np.float32)
    rayd /= np.linalg.norm(rayd, axis=1, keepdims=True)
    z = np.sort(rng.uniform(0.5, 3., size=(n, s)).astype(np.float32), 1)
    d_rgbs = rng.normal(size=(n * s, 4)).astype(np.float32)
    d_rgbs[rng.uniform(size=n * s) < 0.5] = 0.
    assert int((d_rgbs != 0).any(1).sum()) % 16 != 0
    blob = ops.pack_nerf_train_weights(ks, bs).to(cuda)
    args = (dev(rayo, cuda), dev(rayd, cuda), dev(z, cuda), dev(d_rgbs.reshape(n, s, 4), cuda), blob)

    def run():
        dks, dbs = _grad_buffers(ks, bs, cuda)
        ops.nerf_mlp_bwd(*args, dks, dbs)
        return {**_named('dk', dks), **_named('db', dbs)}
    got = check(run)
    assert float((got['dk0'] - 0.25).abs().max()) > 0


@pytest.mark.parametrize('path', ['fused', 'fused3', 'gemm'])
@pytest.mark.parametrize('kind', ['xyz', 'xyz_ldir'])
def test_mlp128_bwd(nfx_lib, cuda, nfx_opt, kind, path):
    """IN_XYZ: n = 77; IN_XYZ_LDIR: n = 21 points x 512 lights.  fused / fused on 3 persistent workgroups / the
    stored-activation path with its weight-gradient GEMMs."""
    from nerfactor_amd import ops
    nfx_opt.set('wgrad_fused', 0 if path == 'gemm' else 1)
    if path == 'fused3':
        nfx_opt.set('m128_blocks', 3)
    lv = kind == 'xyz_ldir'
    n = 21 if lv else 77
    ks, bs = _kb(*net128(95, 90 if lv else 63, 1 if lv else 3))
    rng, lxyz, _, xyz, _, _ = scene(n, 96)
    xyz_j = xyz + rng.normal(size=xyz.shape).astype(np.float32) * 0.01
    dout = dev(rng.normal(size=(n, 512 if lv else 3)), cuda)
    in_kind = nfx_lib.IN_XYZ_LDIR if lv else nfx_lib.IN_XYZ
    blob = ops.pack_mlp128_train_weights(ks, bs, in_kind, 1 if lv else 3).to(cuda)
    kw = dict(lxyz=dev(lxyz, cuda), xyz_dir=dev(xyz, cuda)) if lv else {}
    x = dev(xyz_j, cuda)

    def run():
        dks, dbs = _grad_buffers(ks, bs, cuda)
        ops.mlp128_bwd(in_kind, x, dout, blob, dks, dbs, out_act='sigmoid', xyz_scale=0.9, **kw)
        return {**_named('dk', dks), **_named('db', dbs)}
    got = check(run)
    assert float((got['dk0'] - 0.25).abs().max()) > 0


def test_mlp128_bwd_heads(nfx_lib, cuda):
    """three heads over the same 77 points in one launch pair"""
    from nerfactor_amd import ops
    n = 77
    rng, _, _, xyz, _, _ = scene(n, 96)
    nets = []
    for seed, (od, act, scale) in enumerate([(3, None, 1.0), (3, 'sigmoid', 0.7), (1, 'softplus', 1.0)]):
        ks, bs = _kb(*net128(40 + seed, 63, od))
        nets.append((ks, bs, ops.pack_mlp128_train_weights(ks, bs, nfx_lib.IN_XYZ, od).to(cuda), dev(rng.normal(size=(n, od)), cuda),
                     act, scale))
    x = dev(xyz, cuda)

    def run():
        heads, out = [], {}
        for h, (ks, bs, blob, dout, act, scale) in enumerate(nets):
            dks, dbs = _grad_buffers(ks, bs, cuda)
            heads.append((dout, blob, dks, dbs, act, scale))
            out.update(_named('head%d_dk' % h, dks))
            out.update(_named('head%d_db' % h, dbs))
        ops.mlp128_bwd_heads(nfx_lib.IN_XYZ, x, heads, xyz_scale=0.9)
        return out
    got = check(run)
    assert all(float((got['head%d_dk0' % h] - 0.25).abs().max()) > 0 for h in range(3))


@pytest.mark.parametrize('wgrad_lds', [None, 1])
def test_brdf_rows_bwd(nfx_lib, cuda, nfx_opt, wgrad_lds):
    """z_dim = 3, 37 rows and their reciprocal halves = 74 rows (not a multiple of 16), through both GEMM forms"""
    from nerfactor_amd import ops
    if wgrad_lds is not None:
        nfx_opt.set('wgrad_lds', wgrad_lds)
    zd, n = 3, 37
    ks, bs = _kb(*net128(113, zd + 15, 1))
    blob = ops.pack_brdf_train_weights(ks, bs, zd).to(cuda)
    rng = np.random.default_rng(46)
    z = dev(rng.normal(size=(n, zd)), cuda)
    rusink = dev(np.stack([rng.uniform(0, np.pi, n), rng.uniform(0, np.pi / 2, n), rng.uniform(0, np.pi / 2, n)], 1), cuda)
    dout = dev(rng.normal(size=2 * n), cuda)

    def run():
        dks, dbs = _grad_buffers(ks, bs, cuda)
        d_z = ops.brdf_rows_bwd(z, rusink, blob, dout, dks, dbs, reci=True)
        return {'d_z': d_z, **_named('dk', dks), **_named('db', dbs)}
    got = check(run)
    assert float(got['d_z'].abs().max()) > 0 and float((got['dk0'] - 0.25).abs().max()) > 0


@pytest.mark.parametrize('rows', [0, 1])
def test_brdf_spec_bwd(nfx_lib, cuda, nfx_opt, rows):
    """z_dim = 3, n = 33 points x 512 lights, half of d spec zero and one point without any gradient"""
    from nerfactor_amd import ops
    nfx_opt.set('brdf_bwd_rows', rows)
    zd, n = 3, 33
    ks, bs = _kb(*net128(110 + zd, zd + 15, 1))
    blob = ops.pack_brdf_train_weights(ks, bs, zd).to(cuda)
    rng, lxyz, _, xyz, cam, normal = scene(n, 211)
    zl = rng.normal(size=(n, zd)).astype(np.float32)
    dspec = rng.normal(size=(n, 512)).astype(np.float32)
    dspec[rng.uniform(size=dspec.shape) < 0.5] = 0.
    dspec[5] = 0.
    args = (dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(zl, cuda), dev(lxyz, cuda), blob, dev(dspec, cuda))

    def run():
        d_z, d_normal = ops.brdf_spec_bwd(*args)
        return {'d_z': d_z, 'd_normal': d_normal}
    got = check(run)
    assert float(got['d_normal'].abs().max()) > 0


def test_shade_bwd(nfx_lib, cuda):
    """64 points x 512 lights, microfacet BRDF, with the light's gradient (integer atomics into the workspace)"""
    from nerfactor_amd import ops
    from tests.test_gpu_nerfactor import _shade_inputs
    n = 64
    rng, lxyz, lareas, xyz, cam, normal, albedo, rough, lvis, lights = _shade_inputs(n, 95)
    rough = np.clip(rough, 0.25, 1.)
    light = (lights[0].reshape(512, 3) * 0.5).astype(np.float32)
    drgb = rng.normal(size=(n, 3)).astype(np.float32)
    args = [dev(a, cuda) for a in (xyz, cam, normal, albedo, lvis, lxyz, lareas, light, drgb)]
    r = dev(rough, cuda)

    def run():
        d_light = torch.full((512, 3), 0.125, device=cuda)
        d_albedo, d_normal, d_lvis, d_rough = ops.shade_bwd(*args, d_light, rough=r, f0=0.04, linear2srgb=True)
        return {'d_albedo': d_albedo, 'd_normal': d_normal, 'd_lvis': d_lvis, 'd_rough': d_rough, 'd_light': d_light}
    got = check(run)
    assert float((got['d_light'] - 0.125).abs().max()) > 0


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
def test_mlp_generic_bwd(nfx_lib, cuda, prec):
    """3 -> 64 -> 64 -> 4 on 77 rows (tests/test_gpu_generic.py), weight, bias and input gradients"""
    from nerfactor_amd import ops
    from oracle import nerf_ref
    d_in, widths, acts, n = 3, [64, 64, 4], ['relu', 'relu', None], 77
    rng = np.random.default_rng(sum(widths) + n)
    layers, prev = [], d_in
    for w in widths:
        layers.append((nerf_ref.glorot_uniform(rng, prev, w), rng.uniform(-.2, .2, size=w).astype(np.float32)))
        prev = w
    ks, bs = [k for k, _ in layers], [b for _, b in layers]
    net = ops.GenericNet(ks, bs, acts, None, train=True, prec=prec).to(cuda)
    x, dy = dev(rng.normal(size=(n, d_in)), cuda), dev(rng.normal(size=(n, widths[-1])), cuda)

    def run():
        dks, dbs = _grad_buffers(ks, bs, cuda)
        dx = ops.mlp_generic_bwd(x, net, dy, dks, dbs, want_dx=True)
        return {'dx': dx, **_named('dk', dks), **_named('db', dbs)}
    got = check(run)
    assert float(got['dx'].abs().max()) > 0 and float((got['dk0'] - 0.25).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------ forward ops
@pytest.mark.parametrize('rows', [0, 1])
@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
def test_nerf_sigma_grad(nfx_lib, cuda, nfx_opt, prec, rows):
    """50 rays x 9 samples; every sample, and only the samples with a density (device-side list in the workspace)"""
    from nerfactor_amd import ops
    from tests.test_gpu_nerf import _geom_inputs
    nfx_opt.set('sigma_grad_rows', rows)
    ks, bs = common.nerf_layers(common.nerf_nets(seed=8)[1])
    gblob = ops.pack_nerf_geom_weights(ks, bs, prec).to(cuda)
    rayo, rayd, z = (dev(a, cuda) for a in _geom_inputs(50, 9, 2))

    def run():
        normal, sigma = ops.nerf_sigma_grad(rayo, rayd, z, gblob, prec)
        return {'normal': normal, 'sigma': sigma}
    got = check(run)
    assert 0 < int((got['sigma'] > 0).sum()) < 450


def test_lvis_fwd(nfx_lib, cuda):
    """70 points x 512 lights (the per-point fold lives in the workspace)"""
    from nerfactor_amd import ops
    from tests.test_gpu_nerfactor import pack
    layers, out = net128(30, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    _, lxyz, _, xyz, _, _ = scene(70, 31, 16)
    x, l = dev(xyz, cuda), dev(lxyz, cuda)
    got = check(lambda: {'lvis': ops.lvis_fwd(x, l, blob, xyz_scale=1.)})
    assert got['lvis'].shape == (70, 512)


def test_nerf_mlp_fwd_folded(nfx_lib, cuda):
    """4 rays x 5 samples through the folded render (the folded blob is made in a workspace on every call)"""
    from nerfactor_amd import ops
    from tests.test_gpu_nerf_fold import _inputs
    blob = ops.pack_nerf_weights(*common.nerf_layers(common.nerf_nets(seed=0)[0])).to(cuda)
    rayo, rayd, z = (dev(a, cuda) for a in _inputs(4, 5))
    got = check(lambda: {'rgbs': ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True)})
    assert got['rgbs'].shape == (4, 5, 4)


def test_nerf_refine_coarse(nfx_lib, cuda):
    """the 96 x 96 view of tests/test_gpu_nerf.py: the list and its count are fresh allocations"""
    from nerfactor_amd import ops
    from tests.golden import golden_inputs as gi
    net = gi.trained_nerf_nets()[0]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net)).to(cuda)
    gblob = ops.pack_nerf_geom_weights(*common.nerf_layers(net), prec='fp32').to(cuda)
    rayo, rayd = common.camera_rays(96, 96, cam_loc=(1.9, -2.8, 2.1))
    o, d = dev(rayo, cuda), ops.l2_normalize3(dev(rayd, cuda), 1e-12)
    z = ops.gen_z(2., 6., 64, o.shape[0], device=cuda)
    raw0 = ops.nerf_mlp_fwd(o, d, z, blob)

    def run():
        raw, count = ops.nerf_refine_coarse(o, d, z, raw0.clone(), gblob, want_count=True)
        return {'rgbs': raw, 'count': count}
    got = check(run)
    assert 0 < int(got['count'].item()) < z.numel() and not torch.equal(got['rgbs'], raw0)


def test_occgrid_select(nfx_lib, cuda):
    """97 rays x 41 samples against a random 16^3 grid"""
    from nerfactor_amd import ops
    from tests.test_gpu_occupancy import _rays
    res, box, n, s = 16, [-1.0, 1.0, -1.25, 0.75, -1.0, 1.5], 97, 41
    rayo, rayd, z = _rays(cuda, n, s, seed=5)
    rayo = rayo / 2.
    g = torch.Generator().manual_seed(2)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, ((res ** 3 + 31) // 32,), generator=g, dtype=torch.int64).int().to(cuda)

    def run():
        out = torch.full((n, s), 7.5, device=cuda)
        out, lst, count = ops.occgrid_select(rayo, rayd, z, bits, res, box, None, out=out)
        k = int(count.item())
        return {'out': out, 'count': count.clone(), 'list': lst[:k].clone()}
    got = check(run)
    assert 0 < int(got['count'].item()) < n * s
