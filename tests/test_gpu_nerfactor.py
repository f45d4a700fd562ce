"""GPU parity suite, NeRFactor stage (through the C-ABI) vs the CPU oracle.

Tolerances: fp32 geometry / BRDF / integration kernels 1e-5-class (stated per test); bf16-MFMA MLPs
vs the oracle with the same operand rounding 4e-3 (x logit scale), vs the fp32 oracle 3e-2 on the
[0,1]-valued outputs."""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_ref, nerfactor_ref as R
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_anchors.npz'))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def net128(seed, in_dims, out_dims, bias_scale=.2):
    rng = np.random.default_rng(seed)
    layers, out = R.init_mlp128(rng, in_dims, out_dims)
    for lst in (layers, out):
        for i, (k, b) in enumerate(lst):
            lst[i] = (k, rng.uniform(-bias_scale, bias_scale, size=b.shape).astype(np.float32))
    return layers, out


def pack(layers, out, in_kind, out_dim, cuda, z_dim=0, prec='bf16'):
    from nerfactor_amd import ops
    ks = [k for k, _ in layers] + [out[0][0]]
    bs = [b for _, b in layers] + [out[0][1]]
    return ops.pack_mlp128_weights(ks, bs, in_kind, out_dim, z_dim=z_dim, prec=prec).to(cuda)


def f64(net):
    return [(k.astype(np.float64), b.astype(np.float64)) for k, b in net]


def scene(n, seed, nl_h=16):
    rng = np.random.default_rng(seed)
    lxyz, lareas = R.gen_light_xyz(nl_h, 2 * nl_h)
    lxyz = lxyz.reshape(-1, 3).astype(np.float32)
    xyz = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    cam = (np.array([2.4, -2.6, 1.8]) * 4 / np.linalg.norm([2.4, -2.6, 1.8])).astype(np.float32)
    cam = np.broadcast_to(cam, (n, 3)).copy()
    normal = nerf_ref.l2_normalize(rng.normal(size=(n, 3)).astype(np.float32), 1, 1e-6)
    return rng, lxyz, lareas.astype(np.float32), xyz, cam, normal


def test_dir2rusink_vs_reference_golden(nfx_lib, cuda):
    from nerfactor_amd import ops
    a, b = GOLD['rusink_a'], GOLD['rusink_b']
    got = ops.dir2rusink(dev(a, cuda), dev(b, cuda)).cpu().numpy()
    d = np.abs(got - GOLD['rusink_out'])
    d[:, 0] = np.minimum(d[:, 0], np.pi - d[:, 0])
    assert d.max() < 2e-3  # fp32 acos/atan2 near the poles vs the float64 reference
    want32 = R.dir2rusink(a.astype(np.float32), b.astype(np.float32))
    d = np.abs(got - want32)
    d[:, 0] = np.minimum(d[:, 0], np.pi - d[:, 0])
    assert d.max() < 2e-3


@pytest.mark.parametrize("out_dim,act,scale,bias", [(3, None, 1., 1e-6), (3, 'sigmoid', .77, .03),
                                                    (1, 'sigmoid', 1., 0.), (3, None, 1., 0.)])
def test_mlp128_xyz_vs_oracle(nfx_lib, cuda, out_dim, act, scale, bias):
    from nerfactor_amd import ops
    layers, out = net128(20 + out_dim, 63, out_dim)
    blob = pack(layers, out, nfx_lib.IN_XYZ, out_dim, cuda)
    rng = np.random.default_rng(21)
    for n in (1, 300, 1031):
        xyz = rng.uniform(-1.2, 1.2, size=(n, 3)).astype(np.float32)
        got = ops.mlp128_xyz_fwd(dev(xyz, cuda), blob, out_dim, out_act=act, xyz_scale=0.9,
                                 post_scale=scale, post_bias=bias).cpu().numpy()
        pe = nerf_ref.embed(np.float32(0.9) * xyz, 10)
        want_q = scale * R.mlp128(pe, layers, out, act, quant=nerf_ref.bf16_round) + bias
        want = scale * R.mlp128(pe, layers, out, act) + bias
        assert got.shape == (n, out_dim)
        assert np.max(np.abs(got - want_q)) < 4e-3
        assert np.max(np.abs(got - want)) < 3e-2
    assert ops.mlp128_xyz_fwd(dev(np.zeros((0, 3)), cuda), blob, out_dim).shape == (0, out_dim)


@pytest.mark.parametrize("n,nl_h", [(70, 16), (3, 4), (261, 16)])
def test_lvis_vs_oracle(nfx_lib, cuda, n, nl_h):
    from nerfactor_amd import ops
    layers, out = net128(30, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    rng, lxyz, _, xyz, _, _ = scene(n, 31, nl_h)
    got = ops.lvis_fwd(dev(xyz, cuda), dev(lxyz, cuda), blob, xyz_scale=1.).cpu().numpy()
    net = {'lvis_mlp': layers, 'lvis_out': out}
    surf2l = R.calc_ldir(xyz, lxyz)
    want = R.pred_lvis_at(xyz, surf2l, net)
    want_q = R.pred_lvis_at(xyz, surf2l, net, quant=nerf_ref.bf16_round)
    assert got.shape == (n, lxyz.shape[0]) and np.all((got >= 0) & (got <= 1))
    assert np.max(np.abs(got - want)) < 3e-2
    assert np.max(np.abs(got - want_q)) < 1e-2  # the per-point fold keeps posenc(xyz) sums in fp32


@pytest.mark.parametrize("zd,variant,n,nl_h", [(3, "6", 50, 16), (1, "6", 50, 16), (3, "5", 50, 16), (3, "3", 50, 16),
                                               (3, "6", 1, 16), (3, "6", 700, 4), (2, "6", 1500, 16), (3, "5", 1027, 8),
                                               (3, "6", 300, 20)])
def test_brdf_spec_vs_oracle(nfx_lib, cuda, nfx_opt, zd, variant, n, nl_h):
    """Learned-BRDF specular term: dense kernel (3), front-lit compaction with the reference's per-row op sequence
    (5) and with closed-form Rusinkiewicz angles (6, the default) against the oracle; point counts below / above the
    number of waves of the grid (1024: the default form, `brdf_compact_kernel<4, 1, 4>`, runs one wave per SIMD), light
    counts that leave the last ballot half empty, and 800 lights — within the 832 that form's row queues and light table
    hold, and more than the opt-in two-waves-per-SIMD form (`brdf_ct` 8) takes (576)."""
    from nerfactor_amd import ops
    nfx_opt.set("brdf_variant", variant)
    layers, out = net128(40 + zd, zd + 15, 1)
    blob = pack(layers, out, nfx_lib.IN_Z_RUSINK, 1, cuda, z_dim=zd)
    rng, lxyz, _, xyz, cam, normal = scene(n, 41, nl_h)
    z = rng.normal(size=(n, zd)).astype(np.float32)
    got = ops.brdf_spec_fwd(dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(z, cuda),
                            dev(lxyz, cuda), blob).cpu().numpy()
    brdf_net = {'brdf_mlp': layers, 'brdf_out': out}
    surf2l, surf2c = R.calc_ldir(xyz, lxyz), R.calc_vdir(cam, xyz)
    want = R.learned_spec(surf2l, surf2c, normal, z, brdf_net)
    want_q = R.learned_spec(surf2l, surf2c, normal, z, brdf_net, quant=nerf_ref.bf16_round)
    front = np.einsum('nij,nlj->nli', R.gen_world2local(normal), surf2l)[..., 2]
    stable = np.abs(front) > 1e-4  # the front-lit test is a step function of a fp32 dot product
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.all(got[stable & (front <= 0)] == 0) and np.all(got[stable & (front > 0)] > 0)
    assert np.max(np.abs(got - want_q)[stable]) < 6e-3 * max(1., want.max())
    assert np.max(np.abs(got - want)[stable]) < 3e-2 * max(1., want.max())
    assert ops.brdf_spec_fwd(dev(xyz[:0], cuda), dev(cam[:0], cuda), dev(normal[:0], cuda), dev(z[:0], cuda),
                             dev(lxyz, cuda), blob).shape == (0, lxyz.shape[0])


def test_width128_fp32_class_paths_vs_fp64_oracle(nfx_lib, cuda):
    """NFX_PREC_FP32 of the three width-128 forward kernels (mlp128_x3.hip: bf16 hi/lo operand pairs, 3 MFMAs per
    product, fp32 accumulate) against the oracle evaluated in float64 on the same float32 inputs: within FP32_TOL of
    the output range (measured 1.2e-5 worst), and at least 50x closer than the bf16 kernels (measured 300-600x)."""
    from nerfactor_amd import ops
    FP32_TOL = 5e-5
    report = {}
    # xyz heads: every activation / affine epilogue, tile remainders
    rng = np.random.default_rng(51)
    for out_dim, act, scale, bias in [(3, None, 1., 1e-6), (3, 'sigmoid', .77, .03), (1, 'sigmoid', 1., 0.)]:
        layers, out = net128(50 + out_dim, 63, out_dim)
        blob32, blob16 = (pack(layers, out, nfx_lib.IN_XYZ, out_dim, cuda, prec=p) for p in ('fp32', 'bf16'))
        for n in (1, 300, 1031):
            xyz = rng.uniform(-1.2, 1.2, size=(n, 3)).astype(np.float32)
            run = lambda blob, prec: ops.mlp128_xyz_fwd(dev(xyz, cuda), blob, out_dim, out_act=act, xyz_scale=0.9,
                                                        post_scale=scale, post_bias=bias, prec=prec).cpu().numpy()
            got, got16 = run(blob32, 'fp32'), run(blob16, 'bf16')
            pe = nerf_ref.embed((np.float32(0.9) * xyz).astype(np.float64), 10)
            want = scale * R.mlp128(pe, f64(layers), f64(out), act) + bias
            assert got.shape == (n, out_dim)
            err, err16 = np.abs(got - want).max(), np.abs(got16 - want).max()
            report['xyz', out_dim, act, n] = (err, err16)
            assert err < FP32_TOL * max(1., np.abs(want).max()), (out_dim, act, n, err)
            assert n < 300 or err < 0.02 * err16, (err, err16)
        assert ops.mlp128_xyz_fwd(dev(np.zeros((0, 3)), cuda), blob32, out_dim, prec='fp32').shape == (0, out_dim)
    # light visibility (the plain 90-dim input, no per-point fold)
    layers, out = net128(52, 90, 1)
    blob32, blob16 = (pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda, prec=p) for p in ('fp32', 'bf16'))
    for n, nl_h in [(70, 16), (3, 4), (261, 16)]:
        _, lxyz, _, xyz, _, _ = scene(n, 53, nl_h)
        got = ops.lvis_fwd(dev(xyz, cuda), dev(lxyz, cuda), blob32, xyz_scale=1., prec='fp32').cpu().numpy()
        got16 = ops.lvis_fwd(dev(xyz, cuda), dev(lxyz, cuda), blob16, xyz_scale=1.).cpu().numpy()
        x64 = xyz.astype(np.float64)
        want = R.pred_lvis_at(x64, R.calc_ldir(x64, lxyz.astype(np.float64)), {'lvis_mlp': f64(layers), 'lvis_out': f64(out)})
        err, err16 = np.abs(got - want).max(), np.abs(got16 - want).max()
        report['lvis', n, nl_h] = (err, err16)
        assert got.shape == (n, lxyz.shape[0]) and err < FP32_TOL, (n, nl_h, err)
        assert n < 70 or err < 0.02 * err16, (err, err16)
    # learned-BRDF specular term; the Rusinkiewicz angles are fp32 on the device (acos / atan2 near their poles move
    # by up to 2e-3 rad, test_dir2rusink_vs_reference_golden), so the bulk is held to FP32_TOL and the tail to 4x that
    for zd, n, nl_h in [(3, 50, 16), (1, 700, 4), (2, 1500, 16)]:
        layers, out = net128(54 + zd, zd + 15, 1)
        blob32, blob16 = (pack(layers, out, nfx_lib.IN_Z_RUSINK, 1, cuda, z_dim=zd, prec=p) for p in ('fp32', 'bf16'))
        rng, lxyz, _, xyz, cam, normal = scene(n, 55, nl_h)
        z = rng.normal(size=(n, zd)).astype(np.float32)
        args = [dev(a, cuda) for a in (xyz, cam, normal, z, lxyz)]
        got = ops.brdf_spec_fwd(*args, blob32, prec='fp32').cpu().numpy()
        got16 = ops.brdf_spec_fwd(*args, blob16).cpu().numpy()
        d = lambda a: a.astype(np.float64)
        surf2l, surf2c = R.calc_ldir(d(xyz), d(lxyz)), R.calc_vdir(d(cam), d(xyz))
        want = R.learned_spec(surf2l, surf2c, d(normal), d(z), {'brdf_mlp': f64(layers), 'brdf_out': f64(out)})
        front = np.einsum('nij,nlj->nli', R.gen_world2local(d(normal)), surf2l)[..., 2]
        stable = np.abs(front) > 1e-4
        assert got.shape == want.shape and np.isfinite(got).all()
        assert np.all(got[stable & (front <= 0)] == 0) and np.all(got[stable & (front > 0)] > 0)
        e, e16, rng_ = np.abs(got - want)[stable], np.abs(got16 - want)[stable], max(1., want.max())
        report['brdf', zd, n, nl_h] = (np.quantile(e, .99), e.max(), np.quantile(e16, .99), e16.max())
        assert np.quantile(e, .99) < FP32_TOL * rng_ and e.max() < 4 * FP32_TOL * rng_, report['brdf', zd, n, nl_h]
        assert np.quantile(e, .99) < 0.02 * np.quantile(e16, .99)
    print('fp32-class width-128 kernels, max-abs error (fp32 path, bf16 path):', report)


def _shade_inputs(n, seed):
    rng, lxyz, lareas, xyz, cam, normal = scene(n, seed)
    albedo = rng.uniform(.03, .8, size=(n, 3)).astype(np.float32)
    rough = rng.uniform(.05, 1., size=(n, 1)).astype(np.float32)
    lvis = rng.uniform(size=(n, 512)).astype(np.float32)
    lights = np.exp(rng.normal(size=(5, 16, 32, 3))).astype(np.float32) * .3
    lights[0] = rng.uniform(0, 1, size=(16, 32, 3))
    return rng, lxyz, lareas, xyz, cam, normal, albedo, rough, lvis, lights


@pytest.mark.parametrize("to_srgb", [True, False])
def test_shade_microfacet_vs_oracle(nfx_lib, cuda, to_srgb):
    from nerfactor_amd import ops
    n = 203
    rng, lxyz, lareas, xyz, cam, normal, albedo, rough, lvis, lights = _shade_inputs(n, 50)
    got = ops.shade_fwd(dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(albedo, cuda),
                        dev(lvis, cuda), dev(lxyz, cuda), dev(lareas, cuda),
                        dev(lights.reshape(5, 512, 3), cuda), rough=dev(rough, cuda), f0=0.04,
                        linear2srgb=to_srgb).cpu().numpy()
    surf2l, surf2c = R.calc_ldir(xyz, lxyz), R.calc_vdir(cam, xyz)
    brdf = R.microfacet(surf2l, surf2c, normal, albedo, rough, f0=0.04)
    brdf64 = R.microfacet(surf2l.astype(np.float64), surf2c.astype(np.float64), normal.astype(np.float64),
                          albedo.astype(np.float64), rough.astype(np.float64), f0=0.04)
    for p in range(5):
        want = R.integrate(brdf, lvis, surf2l, normal, lights[p], lareas, to_srgb)
        want64 = R.integrate(brdf64, lvis.astype(np.float64), surf2l.astype(np.float64),
                             normal.astype(np.float64), lights[p].astype(np.float64),
                             lareas.astype(np.float64), to_srgb)
        # vs the fp32 restatement (sRGB's slope near 0 is 12.92) and vs the fp64 anchor: GGX's
        # 1 - cos^2 cancels catastrophically in fp32 for alpha = rough^2 down to 2.5e-3, so the
        # fp32 evaluations (oracle and kernel alike) sit ~3e-4 from fp64
        assert np.max(np.abs(got[:, p] - want)) < 3e-4, p
        assert np.max(np.abs(got[:, p] - want64)) < 1e-3, p


def test_shade_learned_spec_and_olat_vs_oracle(nfx_lib, cuda):
    from nerfactor_amd import ops
    n = 37
    rng, lxyz, lareas, xyz, cam, normal, albedo, rough, lvis, lights = _shade_inputs(n, 51)
    spec = (rng.uniform(size=(n, 512)) ** 4).astype(np.float32)
    args = (dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(albedo, cuda), dev(lvis, cuda),
            dev(lxyz, cuda), dev(lareas, cuda))
    got = ops.shade_fwd(*args, dev(lights[:2].reshape(2, 512, 3), cuda), spec=dev(spec, cuda),
                        spec_scale=0.7).cpu().numpy()
    surf2l = R.calc_ldir(xyz, lxyz)
    brdf = albedo[:, None, :] / np.float32(np.pi) + spec[:, :, None] * np.float32(0.7)
    for p in range(2):
        want = R.integrate(brdf, lvis, surf2l, normal, lights[p], lareas, True)
        assert np.max(np.abs(got[:, p] - want)) < 2e-4
    # OLAT, microfacet BRDF, with ambient term
    got = ops.shade_olat_fwd(*args, 200., 0.05, rough=dev(rough, cuda)).cpu().numpy()
    brdf = R.microfacet(surf2l, R.calc_vdir(cam, xyz), normal, albedo, rough, f0=0.04)
    assert got.shape == (n, 512, 3)
    for (i, j) in ((0, 0), (7, 13), (15, 31)):
        env = R.one_hot_light(16, 32, i, j, 200., 0.05)
        want = R.integrate(brdf, lvis, surf2l, normal, env, lareas, True)
        assert np.max(np.abs(got[:, i * 32 + j] - want)) < 3e-4


def test_c_abi_rejects_bad_arguments(nfx_lib, cuda):
    from nerfactor_amd import ops
    layers, out = net128(60, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    xyz = torch.zeros((4, 3), device=cuda)
    with pytest.raises(nfx_lib.NfxError, match="multiple of 32"):
        ops.lvis_fwd(xyz, torch.zeros((50, 3), device=cuda), blob)
    with pytest.raises(nfx_lib.NfxError):
        ops.mlp128_xyz_fwd(xyz, blob, 9)
    with pytest.raises(nfx_lib.NfxError, match="float32"):
        ops.lvis_fwd(xyz.double(), torch.zeros((32, 3), device=cuda), blob)


# ------------------------------------------------------------------ full model plugin vs oracle
def _fill(model_net, oracle_layers, oracle_out, body, head):
    for layer, (k, b) in zip(model_net[body].layers, oracle_layers):
        layer.kernel.data.copy_(torch.from_numpy(k))
        layer.bias.data.copy_(torch.from_numpy(b))
    k, b = oracle_out[0]
    model_net[head].layers[0].kernel.data.copy_(torch.from_numpy(k))
    model_net[head].layers[0].bias.data.copy_(torch.from_numpy(b))


def _nerfactor_batch(n, seed, cuda):
    rng, lxyz, lareas, xyz, cam, normal = scene(n, seed)
    alpha = (rng.uniform(size=(n, 1)) < 0.6).astype(np.float32)  # 40 % background rays
    rgb = rng.uniform(size=(n, 3)).astype(np.float32)
    lvis = rng.uniform(size=(n, 512)).astype(np.float32)
    rayd = rng.normal(size=(n, 3)).astype(np.float32)
    np_batch = (cam, rgb, alpha, xyz, normal, lvis)
    t_batch = (['v'] * n, torch.tensor([[1, n]] * n), dev(cam, cuda), dev(rayd, cuda), dev(rgb, cuda),
               dev(alpha, cuda), dev(xyz, cuda), dev(normal, cuda), dev(lvis, cuda))
    return np_batch, t_batch, lxyz, lareas


@pytest.mark.parametrize("variant,precision", [("microfacet", "bf16"), ("learned", "bf16"), ("microfacet", "fp32"),
                                               ("learned", "fp32")])
def test_nerfactor_model_call_vs_oracle(nfx_lib, cuda, variant, precision):
    """models.nerfactor(_microfacet).Model.call(mode='test', relight_probes, relight_olat) end to
    end (mask -> MLP heads -> BRDF -> render -> scatter) vs the NumPy restatement of
    nerfactor.py:181-365: max-abs <= 3e-2 on every [0,1]-valued output with bf16 MLPs, <= 2e-4 with the ini key
    `precision = fp32` (fp32-class MLPs, SURVEY.md §8d's tolerance; measured 2.5e-5 worst, 1.2e-4 on the OLAT frames)."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    name = 'nerfactor_microfacet' if variant == 'microfacet' else 'nerfactor'
    tol = 3e-2 if precision == 'bf16' else 2e-4
    cfg = make_config(name, shape_mode='finetune', shape_model_ckpt='none', brdf_model_ckpt='none',
                      test_envmap_dir='', xyz_jitter_std='0.01', precision=precision)
    torch.manual_seed(0)
    model = get_model_class(name)(cfg).to(cuda)
    zd = model.z_dim
    rng = np.random.default_rng(70)
    onet = R.init_nerfactor_net(rng, zd)
    for k in onet:  # non-zero biases everywhere
        onet[k] = [(w, rng.uniform(-.2, .2, size=b.shape).astype(np.float32)) for w, b in onet[k]]
    for body in ('normal', 'lvis', 'albedo', 'brdf_z'):
        _fill(model.net, onet[body + '_mlp'], onet[body + '_out'], body + '_mlp', body + '_out')
    brdf_net = None
    if variant == 'learned':
        brdf_net = R.init_brdf_mlp(rng, z_dim=zd)
        brdf_net = {k: [(w, rng.uniform(-.2, .2, size=b.shape).astype(np.float32)) for w, b in v]
                    for k, v in brdf_net.items()}
        _fill(model.brdf_model.net, brdf_net['brdf_mlp'], brdf_net['brdf_out'], 'brdf_mlp', 'brdf_out')
    probes = [np.exp(rng.normal(size=(16, 32, 3))).astype(np.float32) * .3 for _ in range(3)]
    for i, p in enumerate(probes):
        model.add_probe('probe%d' % i, p)
    n = 150
    np_batch, t_batch, lxyz, lareas = _nerfactor_batch(n, 71, cuda)
    light = model.light.detach().cpu().numpy()
    pred, gt, loss_kwargs, to_vis = model(t_batch, mode='test', relight_olat=True, relight_probes=True)
    opred, ogt, okw, aux = R.nerfactor_call(
        np_batch, onet, lxyz, lareas, light, variant=variant, brdf_net=brdf_net, f0=0.04,
        probes=probes, olat=(200., 0.))
    mask = aux['mask']
    assert pred['rgb_probes'].shape == (n, 3, 3) and pred['rgb_olat'].shape == (n, 512, 3)
    for k in ('normal', 'lvis', 'albedo', 'rgb', 'rgb_probes'):
        g = pred[k].cpu().numpy()
        assert np.all(g[~mask] == 0), k                      # zero-filled scatter
        assert np.max(np.abs(g - opred[k])) < tol, (k, np.max(np.abs(g - opred[k])))
    g = pred['rgb_olat'].cpu().numpy()
    front_ok = np.abs(np.einsum('nlk,nk->nl', aux['surf2l'], opred['normal'][mask])) > 2e-2
    err = np.abs(g[mask] - opred['rgb_olat'][mask]).max(-1)
    assert np.max(err[front_ok]) < 2 * tol, np.max(err[front_ok])   # one light x inten 200: steep tonemap
    zerr = np.max(np.abs(pred['brdf'].cpu().numpy() - opred['brdf']))
    assert zerr < tol, zerr
    print(variant, precision, 'max-abs:', {k: float(np.max(np.abs(pred[k].cpu().numpy() - opred[k])))
                                           for k in ('normal', 'lvis', 'albedo', 'rgb', 'rgb_probes', 'brdf')},
          'olat', float(np.max(err[front_ok])))
    for k in ('rgb', 'normal', 'lvis'):
        np.testing.assert_array_equal(gt[k].cpu().numpy(), ogt[k])
    # losses: vali = rgb MSE only; test-mode call carries no jitter
    loss_kwargs['keep_batch'] = True
    loss_kwargs.pop('keep_batch')
    lv = model.compute_loss(pred, gt, **dict(loss_kwargs, mode='vali')).cpu().numpy()
    want = R.nerfactor_loss({k: v.cpu().numpy() for k, v in pred.items()},
                            {k: v.cpu().numpy() for k, v in gt.items()}, {}, light, mode='vali')
    np.testing.assert_allclose(lv, want, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", ["nerfactor_microfacet", "nerfactor"])
def test_full_frame_nerfactor_vs_oracle(nfx_lib, cuda, name):
    """BASELINE.json configs[2] at its own size (what bench.py times): one 800 x 800 view of surface points (60 %
    foreground), 512 lights, the trained light + 8 HDR probes through Model.call(mode='test', relight_probes=True) with
    the DEFAULT precision settings, and a 16 384-point slice of that very frame against the fp32 torch-CPU restatement
    of nerfactor.py:181-365.  Stated tolerance: max-abs <= 3e-2 on rgb — required on >= 99.9 % of the
    foreground points over all nine lights, no point set excused beforehand; the remainder is counted and printed (the
    reference's own singular set: spec / (4 |l.n| |v.n|), microfacet.py:57, has no bound as v.n -> 0).  Heads: normal
    (fp32-class by default, shape.py `normal_precision`) 1e-3, albedo / visibility / BRDF code 3e-2; PSNR >= 40 dB."""
    import bench
    from nerfactor_amd import synth
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from oracle import torch_ref
    variant = 'microfacet' if name == 'nerfactor_microfacet' else 'learned'
    torch.manual_seed(5)
    cfg = make_config(name, shape_mode='finetune', shape_model_ckpt='none', brdf_model_ckpt='none',
                      test_envmap_dir='', xyz_jitter_std='0')
    model = get_model_class(name)(cfg).to(cuda)
    for i, p in enumerate(synth.probes(8, seed=20)):
        model.add_probe('p%d' % i, p)
    n, m = 800 * 800, 16384
    hb = synth.surface_batch(n, seed=1, n_lights=512)
    batch = tuple(None if a is None else torch.from_numpy(a).to(cuda) for a in hb)
    pred = model(batch, mode='test', relight_probes=True)[0]
    got = {k: pred[k][:m].cpu().numpy() for k in ('normal', 'lvis', 'albedo', 'brdf')}
    got_rgb = torch.cat((pred['rgb'][:m, None], pred['rgb_probes'][:m]), 1).cpu().numpy()
    del pred, batch
    net, brdf_net = bench.nerfactor_nets_of(model, variant)
    lights = torch.stack([model.light.detach().cpu().reshape(-1, 3)] +
                         [p.cpu().reshape(-1, 3) for p in model.novel_probes.values()])
    c = model.config
    with torch.no_grad():
        ref = torch_ref.nerfactor_render(
            tuple(torch.from_numpy(hb[i][:m]) for i in (2, 5, 6)), net, model.lxyz.cpu(), model.lareas.cpu(), lights,
            variant=variant, brdf_net=brdf_net, f0=c.getfloat('DEFAULT', 'fresnel_f0', fallback=0.04),
            brdf_scale=c.getfloat('DEFAULT', 'learned_brdf_scale', fallback=1.),
            albedo_slope=c.getfloat('DEFAULT', 'albedo_slope'), albedo_bias=c.getfloat('DEFAULT', 'albedo_bias'),
            to_srgb=c.getboolean('DEFAULT', 'linear2srgb'))
    fg = hb[5][:m, 0] > 0
    want_rgb = ref['rgb'].numpy()
    assert np.all(got_rgb[~fg] == 0)
    err = np.abs(got_rgb - want_rgb).max((1, 2))
    above = int((err[fg] > 3e-2).sum())
    head = {k: float(np.abs(got[k] - ref[k].numpy()).max()) for k in got}
    psnr = bench.psnr_uint8_luma(got_rgb.reshape(-1, 3), want_rgb.reshape(-1, 3))
    print("%s 800x800 frame, %d points compared (%d foreground) x 9 lights: PSNR %.1f dB, rgb max-abs %.3g, "
          "%d foreground points (%.4f %%) above 3e-2, heads max-abs %s" % (
              name, m, int(fg.sum()), psnr, float(err.max()), above, 100. * above / fg.sum(), head))
    assert above <= 1e-3 * fg.sum(), (above, int(fg.sum()))
    assert psnr >= 40., psnr
    assert head['normal'] < 1e-3 and head['albedo'] < 3e-2 and head['lvis'] < 3e-2 and head['brdf'] < 3e-2, head


def test_nerfactor_train_mode_loss_vs_oracle(nfx_lib, cuda):
    """Train-mode forward (jittered copies, smoothness + light TV terms) through the plugin; the
    jitter noise is drawn by torch, so the oracle is fed the model's own predictions and only the
    loss arithmetic (nerfactor.py:463-541) is compared."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    cfg = make_config('nerfactor_microfacet', shape_mode='finetune', shape_model_ckpt='none',
                      test_envmap_dir='')
    torch.manual_seed(1)
    model = get_model_class('nerfactor_microfacet')(cfg).to(cuda)
    np_batch, t_batch, lxyz, lareas = _nerfactor_batch(96, 72, cuda)
    pred, gt, loss_kwargs, _ = model(t_batch, mode='train')
    assert all(loss_kwargs[k] is not None for k in
               ('normal_jitter', 'lvis_jitter', 'albedo_jitter', 'brdf_prop_jitter'))
    loss = model.compute_loss(pred, gt, **dict(loss_kwargs)).detach().cpu().numpy()
    tonp = lambda d: {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
                      for k, v in d.items()}
    want = R.nerfactor_loss(tonp(pred), tonp(gt), tonp(loss_kwargs), model.light.detach().cpu().numpy(),
                            mode='train', brdf_smooth_weight=0.)
    np.testing.assert_allclose(loss, want, rtol=2e-5, atol=1e-7)
    # jittered predictions are close to, but not equal to, the clean ones
    d = (pred['albedo'] - loss_kwargs['albedo_jitter']).abs().max().item()
    assert 0 < d < 0.5


@pytest.mark.determinism
def test_row_mlp_kernel_variants_are_bit_identical(nfx_lib, cuda, nfx_opt):
    """Streamed 8 x 32 kernels (mlp128.hip) and the LDS-resident ones with 2 / 3 / 4 column tiles (lvis_v2.hip) compute
    the same arithmetic in the same order: light visibility and the learned-BRDF specular term must agree bit for bit,
    also on a row count that is not a multiple of any tile size.  Every form the library SHIPS is here; the 8-wave
    learned-BRDF forms are not (r03: `brdf_compact_kernel<2, 0, 8>` failed this test on a fresh box — that form is no
    longer built, and `<2, 1, 8>` is opt-in; scripts/soak_8wave.py is their soak)."""
    from nerfactor_amd import ops
    n = 333
    rng, lxyz, _, xyz, cam, normal = scene(n, 77)
    layers, out = net128(31, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    outs = {}
    for v in ("0", "2", "3", "4", "8"):    # 8 = eight waves (two per SIMD) x 2 column tiles: the default
        nfx_opt.set("lvis_variant", v)
        outs[v] = ops.lvis_fwd(dev(xyz, cuda), dev(lxyz, cuda), blob, xyz_scale=0.9)
    for v in ("2", "3", "4", "8"):
        common.assert_same_bits(outs["0"], outs[v], "lvis variant %s against the streamed kernel" % v)
    layers, out = net128(43, 18, 1)
    blob = pack(layers, out, nfx_lib.IN_Z_RUSINK, 1, cuda, z_dim=3)
    z = rng.normal(size=(n, 3)).astype(np.float32)
    outs = {}
    for v in ("0", "2", "3", "4", "5", "6"):
        nfx_opt.set("brdf_variant", v)
        outs[v] = ops.brdf_spec_fwd(dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(z, cuda), dev(lxyz, cuda), blob)
    for v in ("2", "3", "4", "5"):   # 5 = front-lit compaction with the same per-row arithmetic
        common.assert_same_bits(outs["0"], outs[v], "brdf variant %s against the streamed kernel" % v)
    nfx_opt.set("brdf_variant", "5")
    for ct in ("3", "2", "4"):     # column tiles per wave, one wave per SIMD
        nfx_opt.set("brdf_ct", ct)
        got = ops.brdf_spec_fwd(dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(z, cuda), dev(lxyz, cuda), blob)
        common.assert_same_bits(outs["0"], got, "brdf variant 5 (brdf_compact_kernel<%s, 0, 4>) against the streamed kernel" % ct)
    # 6 = closed-form angles: same rows evaluated, values within the rounding of the bf16 MLP inputs
    assert torch.equal(outs["0"] > 0, outs["6"] > 0)
    assert (outs["0"] - outs["6"]).abs().max().item() < 2e-2 * max(1., outs["0"].max().item())


@pytest.mark.determinism
def test_lvis8_bit_identical_at_scale(nfx_lib, cuda, nfx_opt):
    """The default light-visibility kernel runs two waves per SIMD; a sibling kernel of that shape proved non-
    deterministic (profiles/r02/brdf_8wave_race/).  100 000 points x 512 lights, three launches: every row equals the
    one-wave-per-SIMD kernel's, launch after launch."""
    from nerfactor_amd import ops
    n = 100000
    rng, lxyz, _, xyz, _, _ = scene(n, 31, 16)
    layers, out = net128(30, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    args = (dev(xyz, cuda), dev(lxyz, cuda), blob)
    nfx_opt.set("lvis_variant", "4")
    ref = ops.lvis_fwd(*args)
    nfx_opt.unset("lvis_variant")       # the default (8)
    for i in range(3):
        common.assert_same_bits(ref, ops.lvis_fwd(*args), "resident128_kernel<2, 0, 8> (default) launch %d against <4, 0, 4>" % i)


@pytest.mark.determinism
def test_brdf_spec_default_is_deterministic_at_scale(nfx_lib, cuda, nfx_opt):
    """Default learned-BRDF kernel (front-lit compaction, closed-form angles, ONE wave per SIMD since r04) on 100 000
    points x 512 lights: launch after launch the same bits, equal to the other one-wave-per-SIMD tilings, the front-lit
    pattern of the dense kernel, and values within the closed-form bound for all but the rows whose phi_d sits on the
    0 / pi wrap (counted)."""
    from nerfactor_amd import ops
    n, zd = 100000, 3
    rng, lxyz, _, xyz, cam, normal = scene(n, 41, 16)
    layers, out = net128(40 + zd, zd + 15, 1)
    blob = pack(layers, out, nfx_lib.IN_Z_RUSINK, 1, cuda, z_dim=zd)
    z = rng.normal(size=(n, zd)).astype(np.float32)
    args = (dev(xyz, cuda), dev(cam, cuda), dev(normal, cuda), dev(z, cuda), dev(lxyz, cuda), blob)
    nfx_opt.unset("brdf_variant")
    nfx_opt.unset("brdf_ct")
    assert nfx_lib.get_option("brdf_ct") is None and nfx_lib.get_option("brdf_variant") is None
    first = ops.brdf_spec_fwd(*args)
    for i in range(3):
        common.assert_same_bits(first, ops.brdf_spec_fwd(*args), "brdf_compact_kernel<4, 1, 4> (default) launch %d against launch 0" % (i + 1))
    nfx_opt.set("brdf_ct", "2")
    common.assert_same_bits(first, ops.brdf_spec_fwd(*args), "brdf_compact_kernel<2, 1, 4> against the default <4, 1, 4>")
    nfx_opt.unset("brdf_ct")
    nfx_opt.set("brdf_variant", "3")
    dense = ops.brdf_spec_fwd(*args)
    assert torch.equal(dense > 0, first > 0)
    far = ((dense - first).abs() > 1e-2).sum().item()
    assert far <= 40, far        # measured 15 of 5.1e7 rows: phi_d within rounding of the wrap, where the bands flip sign


def test_eval_brdf_at_has_the_reference_signature(nfx_lib, cuda):
    """Model._eval_brdf_at(pts2l, pts2c, normal, albedo, brdf_prop) (nerfactor.py:413-461) works from explicit
    directions alone; with xyz= / cam= it routes through the fused kernel: same values within the bf16 bound."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    torch.manual_seed(2)
    cfg = make_config('nerfactor', shape_mode='finetune', shape_model_ckpt='none', brdf_model_ckpt='none',
                      test_envmap_dir='')
    model = get_model_class('nerfactor')(cfg).to(cuda)
    n = 40
    rng, lxyz, _, xyz, cam, normal = scene(n, 5)
    z = dev(rng.normal(size=(n, 3)) * 0.5, cuda)
    albedo = dev(rng.uniform(0.1, 0.8, size=(n, 3)), cuda)
    pts2l = dev(R.calc_ldir(xyz, lxyz), cuda)
    pts2c = dev(R.calc_vdir(cam, xyz), cuda)
    a = model._eval_brdf_at(pts2l, pts2c, dev(normal, cuda), albedo, z)
    b = model._eval_brdf_at(pts2l, pts2c, dev(normal, cuda), albedo, z, xyz=dev(xyz, cuda), cam=dev(cam, cuda))
    assert a.shape == b.shape == (n, lxyz.shape[0], 3)
    front = np.einsum('nij,nlj->nli', R.gen_world2local(normal), R.calc_ldir(xyz, lxyz))[..., 2]
    stable = torch.from_numpy(np.abs(front) > 1e-4).to(cuda)
    assert float((a - b).abs()[stable].max()) < 3e-2 * max(1., float(a.max()))
    brdf_net = {k: [(l.kernel.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in model.brdf_model.net[k].layers]
                for k in ('brdf_mlp', 'brdf_out')}
    want = R.learned_brdf(R.calc_ldir(xyz, lxyz), R.calc_vdir(cam, xyz), normal, albedo.cpu().numpy(), z.cpu().numpy(),
                          brdf_net, 1.)
    # the prior itself runs on the fused bf16 template (nfx_brdf_rows_fwd) in both routes: bf16 bound against fp64
    assert np.abs(a.cpu().numpy() - want)[stable.cpu().numpy()].max() < 3e-2 * max(1., float(want.max()))


def test_all_finite_kernel(nfx_lib, cuda):
    """nfx_any_nonfinite (check_numerics in one pass) against torch.isfinite(x).all(): clean tensors of awkward sizes,
    one NaN / +Inf / -Inf anywhere including the scalar tail, empty tensors."""
    from nerfactor_amd import ops
    g = torch.Generator().manual_seed(1)
    for n in (0, 1, 3, 4, 5, 1023, 4096, 1000003):
        x = (torch.randn(n, generator=g) * 1e30).to(cuda)
        assert bool(ops.all_finite(x)) == bool(torch.isfinite(x).all())
        for pos, bad in ((0, float('nan')), (n - 1, float('inf')), (n // 2, float('-inf'))):
            if n == 0:
                continue
            y = x.clone()
            y[pos] = bad
            assert not bool(ops.all_finite(y)), (n, pos)
    assert bool(ops.all_finite(torch.full((70,), 3.4e38, device=cuda)))          # the largest finite float


@pytest.mark.parametrize("shape", [(1000, 512), (777, 3), (640, 9, 3), (33, 1), (5, 6), (40, 0, 3), (0, 5)])
def test_scatter_rows_is_tf_scatter_nd_of_the_foreground_rows(nfx_lib, cuda, shape):
    """nfx_scatter_rows against zeros + index_put_ (the reference's tf.scatter_nd, nerfactor.py:295-306): bit-equal, every
    output element written (the output buffer is pre-filled with NaN by the allocator trick below).  [n, 0, 3] is what a
    test render without light probes scatters (the drivers' tests found it), [0, d] a view without foreground."""
    from nerfactor_amd import ops
    rng = np.random.default_rng(4)
    n_all = shape[0] * 2 + 7
    mask = np.zeros(n_all, bool)
    mask[rng.permutation(n_all)[:shape[0]]] = True
    idx = torch.from_numpy(np.nonzero(mask)[0]).to(cuda)
    src = dev(rng.normal(size=shape), cuda)
    row_of = torch.full((n_all,), -1, dtype=torch.int32, device=cuda)
    row_of[idx] = torch.arange(idx.numel(), dtype=torch.int32, device=cuda)
    junk = torch.full((n_all,) + shape[1:], float('nan'), device=cuda)   # make stale NaNs likely in the next allocation
    del junk
    got = ops.scatter_rows(src, row_of, n_all)
    want = torch.zeros((n_all,) + shape[1:], device=cuda)
    want[idx] = src
    assert torch.equal(got, want)
    with pytest.raises(nfx_lib.NfxError):
        ops.scatter_rows(src, row_of.long(), n_all)


def test_lvis_verify_option_checks_the_two_wave_kernel_against_the_one_wave_form(nfx_lib, cuda, nfx_opt, monkeypatch):
    """nfx_set_option("lvis_verify", k): every k-th launch of the default light-visibility kernel
    (two waves per SIMD) is checked bit for bit against the one-wave-per-SIMD kernel on ~1 % of its points.  Here: it
    stays silent on a healthy kernel (40 launches, every 2nd checked), and it does raise when the comparison sees a
    difference (the reference launch is doctored through the xyz_scale it is given)."""
    from nerfactor_amd import _capi, ops
    layers, out = net128(30, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    rng, lxyz, _, xyz, _, _ = scene(20000, 31)
    x, l = dev(xyz, cuda), dev(lxyz, cuda)
    plain = ops.lvis_fwd(x, l, blob)
    nfx_opt.set("lvis_verify", "2")
    before = ops._lvis_launches[0]
    for _ in range(40):
        assert torch.equal(ops.lvis_fwd(x, l, blob), plain)
    assert ops._lvis_launches[0] - before == 40
    # a checker that cannot fail proves nothing: make the reference launch see a different scale
    real = _capi.lib.nfx_lvis_fwd
    calls = {'n': 0}

    class Doctored:
        def __call__(self, xp, xd, n, scale, *rest):
            calls['n'] += 1
            return real(xp, xd, n, scale * (1.001 if calls['n'] % 2 == 0 else 1.0), *rest)
    monkeypatch.setattr(ops.lib, 'nfx_lvis_fwd', Doctored(), raising=False)
    with pytest.raises(_capi.NfxError, match="lvis_verify"):
        for _ in range(4):
            ops.lvis_fwd(x, l, blob)


@pytest.mark.determinism
@pytest.mark.parametrize("variant", ["8", "4"])
def test_lvis_rows_mode_stores_at_final_rows_and_flags_nans(nfx_lib, cuda, nfx_opt, variant):
    """nfx_lvis_fwd_rows (round 6): the visibilities of compact point i land in row out_row[i] of a full-size buffer, bit-identical
    to the compact launch; rows that are not named stay what they were (nfx_zero_rows zeroes exactly the background rows); a NaN
    input raises the flag; the shading kernels read the same rows through `lvis_row`."""
    from nerfactor_amd import ops
    nfx_opt.set("lvis_variant", variant)
    nfx_opt.set("lvis_rows", "1")
    layers, out = net128(30, 90, 1)
    blob = pack(layers, out, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    n_all, n = 3000, 1777
    rng, lxyz, lareas, xyz, cam, normal = scene(n, 31)
    rows = np.sort(rng.choice(n_all, n, replace=False)).astype(np.int32)
    x, l = dev(xyz, cuda), dev(lxyz, cuda)
    compact = ops.lvis_fwd(x, l, blob)
    full = torch.full((n_all, l.shape[0]), -7., device=cuda)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    out_row = torch.from_numpy(rows).to(cuda)
    assert ops.lvis_rows_supported()
    got = ops.lvis_fwd(x, l, blob, out=full, out_row=out_row, nan_flag=flag)
    assert got is full and int(flag.item()) == 0
    assert torch.equal(full[out_row.long()], compact)
    others = torch.ones(n_all, dtype=torch.bool, device=cuda)
    others[out_row.long()] = False
    assert bool((full[others] == -7.).all())
    row_of = torch.full((n_all,), -1, dtype=torch.int32, device=cuda)
    row_of[out_row.long()] = torch.arange(n, dtype=torch.int32, device=cuda)
    ops.zero_rows(full, row_of)
    assert torch.equal(full, ops.scatter_rows(compact, row_of, n_all))            # = the zero-filled scatter of the compact tensor
    # shading through the row index = shading of the compact tensor
    albedo = dev(rng.uniform(0.1, 0.9, size=(n, 3)), cuda)
    rough = dev(rng.uniform(0.1, 0.9, size=(n,)), cuda)
    lights = dev(rng.uniform(0, 2, size=(3, l.shape[0], 3)), cuda)
    args = (x, dev(cam, cuda), dev(normal, cuda), albedo)
    a = ops.shade_fwd(*args, compact, l, dev(lareas, cuda), lights, rough=rough)
    b = ops.shade_fwd(*args, full, l, dev(lareas, cuda), lights, rough=rough, lvis_row=out_row)
    assert torch.equal(a, b)
    a = ops.shade_olat_fwd(*args, compact, l, dev(lareas, cuda), 200., 0.1, rough=rough)
    b = ops.shade_olat_fwd(*args, full, l, dev(lareas, cuda), 200., 0.1, rough=rough, lvis_row=out_row)
    assert torch.equal(a, b)
    # a NaN visibility: the kernel's own epilogue reports it.  (A NaN INPUT does not make one — v_med3 / fmaxf drop NaNs at the
    # first ReLU and in the direction's normalisation, for the compact launch and check_numerics alike; NaN WEIGHTS, what a
    # diverged training leaves behind, do: here the output layer's bias)
    out_nan = [(out[0][0], np.full_like(out[0][1], np.nan))]
    blob_nan = pack(layers, out_nan, nfx_lib.IN_XYZ_LDIR, 1, cuda)
    flag.zero_()
    ops.lvis_fwd(x, l, blob_nan, out=full, out_row=out_row, nan_flag=flag)
    assert int(flag.item()) == 1 and bool(torch.isnan(full[out_row.long()]).all())
    assert bool(torch.isnan(ops.lvis_fwd(x, l, blob_nan)).all())
    # unsupported forms say so
    nfx_opt.set("lvis_variant", "0")
    assert not ops.lvis_rows_supported()
    with pytest.raises(nfx_lib.NfxError):
        ops.lvis_fwd(x, l, blob, out=full, out_row=out_row)


@pytest.mark.determinism
@pytest.mark.parametrize("name", ["nerfactor_microfacet", "nerfactor"])
def test_render_with_background_rays_is_the_same_through_the_final_row_stores(nfx_lib, cuda, nfx_opt, name):
    """Model.call(mode='test', relight_probes, relight_olat) on a batch with background rays: the round-6 path (visibilities stored
    at their final rows by the kernel, shading through the row index, NaN flag from the kernel) against the round-5 path
    (compact tensor + nfx_scatter_rows + nfx_any_nonfinite: option lvis_rows = 0): every output tensor bit for bit; and NaN
    weights raise as check_numerics would."""
    from nerfactor_amd import synth
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    torch.manual_seed(5)
    cfg = make_config(name, shape_mode='finetune', shape_model_ckpt='none', brdf_model_ckpt='none', test_envmap_dir='', xyz_jitter_std='0')
    model = get_model_class(name)(cfg).to(cuda)
    for i, p in enumerate(synth.probes(2, seed=20)):
        model.add_probe('p%d' % i, p)
    hb = synth.surface_batch(5000, seed=3, n_lights=512)
    batch = tuple(None if a is None else torch.from_numpy(a).to(cuda) for a in hb)

    def run():
        with torch.no_grad():
            pred, gt, _, _ = model(batch, mode='test', relight_probes=True, relight_olat=True)
        return {k: v.clone() for k, v in pred.items()}, {k: v.clone() for k, v in gt.items()}
    nfx_opt.set("lvis_rows", "1")             # opt-in: final-row stores
    with torch.no_grad():
        assert model._lvis_rows_ok()
    new, gt_new = run()
    nfx_opt.set("lvis_rows", "0")             # the default path: compact tensor, nfx_scatter_rows, nfx_any_nonfinite
    with torch.no_grad():
        assert not model._lvis_rows_ok()
    old, gt_old = run()
    assert set(new) == set(old) and {'rgb', 'lvis', 'rgb_probes', 'rgb_olat'} <= set(new)
    for k in new:
        assert torch.equal(new[k], old[k]), k
    for k in gt_new:
        assert torch.equal(gt_new[k], gt_old[k]), k
    bg = batch[5][:, 0] == 0
    assert 0.3 * bg.numel() < int(bg.sum()) < 0.5 * bg.numel() and not bool(new['lvis'][bg].any())
    # NaN weights (a diverged training): the kernel's flag raises what check_numerics raised
    with torch.no_grad():
        model.net['lvis_out'].layers[0].bias.fill_(float('nan'))
    for rows_on in ("1", "0"):
        nfx_opt.set("lvis_rows", rows_on)
        with pytest.raises(FloatingPointError, match="Light visibility"):
            with torch.no_grad():
                model(batch, mode='test')
