"""Rendering a trained NeRFactor straight from camera rays (nerfactor/surface.py, nerfactor/render_from_nerf.py) on the
GPU: the surface kernel nfx_nerf_surface_fwd against the ops it replaces, march_surface against the reference's own
geometry outputs, and the direct route against geometry_from_nerf -> test.py end to end (one process and two ranks)."""
import glob
import os
import shutil
import socket
import subprocess
import sys
from os.path import basename, exists, join

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import nerf_ref
from tests import common, synth_scene
from tests.golden import golden_inputs as gi

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'reference_models.npz'))
BBOX = '-1.5,1.5,-1.5,1.5,-1.5,1.5'
PRECISIONS = ('fp32', 'bf16')


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def fill_nerf(model, nets):
    with torch.no_grad():
        for pref, net in zip(('coarse_', 'fine_'), nets):
            for part in ('enc', 'sigma_out', 'bottleneck', 'rgb_out'):
                for layer, (k, b) in zip(model.net[pref + part].layers, net[part]):
                    layer.kernel.copy_(torch.from_numpy(np.asarray(k, np.float32)))
                    layer.bias.copy_(torch.from_numpy(np.asarray(b, np.float32)))


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.


def _excluded(err, tol, what, max_frac=0.02):
    """tests/test_gpu_reference_golden.py's counted exclusion rule: every element within `tol` but an explicit, reported
    set of at most `max_frac` of them."""
    bad = np.flatnonzero(err > tol)
    print("%s: %d of %d elements above %.0e (max %.3e): %s" % (what, len(bad), err.size, tol, err.max(), bad[:16].tolist()))
    assert len(bad) <= max_frac * err.size, (what, len(bad), err.size, float(err.max()))


# ---------------------------------------------------------------------------------------------- the kernel
def _surface_inputs(n, s, seed, cuda, kind='random'):
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(2. + 4. * torch.rand((n, s), generator=g), dim=1)[0]
    rayo = torch.randn((n, 3), generator=g) * 2.
    rayd = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=1)
    sigma = torch.randn((n, s), generator=g) * 8.
    sigma[torch.rand((n, s), generator=g) < 0.5] = 0.               # runs of empty space
    if kind == 'empty':
        sigma = -torch.rand((n, s), generator=g)                     # relu: nothing anywhere
    elif kind == 'saturated':                                      # evenly spaced: the first sample takes it all
        z = torch.linspace(2., 6., s)[None].expand(n, s).contiguous()
        sigma = 1e3 + torch.rand((n, s), generator=g)
    elif kind == 'faint':                                          # occupancies spread over (0, 1)
        sigma = sigma.abs() * 0.3 * torch.rand((n, 1), generator=g)
    elif kind == 'mixed' and n:                                     # every fourth ray empty, every fourth saturated
        sigma[0::4] = 0.
        sigma[1::4] = 1e4
    return tuple(t.to(cuda) for t in (sigma, z, rayo, rayd))


def _reference(sigma, z, rayo, rayd, thres):
    """Model.accumulate_sigma (the compositing kernel's weights), float64 sums, process_view's epilogue."""
    from nerfactor_amd.nerfactor.models.nerf import Model
    w = Model.accumulate_sigma(sigma, z, rayd).double()
    occu = w.sum(-1)
    depth = (w * z.double()).sum(-1)
    alpha = torch.where(occu < thres, torch.zeros_like(occu), occu).clamp(0., 1.)
    xyz = (rayo.double() + rayd.double() * depth[:, None]) * alpha[:, None]
    return occu, depth, alpha, xyz


def _check_surface(sigma, z, rayo, rayd, thres, want_occu=True):
    from nerfactor_amd import ops
    alpha_q, xyz, depth, occu = ops.nerf_surface(sigma, z, rayo, rayd, occu_thres=thres, want_occu=want_occu)
    alpha, xyz2, depth2, _ = ops.nerf_surface(sigma, z, rayo, rayd, occu_thres=thres, quantize_alpha=False)
    torch.cuda.synchronize()
    r_occu, r_depth, r_alpha, r_xyz = _reference(sigma, z, rayo, rayd, thres)
    n = sigma.shape[0]
    assert alpha_q.shape == (n,) and xyz.shape == (n, 3) and depth.shape == (n,)
    assert (occu is None) == (not want_occu)
    if occu is not None:
        assert _maxabs(occu.double() - r_occu) <= 1e-6
    assert torch.equal(xyz, xyz2) and torch.equal(depth, depth2)
    assert _maxabs(depth.double() - r_depth) <= 1e-5 * 6.     # 1e-5 x far
    assert _maxabs(xyz.double() - r_xyz) <= 1e-5
    assert _maxabs(alpha.double() - r_alpha) <= 1e-6
    # quantised alpha = what alpha.png read back gives, except where 255 alpha sits on a rounding edge
    a255 = (r_alpha * 255.).cpu().numpy()
    edge = np.abs(a255 - np.floor(a255) - 0.5) < 1e-4
    want_q = np.floor(a255 + 0.5) / 255.
    got_q = alpha_q.cpu().numpy().astype(np.float64)
    assert np.all((np.abs(got_q - want_q) < 1e-7) | edge)
    assert np.all(np.abs(got_q * 255. - np.round(got_q * 255.)) < 1e-4)        # a multiple of 1/255
    return alpha_q, xyz, depth, occu


@pytest.mark.parametrize('s', [1, 63, 64, 65, 320])
@pytest.mark.parametrize('n', [1, 5, 1027])
def test_surface_kernel_equals_accumulate_sigma_sums_and_blend(nfx_lib, cuda, n, s):
    _check_surface(*_surface_inputs(n, s, seed=n * 1000 + s, cuda=cuda, kind='mixed'), thres=0.)


@pytest.mark.parametrize('thres', [0.3, 0.9])
def test_surface_kernel_occupancy_threshold(nfx_lib, cuda, thres):
    inputs = _surface_inputs(2049, 320, seed=7, cuda=cuda, kind='faint')
    alpha_q, xyz, _, occu = _check_surface(*inputs, thres=thres)
    below = occu < thres
    assert bool(below.any()) and bool((~below).any())
    assert float(alpha_q[below].abs().max()) == 0. and float(xyz[below].abs().max()) == 0.


def test_surface_kernel_empty_and_saturated_rays(nfx_lib, cuda):
    inputs = _surface_inputs(37, 65, seed=3, cuda=cuda, kind='empty')
    alpha_q, xyz, depth, occu = _check_surface(*inputs, thres=0.)
    assert float(alpha_q.abs().max()) == 0. and float(xyz.abs().max()) == 0. and float(occu.abs().max()) == 0.
    assert not torch.signbit(xyz).any()                   # + 0 as _alpha_blend gives, not -0
    inputs = _surface_inputs(37, 65, seed=4, cuda=cuda, kind='saturated')
    alpha_q, xyz, depth, occu = _check_surface(*inputs, thres=0.)
    assert float((alpha_q - 1.).abs().max()) == 0.
    # a saturated ray stops at its first sample
    np.testing.assert_allclose(depth.cpu().numpy(), inputs[1][:, 0].cpu().numpy(), rtol=1e-5)


def test_surface_kernel_without_the_occupancy_output_and_without_rays(nfx_lib, cuda):
    from nerfactor_amd import ops
    _check_surface(*_surface_inputs(130, 192, seed=11, cuda=cuda), thres=0.1, want_occu=False)
    empty = torch.empty((0, 320), device=cuda)
    alpha, xyz, depth, occu = ops.nerf_surface(empty, empty, torch.empty((0, 3), device=cuda),
                                               torch.empty((0, 3), device=cuda), want_occu=True)
    assert alpha.shape == (0,) and xyz.shape == (0, 3) and depth.shape == (0,) and occu.shape == (0,)


def test_surface_kernel_rejects_bad_arguments(nfx_lib, cuda):
    from nerfactor_amd import ops
    sigma, z, rayo, rayd = _surface_inputs(8, 16, seed=1, cuda=cuda)
    with pytest.raises(nfx_lib.NfxError):
        ops.nerf_surface(sigma, z[:, :15], rayo, rayd)
    with pytest.raises(nfx_lib.NfxError):
        ops.nerf_surface(sigma, z, rayo, rayd, occu_thres=float('nan'))
    with pytest.raises(nfx_lib.NfxError):
        ops.nerf_surface(sigma.double(), z, rayo, rayd)


# ---------------------------------------------------------------------------------------------- against the reference
def _nerf(cuda, nets):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    torch.manual_seed(0)
    model = get_model_class('nerf')(make_config('nerf'))
    fill_nerf(model, nets)
    return model.to(cuda)


@pytest.mark.parametrize('bbox', [False, True])
def test_march_surface_vs_reference_outputs(nfx_lib, cuda, bbox):
    """occupancy / depth of march_surface against what the reference's geometry_from_nerf computed for the fixture
    networks and rays, under the tolerances and the counted exclusion rule tests/test_gpu_reference_golden.py holds
    compute_depth_and_normal to on the same arrays."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.surface import march_surface
    model = _nerf(cuda, common.nerf_nets(seed=gi.NERF_SEED))
    box = tuple(float(v) for v in gi.GEOM_BBOX.split(',')) if bbox else None
    tag = 'geo_bbox_' if bbox else 'geo_'
    rayo, rayd, _ = gi.nerf_rays()
    rayo, rayd = rayo[:gi.GEOM_RAYS], rayd[:gi.GEOM_RAYS]          # (march_surface normalises the directions itself)
    with torch.no_grad():
        alpha, xyz, occu, depth = march_surface(model, dev(rayo, cuda), dev(rayd, cuda), make_config('nerf'), bbox=box,
                                                full=True)
    occu, depth = occu.cpu().numpy(), depth.cpu().numpy()
    _excluded(np.abs(occu - GOLD[tag + 'occu']), 3e-2, tag + 'occupancy')
    _excluded(np.abs(depth - GOLD[tag + 'depth']), 0.16, tag + 'depth')
    a = np.clip(occu, 0., 1.)
    np.testing.assert_array_equal(alpha.cpu().numpy(), np.floor(a.astype(np.float32) * np.float32(255) + np.float32(.5))
                                  / np.float32(255))


def test_march_surface_on_the_trained_nerf_vs_reference_outputs(nfx_lib, cuda):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.surface import march_surface
    model = _nerf(cuda, gi.trained_nerf_nets())
    rayo, rayd, _ = gi.nerf1k_rays()
    rayo, rayd = rayo[gi.GEO1K_RAYS], rayd[gi.GEO1K_RAYS]
    with torch.no_grad():
        _, _, occu, depth = march_surface(model, dev(rayo, cuda), dev(rayd, cuda), make_config('nerf'), full=True)
    _excluded(np.abs(occu.cpu().numpy() - GOLD['geo1k_occu']), 3e-2, 'geometry occu')
    _excluded(np.abs(depth.cpu().numpy() - GOLD['geo1k_depth']), 0.12, 'geometry depth')


def test_march_surface_equals_the_geometry_march(nfx_lib, cuda):
    """The same march as compute_depth_and_normal (whose fine densities come from the gradient kernel: bit-identical
    densities), reduced in the kernel instead of torch: occupancy and depth within fp32 summation order, chunked or not."""
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.surface import march_surface
    cfg = make_config('nerf')
    model = _nerf(cuda, gi.trained_nerf_nets())
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), dev(rayd, cuda)
    with torch.no_grad():
        occu, depth, _ = G.compute_depth_and_normal(model, o, torch.nn.functional.normalize(d, dim=1, eps=1e-12), cfg)
        alpha, xyz, occu2, depth2 = march_surface(model, o, d, cfg, full=True)
        alpha3, xyz3 = march_surface(model, o, d, cfg, mlp_chunk=320 * 100)          # ragged chunks of 100 rays
    assert float((occu - occu2).abs().max()) <= 1e-6 and float((depth - depth2).abs().max()) <= 6e-6
    assert torch.equal(alpha, alpha3) and torch.equal(xyz, xyz3)
    assert 100 < int((alpha > 0).sum()) < 1024


# ---------------------------------------------------------------------------------------------- the two routes
@pytest.fixture(scope='module')
def runs(tmp_path_factory, nfx_lib, cuda):
    """A 24 x 24 synthetic scene (tests/synth_scene.py), the NeRF fitted to its unit sphere in the trainvali layout, a BRDF
    prior and one NeRFactor checkpoint per model, two HDR probes; then both routes: geometry_from_nerf -> test.py and
    render_from_nerf."""
    from nerfactor_amd.nerfactor import geometry_from_nerf, render_from_nerf, test as test_driver
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.util import light as L
    root = str(tmp_path_factory.mktemp('from_nerf'))
    data_root, _ = synth_scene.write_scene(root, imh=24, imw=24, n_train=1, n_val=1, n_test=3)

    def save(name, outdir, model, **over):
        os.makedirs(join(outdir, 'checkpoints'))
        with open(outdir + '.ini', 'w') as h:
            make_config(name, **over).write(h)
        model.register_trainable()
        torch.save({'net': model.state_dict(), 'step': 0}, join(outdir, 'checkpoints', 'ckpt-1'))
        return join(outdir, 'checkpoints', 'ckpt-1')
    nerf_dir = join(root, 'out_nerf', 'lr1e-4')
    nerf_over = dict(data_root=data_root, imh=24)
    nerf = get_model_class('nerf')(make_config('nerf', **nerf_over))
    fill_nerf(nerf, gi.trained_nerf_nets())
    save('nerf', nerf_dir, nerf, **nerf_over)
    merl = join(root, 'merl')
    synth_scene.write_merl(merl)
    brdf_over = dict(data_root=merl)
    torch.manual_seed(1)
    brdf_ckpt = save('brdf', join(root, 'out_brdf', 'lr1e-2'), get_model_class('brdf')(make_config('brdf', **brdf_over)),
                     **brdf_over)
    probes = join(root, 'probes')
    os.makedirs(probes)
    for i, p in enumerate(synth_scene_probes()):
        L.write_hdr(p, join(probes, 'p%d.hdr' % i))
    surf_root = join(root, 'surf')
    thres = '0.05'
    geometry_from_nerf.main(['--trained_nerf=' + nerf_dir, '--out_root=' + surf_root, '--imh=24', '--scene_bbox=' + BBOX,
                             '--occu_thres=' + thres])
    out = {'root': root, 'nerf_dir': nerf_dir, 'surf_root': surf_root, 'data_root': data_root, 'thres': thres}
    for name in ('nerfactor_microfacet', 'nerfactor'):
        for prec in PRECISIONS:
            over = dict(data_root=data_root, data_nerf_root=surf_root, imh=24, shape_mode='finetune', shape_model_ckpt='none',
                        brdf_model_ckpt=brdf_ckpt, test_envmap_dir=probes, precision=prec)
            torch.manual_seed(2)            # the same weights in both precisions
            ckpt = save(name, join(root, 'out_%s_%s' % (name, prec), 'lr5e-3'),
                        get_model_class(name)(make_config(name, **over)), **over)
            disk = test_driver.main(['--ckpt=' + ckpt])
            direct = render_from_nerf.main(['--ckpt=' + ckpt, '--trained_nerf=' + nerf_dir, '--scene_bbox=' + BBOX,
                                            '--occu_thres=' + thres])
            out[name, prec] = (ckpt, disk, direct)
    return out


def synth_scene_probes():
    from nerfactor_amd import synth
    return [p * 0.5 for p in synth.probes(2, seed=40)]


def _images(d):
    return sorted(os.path.relpath(p, d) for p in glob.glob(join(d, 'batch*', '**', '*.png'), recursive=True))


# The two routes march the same densities; their surfaces differ only by the fp32 summation order of occupancy and depth
# (torch's reduction against the kernel's wave sum): xyz by an ulp or so on some rays.  The NeRFactor networks take
# posenc(xyz) with frequencies up to 2^9, and precision = bf16 rounds those features to 8 bits: an ulp of xyz flips the
# rounding of a feature now and then, and the output jumps by a weight x bf16 ulp (1e-4 .. 1e-3), where the fp32-class
# render (bf16 hi / lo pairs, 16 bits) moves by ~1e-6.  So the fp32-class render is held to the route bound itself, the
# default bf16 render to what its operand rounding does to an ulp of input.
BOUNDS = {'fp32': dict(rgb=1e-4, image_frac=0.01, total_frac=0.01),
          'bf16': dict(rgb=1e-3, image_frac=0.05, total_frac=0.01)}


def _assert_images_agree(a_dir, b_dir, names, image_frac=0.01, total_frac=0.01, outlier_frac=1e-4):
    """Every image off by at most one LSB on at most `image_frac` of its pixels, all images together on at most
    `total_frac` of theirs.  Counted exclusion (the idiom of tests/test_gpu_reference_golden.py): pixels off by more than
    one LSB, at most `outlier_frac` of all, in OLAT images only — one light at grazing incidence turns a 1e-5 change of
    the surface into a few LSB of that light's image."""
    worst, off, total, outliers = 0., 0, 0, []
    for f in names:
        x = np.asarray(Image.open(join(a_dir, f))).astype(int)
        y = np.asarray(Image.open(join(b_dir, f))).astype(int)
        assert x.shape == y.shape, f
        diff = np.abs(x - y).reshape(x.shape[0], x.shape[1], -1).max(-1)
        outliers += [(f, int(d)) for d in diff[diff > 1]]
        px = diff > 0
        worst = max(worst, float(px.mean()))
        off, total = off + int(px.sum()), total + px.size
        assert px.mean() <= image_frac, (f, float(px.mean()))
    print("%d images: pixels off by one LSB or more %.4f %% of all, %.4f %% in the worst image; above one LSB: %s" % (
        len(names), 100. * off / max(total, 1), 100. * worst, outliers[:16]))
    assert off <= total_frac * total, (off, total)
    assert len(outliers) <= outlier_frac * total and all('/pred_rgb_olat/' in f for f, _ in outliers), outliers


@pytest.mark.parametrize('prec', PRECISIONS)
@pytest.mark.parametrize('name', ['nerfactor_microfacet', 'nerfactor'])
def test_direct_route_writes_what_the_disk_route_writes(runs, name, prec):
    ckpt, disk, direct = runs[name, prec]
    assert direct == disk + '_from_nerf' and basename(direct) == 'ckpt-1_from_nerf' and exists(direct + '.txt')
    a, b = _images(disk), _images(direct)
    assert len(glob.glob(join(direct, 'batch?????????'))) == 3
    common_names = sorted(set(a) & set(b))
    # the disk route also writes the ground-truth normal / visibility it read; the direct route has none
    assert sorted(set(a) - set(b)) == ['batch%09d/gt_%s.png' % (i, k) for i in range(3) for k in ('lvis', 'normal')]
    assert set(b) <= set(a)
    for k in ('pred_rgb', 'pred_albedo', 'pred_normal', 'pred_lvis', 'gt_alpha'):
        assert 'batch000000000/%s.png' % k in common_names, k
    assert sum(1 for f in common_names if '/pred_rgb_probes/' in f) == 3 * 2
    assert sum(1 for f in common_names if f.startswith('batch000000002/pred_rgb_olat/')) == 512
    assert not any(f.startswith('batch000000000/pred_rgb_olat/') for f in common_names)   # OLAT on the last view only
    bound = BOUNDS[prec]
    _assert_images_agree(disk, direct, common_names, image_frac=bound['image_frac'], total_frac=bound['total_frac'])


@pytest.mark.parametrize('prec', PRECISIONS)
@pytest.mark.parametrize('name', ['nerfactor_microfacet', 'nerfactor'])
def test_direct_batch_renders_what_the_disk_batch_renders(runs, name, prec, cuda):
    """In memory: Model.call on the batch datasets/nerf_shape.py reads from geometry_from_nerf's files and on the batch
    marched from the same rays — pred['rgb'] within the bound, the same foreground mask, and no ground-truth normal /
    visibility in the marched batch's outputs."""
    from nerfactor_amd.nerfactor import render_from_nerf as R
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.surface import march_surface, nerfactor_test_batch
    from nerfactor_amd.nerfactor.util import config as configutil
    ckpt = runs[name, prec][0]
    cfg = configutil.read_config(configutil.get_config_ini(ckpt))
    model = get_model_class(name)(cfg).to(cuda)
    configutil.restore_model(model, ckpt)
    model.to(cuda)
    nerf, nerf_cfg = R.load_nerf(runs['nerf_dir'], cuda)
    ds = get_dataset_class('nerf_shape')(cfg, 'test', device=cuda)
    metas = R.view_metadata(cfg, 'test')
    for meta, disk_batch in zip(metas, ds.build_pipeline(no_batch=True, no_shuffle=True)):
        id_, hw, rayo, rayd = R.view_rays(cfg, meta)
        rayo, rayd = dev(rayo, cuda), dev(rayd, cuda)
        with torch.no_grad():
            alpha, xyz = march_surface(nerf, rayo, rayd, nerf_cfg, bbox=R.parse_bbox(BBOX), occu_thres=float(runs['thres']))
        batch = nerfactor_test_batch(id_, hw, rayo, rayd, alpha, xyz)
        assert torch.equal(batch[2], disk_batch[2])
        assert torch.equal(batch[5] > 0, disk_batch[5] > 0), id_
        assert float((batch[5] - disk_batch[5]).abs().max()) <= 1. / 255 + 1e-7
        dx = (batch[6] - disk_batch[6]).abs()
        assert float(dx.max()) <= 1e-5
        pred_a, gt_a, _, vis_a = model(disk_batch, mode='test', relight_probes=True)
        pred_b, gt_b, _, vis_b = model(batch, mode='test', relight_probes=True)
        d_rgb = (pred_a['rgb'] - pred_b['rgb']).abs().max(1)[0]
        print("%s %s %s: xyz differs on %d of %d rays (max %.1e); rgb differs on %d (max %.1e)" % (
            name, prec, id_, int((dx.max(1)[0] > 0).sum()), dx.shape[0], float(dx.max()), int((d_rgb > 0).sum()),
            float(d_rgb.max())))
        assert float(d_rgb.max()) <= BOUNDS[prec]['rgb'], id_
        assert float((pred_a['rgb_probes'] - pred_b['rgb_probes']).abs().max()) <= BOUNDS[prec]['rgb'], id_
        assert sorted(gt_b) == ['alpha', 'rgb'] and 'gt_normal' not in vis_b and 'gt_lvis' not in vis_b
        assert 'gt_normal' in vis_a and 'gt_lvis' in vis_a


def test_direct_route_editing_variants(runs):
    from nerfactor_amd.nerfactor import render_from_nerf as R
    for name in ('nerfactor_microfacet', 'nerfactor'):
        ckpt, disk, direct = runs[name, 'bf16']
        out = R.main(['--ckpt=' + ckpt, '--trained_nerf=' + runs['nerf_dir'], '--scene_bbox=' + BBOX,
                      '--occu_thres=' + runs['thres'], '--tgt_albedo=rainbow', '--sv_axis_i=2', '--sv_axis_min=-1',
                      '--sv_axis_max=1', '--debug'])
        assert out == direct + '_rainbow' and exists(join(out, 'batch000000000', 'pred_albedo.png'))
        assert os.listdir(join(out, 'batch000000000', 'pred_rgb_olat'))    # --debug: one view, the last (OLAT)
        alb = np.asarray(Image.open(join(out, 'batch000000000', 'pred_albedo.png')))
        assert len(np.unique(alb.reshape(-1, 3), axis=0)) <= 8 + 1                     # 7 bands + background
    ckpt, disk, direct = runs['nerfactor', 'bf16']
    out = R.main(['--ckpt=' + ckpt, '--trained_nerf=' + runs['nerf_dir'], '--tgt_brdf=blue_rubber', '--debug'])
    assert out == direct + '_blue_rubber' and exists(join(out, 'batch000000000', 'pred_rgb.png'))


def test_two_ranks_write_the_images_of_one_rank(runs):
    """torch.distributed.run with two ranks on this one GPU (NFX_REHEARSAL=1: gloo collectives): each rank marches and
    renders its own contiguous ray range of every view; rank 0 writes what the one-process run writes."""
    ckpt = runs['nerfactor_microfacet', 'bf16'][0]
    run_dir = os.path.dirname(os.path.dirname(ckpt))

    def run(tag, launcher, env):
        dst = run_dir + '_' + tag
        shutil.copytree(run_dir, dst)
        shutil.copy(run_dir + '.ini', dst + '.ini')
        args = ['-m', 'nerfactor_amd.nerfactor.render_from_nerf', '--ckpt=' + join(dst, 'checkpoints', 'ckpt-1'),
                '--trained_nerf=' + runs['nerf_dir'], '--scene_bbox=' + BBOX, '--occu_thres=' + runs['thres']]
        res = subprocess.run(launcher + args, env=dict(os.environ, **env), cwd=os.getcwd(), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:]
        return join(dst, 'vis_test', 'ckpt-1_from_nerf')

    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    one = run('one', [sys.executable], {})
    two = run('two', [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                      '--master-addr=127.0.0.1', '--master-port=%d' % port], {'NFX_REHEARSAL': '1'})
    names = _images(one)
    assert names == _images(two) and len(names) > 512
    _assert_images_agree(one, two, names)
