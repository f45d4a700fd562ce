"""The occupancy grid of the density marches on the GPU: the list form of the density kernel
against the every-sample kernel (bit for bit), the selection and the bake against torch restatements of nfx.h's rules, and
the marches — light visibility, depth + normals, march_surface, both drivers — bit-identical with and without a grid baked
from the NeRF fitted to a unit sphere, check mode included."""
import os
from os.path import join

import numpy as np
import pytest
import torch
from PIL import Image

from tests import common, synth_scene
from tests.golden import golden_inputs as gi
from tests.test_gpu_render_from_nerf import fill_nerf, synth_scene_probes

pytestmark = pytest.mark.gpu
BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
BBOX = '-1.5,1.5,-1.5,1.5,-1.5,1.5'
GRID = dict(res=64, probes=4, margin=10., dilate=2)      # the drivers' defaults at R = 64


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def _bits_eq(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rays(cuda, n, s, seed):
    g = torch.Generator().manual_seed(seed)
    rayo = (torch.rand((n, 3), generator=g) * 2 - 1) * 3.
    rayd = torch.nn.functional.normalize(-rayo + torch.randn((n, 3), generator=g) * 0.3, dim=1)
    z = torch.sort(torch.rand((n, s), generator=g) * 5. + 0.5, 1)[0]
    return rayo.to(cuda), rayd.to(cuda), z.to(cuda)


def _nerf(cuda, nets, precision='bf16'):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    torch.manual_seed(0)
    model = get_model_class('nerf')(make_config('nerf', precision=precision))
    fill_nerf(model, nets)
    return model.to(cuda)


# ---------------------------------------------------------------------------------------------- list kernel
@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@pytest.mark.parametrize('weights', ['glorot', 'fitted'])
@pytest.mark.parametrize('n,blocks', [(97, None), (97, 3), (1800, None)])
def test_list_kernel_equals_the_full_kernel(nfx_lib, cuda, prec, weights, n, blocks):
    """n = 97: 3977 samples, ragged last tiles of every kernel; blocks = 3 (option nerf_blocks) makes each workgroup of the
    list kernel walk several tiles of its persistent loop, and so does n = 1800 (73 800 samples: more tiles than the
    default 256 workgroups) at the default grid."""
    from nerfactor_amd import ops
    nets = common.nerf_nets(seed=3) if weights == 'glorot' else gi.trained_nerf_nets()
    blob = ops.pack_nerf_geom_weights(*common.nerf_layers(nets[1]), prec=prec).to(cuda)
    s = 41
    rayo, rayd, z = _rays(cuda, n, s, seed=7)
    if weights == 'fitted':
        rayo, rayd = rayo / 3., rayd            # through the fitted sphere
    full = ops.nerf_sigma_fwd(rayo, rayd, z, blob, prec)
    g = torch.Generator().manual_seed(11)
    lists = {'empty': torch.zeros(0, dtype=torch.int64), 'one': torch.tensor([n * s - 1]), 'first': torch.tensor([0]),
             'tile_plus_one': torch.arange(257) * 13 % (n * s),
             'random': torch.nonzero(torch.rand(n * s, generator=g) < 0.3)[:, 0],
             'all': torch.arange(n * s)}
    for name, idx in lists.items():
        idx = torch.unique(idx)
        lst = torch.zeros(n * s, dtype=torch.int32)
        lst[:idx.numel()] = idx.int()
        lst, count = lst.to(cuda), torch.tensor([idx.numel()], dtype=torch.int32, device=cuda)
        out = torch.full((n, s), -1234.5, device=cuda)
        if blocks is None:
            ops.nerf_sigma_fwd_list(rayo, rayd, z, blob, lst, count, out, prec)
        else:
            with nfx_lib.option('nerf_blocks', blocks):
                ops.nerf_sigma_fwd_list(rayo, rayd, z, blob, lst, count, out, prec)
        listed = torch.zeros(n * s, dtype=torch.bool, device=cuda)
        listed[idx.to(cuda)] = True
        listed = listed.view(n, s)
        assert _bits_eq(out[listed], full[listed]), (name, prec, weights)
        assert bool((out[~listed] == -1234.5).all()), (name, "an unlisted sample was written")


# ---------------------------------------------------------------------------------------------- selection
def _torch_select(rayo, rayd, z, bits, res, box, bbox):
    """nfx.h's rule, restated in torch fp32 on the CPU: a bool [N, S] of the listed samples."""
    rayo, rayd, z, bits = rayo.cpu(), rayd.cpu(), z.cpu(), bits.cpu()
    p = rayo[:, None, :] + rayd[:, None, :] * z[:, :, None]
    lo, hi = torch.tensor(box[0::2]), torch.tensor(box[1::2])
    inside = ((p >= lo) & (p <= hi)).all(-1)
    cell = ((p - lo) / (hi - lo) * float(res)).clamp(min=0).to(torch.int64).clamp(max=res - 1)
    c = (cell[..., 0] * res + cell[..., 1]) * res + cell[..., 2]
    c = torch.where(inside, c, torch.zeros_like(c))
    on = ((bits.to(torch.int64)[c >> 5] >> (c & 31)) & 1).bool()
    listed = ~inside | on
    if bbox is not None:
        blo, bhi = torch.tensor(bbox[0::2]), torch.tensor(bbox[1::2])
        listed &= ~((p < blo) | (p > bhi)).any(-1)
    return listed


@pytest.mark.parametrize('bbox', [None, [-0.9, 1.2, -1.1, 0.7, -1.4, 1.0]])
def test_select_equals_its_torch_restatement(nfx_lib, cuda, bbox):
    from nerfactor_amd import ops
    res, box = 16, [-1.0, 1.0, -1.25, 0.75, -1.0, 1.5]
    n, s = 300, 37
    rayo, rayd, z = _rays(cuda, n, s, seed=5)
    rayo = rayo / 2.                                # most samples inside the box, some outside
    # samples exactly on cell faces and on the box's faces: axis-aligned rays through lattice coordinates
    m = 40
    face = torch.tensor([box[0] + (box[1] - box[0]) * k / res for k in range(res + 1)])
    o = torch.stack((face[torch.arange(m) % (res + 1)], torch.full((m,), box[2]), torch.full((m,), box[4])), 1)
    d = torch.tensor([[0., 0., 1.]]).expand(m, 3)
    zz = torch.tensor([box[5] - box[4]]) * torch.arange(s)[None].float() / (s - 1) * torch.ones((m, 1))
    rayo = torch.cat((rayo, o.to(cuda)))
    rayd = torch.cat((rayd, d.to(cuda)))
    z = torch.cat((z, zz.to(cuda))).contiguous()
    n = rayo.shape[0]
    g = torch.Generator().manual_seed(2)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, ((res ** 3 + 31) // 32,), generator=g, dtype=torch.int64).int().to(cuda)
    out = torch.full((n, s), 7.5, device=cuda)
    out, lst, count = ops.occgrid_select(rayo, rayd, z, bits, res, box, bbox, out=out)
    want = _torch_select(rayo, rayd, z, bits, res, box, bbox).view(-1)
    k = int(count.item())
    assert 0 < k < n * s
    assert torch.equal(lst[:k].cpu().long(), torch.nonzero(want)[:, 0]), "the list is the ascending listed samples"
    flat = out.view(-1).cpu()
    assert bool((flat[~want] == 0.).all()) and bool((flat[want] == 7.5).all())
    # a grid with every bit set lists every sample in the bbox; an empty one only those outside the box
    for fill in (-1, 0):
        b = torch.full_like(bits, fill)
        _, lst2, count2 = ops.occgrid_select(rayo, rayd, z, b, res, box, bbox)
        want2 = _torch_select(rayo, rayd, z, b, res, box, bbox).view(-1)
        assert torch.equal(lst2[:int(count2.item())].cpu().long(), torch.nonzero(want2)[:, 0])


# ---------------------------------------------------------------------------------------------- bake
def _torch_bake(sigma, res, probes, margin, dilate):
    m = res * probes
    s = sigma.cpu().view(res, probes, res, probes, res, probes)
    occ = ((s > -margin) | torch.isnan(s)).any(5).any(3).any(1).float()
    if dilate:
        occ = torch.nn.functional.max_pool3d(occ[None, None], 2 * dilate + 1, stride=1, padding=dilate)[0, 0]
    flat = occ.reshape(-1).bool()
    flat = torch.cat((flat, torch.zeros((-flat.numel()) % 32, dtype=torch.bool)))
    words = (flat.view(-1, 32).long() << torch.arange(32)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).int()


@pytest.mark.parametrize('res,probes,margin,dilate', [(9, 2, 0., 0), (9, 2, 0.5, 1), (12, 1, 0., 2), (5, 3, -0.2, 1)])
def test_bake_equals_its_torch_restatement(nfx_lib, cuda, res, probes, margin, dilate):
    from nerfactor_amd import ops
    m = res * probes
    g = torch.Generator().manual_seed(res * 7 + dilate)
    sigma = torch.randn(m ** 3, generator=g) - 2.4          # sparse: a few cells have a probe above the threshold
    bits = ops.occgrid_bake(sigma.to(cuda), res, probes, margin, dilate)
    want = _torch_bake(sigma, res, probes, margin, dilate)
    assert torch.equal(bits.cpu(), want)
    assert 0 < int(want.ne(0).sum())


def test_bake_probes_the_lattice_of_the_header(nfx_lib, cuda):
    """OccupancyGrid.bake's probe rays put sample (a, b, c) at lo + (idx + 0.5) / M (hi - lo) per axis."""
    from nerfactor_amd.nerfactor.occupancy import probe_rays
    box = [-1., 2., 0., 1., -3., -1.]
    rayo, rayd, z = probe_rays(box, 3, 2, cuda)
    p = (rayo[:, None, :] + rayd[:, None, :] * z[None, :, None]).view(6, 6, 6, 3).double().cpu()
    t = (torch.arange(6).double() + 0.5) / 6
    for k in range(3):
        axis = box[2 * k] + t * (box[2 * k + 1] - box[2 * k])
        got = p.select(3, k)
        line = got[:, 0, 0] if k == 0 else got[0, :, 0] if k == 1 else got[0, 0, :]
        assert torch.allclose(line, axis, atol=1e-6)


# ---------------------------------------------------------------------------------------------- the marches, fitted NeRF
@pytest.fixture(scope='module')
def fitted(nfx_lib, cuda):
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid
    model = _nerf(cuda, gi.trained_nerf_nets())
    grid = OccupancyGrid.bake(model, BOX, **GRID)
    return model, grid


def _fraction(grid, what):
    seen, evaluated = grid.take_counts()
    frac = evaluated / seen
    print("%s: occupancy grid evaluated %d of %d density samples (%.4f)" % (what, evaluated, seen, frac))
    assert 0 < frac < 1, what
    return frac


def test_light_visibility_with_the_grid_is_bit_identical(fitted, cuda):
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    model, grid = fitted
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), torch.nn.functional.normalize(dev(rayd, cuda), dim=1, eps=1e-12)
    with torch.no_grad():
        occu, depth, normal = G.compute_depth_and_normal(model, o, d, cfg)
        hit = torch.nonzero(occu.clamp(0, 1) > 0)[:, 0][::8]
        surf = (o[hit] + d[hit] * depth[hit, None]).contiguous()
        nrm = normal[hit].contiguous()
        grid.take_counts()
        want = G.compute_light_visibility(model, surf, nrm, cfg, light_h=8)
        got = G.compute_light_visibility(model, surf, nrm, cfg, light_h=8, grid=grid)
    assert surf.shape[0] >= 32
    common.assert_same_bits(want, got, 'lvis with the occupancy grid')
    _fraction(grid, 'shadow rays')


@pytest.mark.parametrize('bbox', [None, BOX])
def test_depth_and_normal_with_the_grid_are_bit_identical(fitted, cuda, bbox):
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    model, grid = fitted
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), torch.nn.functional.normalize(dev(rayd, cuda), dim=1, eps=1e-12)
    grid.take_counts()
    with torch.no_grad():
        want = G.compute_depth_and_normal(model, o, d, cfg, bbox=bbox)
        got = G.compute_depth_and_normal(model, o, d, cfg, bbox=bbox, grid=grid)
    for a, b, name in zip(want, got, ('occu', 'depth', 'normal')):
        common.assert_same_bits(a, b, name + ' with the occupancy grid')
    _fraction(grid, 'depth + normal (coarse pass)')


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_march_surface_with_the_grid_is_bit_identical(nfx_lib, cuda, fitted, precision):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid
    from nerfactor_amd.nerfactor.surface import march_surface
    model, grid = fitted
    if precision == 'fp32':
        model = _nerf(cuda, gi.trained_nerf_nets(), 'fp32')
        grid = OccupancyGrid.bake(model, BOX, **GRID)
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), dev(rayd, cuda)
    grid.take_counts()
    with torch.no_grad():
        want = march_surface(model, o, d, cfg, full=True)
        got = march_surface(model, o, d, cfg, full=True, grid=grid)
        chunked = march_surface(model, o, d, cfg, full=True, grid=grid, mlp_chunk=320 * 100)   # ragged chunks of 100 rays
    for a, b, c, name in zip(want, got, chunked, ('alpha', 'xyz', 'occu', 'depth')):
        common.assert_same_bits(a, b, name + ' with the occupancy grid')
        common.assert_same_bits(a, c, name + ' with the occupancy grid, chunked')
    _fraction(grid, 'march_surface ' + precision)


def test_check_mode(fitted, cuda, monkeypatch):
    """An empty grid over the sphere skips samples with a density: check mode raises with their count.  The baked grid
    passes the same check, and every K-th pass of EACH network is checked."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid, OccupancyMiss
    from nerfactor_amd.nerfactor.surface import march_surface
    model, baked = fitted
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), dev(rayd, cuda)
    empty = OccupancyGrid(BOX, GRID['res'], {k: torch.zeros_like(v) for k, v in baked.bits.items()}, check_every=1)
    with torch.no_grad(), pytest.raises(OccupancyMiss, match=r'coarse network\): [1-9]\d* skipped samples'):
        march_surface(model, o, d, cfg, grid=empty)
    checked = []
    verify = OccupancyGrid.verify
    monkeypatch.setattr(OccupancyGrid, 'verify', staticmethod(lambda a, b, pref: checked.append(pref) or verify(a, b, pref)))
    sound = OccupancyGrid(BOX, GRID['res'], baked.bits, check_every=2)
    with torch.no_grad():
        march_surface(model, o, d, cfg, grid=sound, mlp_chunk=320 * 256)         # 4 chunks: 4 passes per network
    assert sound._passes == {'coarse_': 4, 'fine_': 4}
    assert sorted(checked) == ['coarse_'] * 2 + ['fine_'] * 2


@pytest.mark.parametrize('march', ['march_surface', 'light_visibility'])
def test_check_mode_checks_the_fine_network_at_an_even_period(fitted, cuda, march):
    """A sound coarse grid and an empty fine one, K = 2: the marches alternate coarse and fine passes, and check mode
    still compares the fine network's passes with the full pass."""
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid, OccupancyMiss
    from nerfactor_amd.nerfactor.surface import march_surface
    model, baked = fitted
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o, d = dev(rayo, cuda), torch.nn.functional.normalize(dev(rayd, cuda), dim=1, eps=1e-12)
    bits = {'coarse_': baked.bits['coarse_'], 'fine_': torch.zeros_like(baked.bits['fine_'])}
    grid = OccupancyGrid(BOX, GRID['res'], bits, check_every=2)
    with torch.no_grad(), pytest.raises(OccupancyMiss, match=r'fine network\): [1-9]\d* skipped samples'):
        if march == 'march_surface':
            march_surface(model, o, d, cfg, grid=grid, mlp_chunk=320 * 256)
        else:
            occu, depth, normal = G.compute_depth_and_normal(model, o, d, cfg)
            hit = torch.nonzero(occu.clamp(0, 1) > 0)[:, 0][::8]
            G.compute_light_visibility(model, (o[hit] + d[hit] * depth[hit, None]).contiguous(), normal[hit].contiguous(),
                                       cfg, light_h=8, grid=grid, mlp_chunk=320 * 2048)


def test_grid_refuses_runtime_shaped_networks(nfx_lib, cuda, fitted):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid
    _, grid = fitted
    model = get_model_class('nerf')(make_config('nerf', mlp_width='64', enc_depth='4')).to(cuda)
    assert not model.tuned
    o = torch.zeros((4, 3), device=cuda)
    d = torch.ones((4, 3), device=cuda)
    z = torch.linspace(1, 2, 8, device=cuda)[None].expand(4, 8).contiguous()
    with pytest.raises(NotImplementedError, match='runtime-shaped'):
        model.eval_sigma(o, d, z, grid=grid)
    with pytest.raises(NotImplementedError, match='runtime-shaped'):
        OccupancyGrid.bake(model, BOX, 8)


# ---------------------------------------------------------------------------------------------- the drivers
@pytest.fixture(scope='module')
def scene(tmp_path_factory, nfx_lib, cuda):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.util import light as L
    root = str(tmp_path_factory.mktemp('occupancy'))
    data_root, _ = synth_scene.write_scene(root, imh=24, imw=24, n_train=1, n_val=1, n_test=2)

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
    torch.manual_seed(1)
    brdf_ckpt = save('brdf', join(root, 'out_brdf', 'lr1e-2'), get_model_class('brdf')(make_config('brdf', data_root=merl)),
                     data_root=merl)
    probes = join(root, 'probes')
    os.makedirs(probes)
    for i, p in enumerate(synth_scene_probes()):
        L.write_hdr(p, join(probes, 'p%d.hdr' % i))
    over = dict(data_root=data_root, data_nerf_root=join(root, 'surf'), imh=24, shape_mode='finetune',
                shape_model_ckpt='none', brdf_model_ckpt=brdf_ckpt, test_envmap_dir=probes)
    torch.manual_seed(2)
    ckpt = save('nerfactor_microfacet', join(root, 'out_nfm', 'lr5e-3'),
                get_model_class('nerfactor_microfacet')(make_config('nerfactor_microfacet', **over)), **over)
    return {'root': root, 'nerf_dir': nerf_dir, 'ckpt': ckpt}


GRID_FLAGS = ['--occupancy_grid=64', '--grid_check=1']     # a skipped sample with a density raises, naming it


@pytest.mark.parametrize('box', ['bbox', 'cameras'])
def test_geometry_from_nerf_with_the_grid_writes_the_same_files(scene, box, capsys):
    from nerfactor_amd.nerfactor import geometry_from_nerf
    bb = ['--scene_bbox=' + BBOX] if box == 'bbox' else []
    base = ['--trained_nerf=' + scene['nerf_dir'], '--imh=24', '--occu_thres=0.05', '--light_h=8'] + bb
    plain = geometry_from_nerf.main(base + ['--out_root=' + join(scene['root'], 'geo_plain_' + box)])
    capsys.readouterr()
    grid = geometry_from_nerf.main(base + ['--out_root=' + join(scene['root'], 'geo_grid_' + box)] + GRID_FLAGS)
    log = capsys.readouterr().out
    assert len(plain) == len(grid) >= 3
    for a, b in zip(plain, grid):
        for f in ('lvis.npy', 'xyz.npy', 'normal.npy'):
            x, y = np.load(join(a, f)), np.load(join(b, f))
            assert x.tobytes() == y.tobytes(), (b, f)
        for f in ('alpha.png', 'xyz.png', 'normal.png', 'lvis.png'):
            assert np.array_equal(np.asarray(Image.open(join(a, f))), np.asarray(Image.open(join(b, f)))), (b, f)
    fracs = [float(line.rsplit('(', 1)[1].rstrip(')')) for line in log.splitlines() if 'occupancy grid evaluated' in line]
    print(log)
    assert len(fracs) == len(grid) and all(0 < f < 1 for f in fracs), fracs


def test_render_from_nerf_with_the_grid_renders_the_same_images(scene, capsys):
    from nerfactor_amd.nerfactor import render_from_nerf
    base = ['--ckpt=' + scene['ckpt'], '--trained_nerf=' + scene['nerf_dir'], '--scene_bbox=' + BBOX, '--occu_thres=0.05']
    plain = render_from_nerf.main(base)
    images = {}
    for root, _, files in os.walk(plain):
        for f in files:
            if f.endswith('.png'):
                images[os.path.relpath(join(root, f), plain)] = np.asarray(Image.open(join(root, f)))
    import shutil
    moved = plain + '_plain'
    shutil.move(plain, moved)
    capsys.readouterr()
    grid = render_from_nerf.main(base + GRID_FLAGS)
    log = capsys.readouterr().out
    assert grid == plain and len(images) > 4
    for rel, img in images.items():
        assert np.array_equal(img, np.asarray(Image.open(join(grid, rel)))), rel
    fracs = [float(line.rsplit('(', 1)[1].rstrip(')')) for line in log.splitlines() if 'occupancy grid evaluated' in line]
    print(log)
    assert len(fracs) == 2 and all(0 < f < 1 for f in fracs), fracs
