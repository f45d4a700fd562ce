"""The occupancy grid without a GPU: the drivers' flags and their defaults (off = grid None all the way down to the density
passes), the refusals that come before any GPU work, the box derived from the cameras, and the new kernels' metadata
(no scratch; one wave per SIMD for the list form of the density kernel)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import synth_scene
from tests.conftest import ROOT

GRID_FLAGS = ['--occupancy_grid=96', '--grid_margin=0.5', '--grid_dilate=2', '--grid_probes=3', '--grid_check=5']


@pytest.mark.parametrize('driver', ['geometry_from_nerf', 'render_from_nerf'])
def test_flags_and_defaults(driver):
    import importlib
    D = importlib.import_module('nerfactor_amd.nerfactor.' + driver)
    req = ['--trained_nerf=n'] + (['--out_root=o'] if driver == 'geometry_from_nerf' else ['--ckpt=c'])
    a = D.parse_args(req)
    assert (a.occupancy_grid, a.grid_margin, a.grid_dilate, a.grid_probes, a.grid_check) == (0, 10., 2, 4, 0)
    a = D.parse_args(req + GRID_FLAGS)
    assert (a.occupancy_grid, a.grid_margin, a.grid_dilate, a.grid_probes, a.grid_check) == (96, 0.5, 2, 3, 5)


def test_grid_off_is_none_all_the_way_down(monkeypatch):
    """--occupancy_grid 0: no grid is baked and every density pass of both drivers' marches gets grid = None."""
    from nerfactor_amd.nerfactor import geometry_from_nerf as G, occupancy
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.surface import march_surface
    args = G.parse_args(['--trained_nerf=n', '--out_root=o'])
    baked = []
    monkeypatch.setattr(occupancy.OccupancyGrid, 'bake', classmethod(lambda *a, **k: baked.append(1)))
    assert occupancy.from_arguments(args, SimpleNamespace(tuned=False), None, '/nonexistent') is None and not baked
    seen = []

    class Recorder:
        """The NeRF model's march interface on the CPU, recording the grid every density pass receives."""
        tuned = True

        def gen_z(self, near, far, n, n_rays, **kw):
            return torch.linspace(near, far, n)[None].expand(n_rays, n).contiguous()

        def accumulate_sigma(self, sigma, z, d):
            return torch.full_like(sigma, 1. / sigma.shape[1])

        def gen_z_fine(self, z, w, n_fine, perturb=False):
            return torch.cat((z, z[:, :1].expand(-1, n_fine)), 1)

        def eval_sigma(self, o, d, z, use_fine=False, bbox=None, grid='missing'):
            seen.append(grid)
            return torch.zeros_like(z)

        def eval_sigma_normal(self, o, d, z, bbox=None):
            return torch.zeros_like(z), torch.zeros(z.shape + (3,))

    cfg = make_config('nerf')
    m = Recorder()
    o, d = torch.zeros((5, 3)), torch.tensor([[0., 0., 1.]]).expand(5, 3).contiguous()
    G.compute_depth_and_normal(m, o, d, cfg, mlp_chunk=2 * 448)
    G.compute_light_visibility(m, o + 1., torch.ones((5, 3)), cfg, light_h=2, mlp_chunk=448 * 8)
    monkeypatch.setattr('nerfactor_amd.ops.nerf_surface', lambda sigma, z, o, d, **kw: (
        torch.zeros(o.shape[0]), torch.zeros((o.shape[0], 3)), None, None))
    march_surface(m, o, d, cfg)
    assert len(seen) > 6 and all(g is None for g in seen), seen


def test_refusals_before_any_gpu_work(tmp_path, monkeypatch):
    from nerfactor_amd.nerfactor import geometry_from_nerf as G, occupancy
    touched = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: touched.append(1) or True)
    for flags, msg in ((['--occupancy_grid=-4'], 'occupancy_grid'), (['--occupancy_grid=8', '--grid_dilate=-1'], 'grid_dilate'),
                       (['--occupancy_grid=8', '--grid_probes=0'], 'grid_probes'),
                       (['--occupancy_grid=8', '--grid_check=-2'], 'grid_check')):
        with pytest.raises(ValueError, match=msg):
            G.main(['--trained_nerf=' + str(tmp_path), '--out_root=' + str(tmp_path)] + flags)
    assert not touched
    # render_from_nerf refuses them before it opens the device as well
    from nerfactor_amd.nerfactor import render_from_nerf as R
    from nerfactor_amd.nerfactor.config import make_config
    outdir = tmp_path / 'out' / 'lr5e-3'
    os.makedirs(outdir / 'checkpoints')
    with open(str(outdir) + '.ini', 'w') as h:
        make_config('nerfactor_microfacet', shape_mode='finetune').write(h)
    with pytest.raises(ValueError, match='grid_dilate'):
        R.main(['--ckpt=' + str(outdir / 'checkpoints' / 'ckpt-1'), '--trained_nerf=n', '--occupancy_grid=8',
                '--grid_dilate=-3'])
    assert not touched
    # the grid object itself
    with pytest.raises(ValueError, match='res'):
        occupancy.OccupancyGrid.bake(SimpleNamespace(tuned=True), [-1, 1] * 3, 0)
    with pytest.raises(ValueError, match='dilate'):
        occupancy.OccupancyGrid.bake(SimpleNamespace(tuned=True), [-1, 1] * 3, 8, dilate=-1)
    # the bake's limits come before the probe lattice is allocated (a model without parameters would fail after them)
    for kw, msg in ((dict(res=2048), 'res'), (dict(res=8, probes=17), 'probes'), (dict(res=512, probes=4), r'2\^30'),
                    (dict(res=64, dilate=17), 'dilate')):
        with pytest.raises(ValueError, match=msg):
            occupancy.OccupancyGrid.bake(SimpleNamespace(tuned=True), [-1, 1] * 3, **kw)
    with pytest.raises(ValueError, match=r'2\^30'):
        G.main(['--trained_nerf=' + str(tmp_path), '--out_root=' + str(tmp_path), '--occupancy_grid=1024'])
    assert not touched
    with pytest.raises(ValueError, match='box'):
        occupancy.OccupancyGrid([1, -1, 0, 1, 0, 1], 8, {'fine_': torch.zeros(16, dtype=torch.int32)})


def test_runtime_shaped_networks_are_refused():
    from nerfactor_amd.nerfactor import occupancy
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    model = get_model_class('nerf')(make_config('nerf', mlp_width='64', enc_depth='4'))
    assert not model.tuned
    args = SimpleNamespace(occupancy_grid=8, grid_margin=0., grid_dilate=1, grid_probes=2, grid_check=0)
    with pytest.raises(NotImplementedError, match='runtime-shaped'):
        occupancy.from_arguments(args, model, [-1, 1] * 3, '/nonexistent')
    with pytest.raises(NotImplementedError, match='runtime-shaped'):
        occupancy.OccupancyGrid.bake(model, [-1, 1] * 3, 8)
    grid = SimpleNamespace()        # eval_sigma refuses before it touches the grid or the device
    with pytest.raises(NotImplementedError, match='runtime-shaped'):
        model.eval_sigma(torch.zeros((2, 3)), torch.ones((2, 3)), torch.ones((2, 4)), grid=grid)


def test_box_from_the_cameras(tmp_path):
    from nerfactor_amd.nerfactor.occupancy import cameras_box
    data_root, _ = synth_scene.write_scene(str(tmp_path), imh=4, imw=4, n_train=3, n_val=1, n_test=2)
    box = cameras_box(data_root)
    assert len(box) == 6 and all(box[2 * k] < box[2 * k + 1] for k in range(3))
    # the unit sphere the cameras look at lies inside their box
    assert all(box[2 * k] <= -1. and box[2 * k + 1] >= 1. for k in range(3)), box
    with pytest.raises(ValueError, match='scene_bbox'):
        cameras_box(str(tmp_path / 'nothing'))


@pytest.fixture(scope='module')
def rows(nfx_lib):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_metadata
    if not os.path.exists(os.path.join(kernel_metadata.LLVM, 'llvm-objdump')):
        pytest.skip("no llvm-objdump")
    return kernel_metadata.kernels(os.path.join(ROOT, 'nerfactor_amd', 'libnfx.so'))


def test_new_kernels_use_no_scratch_and_the_list_kernel_runs_one_wave_per_simd(rows):
    def one(sub):
        found = [r for r in rows if sub in r['name']]
        assert len(found) == 1, (sub, [r['name'] for r in found])
        return found[0]
    full, lst = one('nerf_sigma_v6_kernel('), one('nerf_sigma_v6_list_kernel(')
    for r in (lst, one('occ::occupancy_kernel'), one('occ::dilate_kernel'), one('count_kernel<nfx::occ::Select>'),
              one('write_kernel<nfx::occ::Select>')):
        assert r['private_segment_fixed_size'] == 0 and not r['vgpr_spill_count'] and not r['sgpr_spill_count'], r
    # the fp32-class density kernel, whose list form gained a flat output, still runs without scratch
    assert one('nerf_sigma_x3_kernel<false>')['private_segment_fixed_size'] == 0
    # one wave per SIMD: four waves per workgroup, one workgroup per CU (its register file and LDS: the full kernel's)
    assert lst['max_flat_workgroup_size'] == full['max_flat_workgroup_size'] == 256
    assert lst['vgpr_count'] > 256 and lst['group_segment_fixed_size'] == full['group_segment_fixed_size']
