"""render_from_nerf without a GPU: its command line, the refusals that come before any GPU work, the cameras it marches
(the rays datasets/nerf_shape.py gives the same view), and the argument checks of nfx_nerf_surface_fwd."""
import ctypes
import os
import re
from os.path import join

import numpy as np
import pytest
import torch

from tests import synth_scene
from tests.conftest import ROOT


def _run_dir(tmp_path, name, **over):
    """A NeRFactor run in the trainvali layout: <outdir>.ini next to <outdir>/checkpoints/ (no checkpoint needed: the
    refusals come first)."""
    from nerfactor_amd.nerfactor.config import make_config
    outdir = tmp_path / 'out' / 'lr5e-3'
    os.makedirs(outdir / 'checkpoints', exist_ok=True)
    with open(str(outdir) + '.ini', 'w') as h:
        make_config(name, **over).write(h)
    return str(outdir / 'checkpoints' / 'ckpt-1')


def test_command_line():
    from nerfactor_amd.nerfactor import render_from_nerf as R
    a = R.parse_args(['--ckpt=/x/checkpoints/ckpt-3', '--trained_nerf=/n'])
    assert (a.split, a.occu_thres, a.mlp_chunk, a.scene_bbox, a.tgt_albedo, a.tgt_brdf, a.debug) == (
        'test', 0., 1 << 25, None, None, None, False)
    a = R.parse_args(['--ckpt=c', '--trained_nerf=n', '--scene_bbox=-1,1,-2,2,-3,3', '--occu_thres=0.2', '--split=val',
                      '--tgt_albedo=rainbow', '--sv_axis_i=2', '--color_correct_albedo', '--debug'])
    assert R.parse_bbox(a.scene_bbox) == [-1., 1., -2., 2., -3., 3.] and a.occu_thres == 0.2 and a.sv_axis_i == 2
    assert R.parse_bbox(None) is None
    with pytest.raises(ValueError, match='scene_bbox'):
        R.parse_bbox('1,2,3')
    with pytest.raises(SystemExit):
        R.parse_args(['--ckpt=c'])             # --trained_nerf is required


@pytest.mark.parametrize('name', ['nerfactor', 'nerfactor_microfacet'])
def test_shape_mode_nerf_is_refused_before_any_gpu_work(tmp_path, monkeypatch, name):
    from nerfactor_amd.nerfactor import render_from_nerf as R
    ckpt = _run_dir(tmp_path, name, shape_mode='nerf')
    touched = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: touched.append(1) or True)
    with pytest.raises(ValueError, match='geometry_from_nerf') as e:
        R.main(['--ckpt=' + ckpt, '--trained_nerf=' + str(tmp_path / 'no_nerf')])
    assert 'test.py' in str(e.value) and not touched


def test_scenes_without_ray_cameras_are_refused(tmp_path):
    from nerfactor_amd.nerfactor import render_from_nerf as R
    ckpt = _run_dir(tmp_path, 'nerfactor_mvs', shape_mode='finetune')
    with pytest.raises(ValueError, match='mvs_shape'):
        R.main(['--ckpt=' + ckpt, '--trained_nerf=' + str(tmp_path / 'no_nerf')])


def test_model_refuses_a_batch_without_surface_buffers_under_shape_mode_nerf():
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.surface import nerfactor_test_batch
    model = get_model_class('nerfactor_microfacet')(make_config('nerfactor_microfacet', shape_mode='nerf',
                                                                test_envmap_dir=''))
    n = 6
    batch = nerfactor_test_batch('test_000', (2, 3), torch.zeros(n, 3), torch.ones(n, 3), torch.ones(n),
                                 torch.zeros(n, 3))
    assert batch[7] is None and batch[8] is None and tuple(batch[5].shape) == (n, 1)
    assert batch[0] == ['test_000'] * n and batch[1].tolist() == [[2, 3]] * n and float(batch[4].abs().sum()) == 0.
    with pytest.raises(ValueError, match='geometry_from_nerf'):
        model(batch, mode='test')


def test_cameras_are_the_rays_of_the_surface_dataset(tmp_path):
    """The rays render_from_nerf marches are, bit for bit, the rayo / rayd of the batches datasets/nerf_shape.py yields
    for the same views (and what geometry_from_nerf marched at the same imh)."""
    from nerfactor_amd.nerfactor import render_from_nerf as R
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    data_root, nerf_root = synth_scene.write_scene(str(tmp_path), imh=12, imw=12, n_train=1, n_val=1, n_test=3)
    cfg = make_config('nerfactor', data_root=data_root, data_nerf_root=nerf_root, imh=8)
    metas = R.view_metadata(cfg, 'test')
    assert [os.path.basename(os.path.dirname(m)) for m in metas] == ['test_000', 'test_001', 'test_002']
    assert [os.path.basename(os.path.dirname(m)) for m in R.view_metadata(cfg, 'test', debug=True)] == ['test_002']
    ds = get_dataset_class('nerf_shape')(cfg, 'test', always_all_rays=True, device='cpu')
    batches = list(ds.build_pipeline(no_batch=True, no_shuffle=True))
    assert len(batches) == len(metas)
    for m, b in zip(metas, batches):
        id_, hw, rayo, rayd = R.view_rays(cfg, m)
        assert id_ == b[0][0] and hw == (8, 8) and tuple(b[1][0].tolist()) == hw
        np.testing.assert_array_equal(rayo, b[2].numpy())
        np.testing.assert_array_equal(rayd, b[3].numpy())


def test_surface_entry_point_is_declared_and_bound(nfx_lib):
    src = open(join(ROOT, 'include', 'nfx.h')).read()
    assert re.search(r'^NFX_API int nfx_nerf_surface_fwd\(', src, flags=re.M)
    assert 'nfx_nerf_surface_fwd' in nfx_lib.SIGNATURES
    assert hasattr(nfx_lib.lib, 'nfx_nerf_surface_fwd')


def test_surface_bad_arguments_return_errors_without_launching(nfx_lib):
    """Every check comes before the launch: these return NFX_EINVAL on a machine without a GPU as well."""
    lib, p = nfx_lib.lib, ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    ok = ctypes.cast(buf, p)

    def call(sigma, n, s, thres=0., alpha=ok, xyz=ok, depth=ok):
        return lib.nfx_nerf_surface_fwd(sigma, ok, ok, ok, n, s, thres, 1, alpha, xyz, depth, None, None)
    einval = -1
    assert call(ok, -1, 4) == einval                   # n < 0
    assert call(ok, 4, 0) == einval                    # no samples
    assert call(None, 4, 4) == einval                  # null input
    assert call(ok, 4, 4, alpha=None) == einval        # null output (only occu may be NULL)
    assert call(ok, 4, 4, depth=None) == einval
    assert call(ok, 4, 4, thres=float('nan')) == einval
    assert 'nfx_nerf_surface_fwd' in nfx_lib.last_error()
    assert call(None, 0, 4, alpha=None, xyz=None, depth=None) == 0   # nothing to do: no pointer is read
    from nerfactor_amd import ops
    with pytest.raises(nfx_lib.NfxError):
        ops.nerf_surface(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(4, 3))
