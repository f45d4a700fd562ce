"""The readers' opt-in ini key resize_on_device: nerf_shape at [16, 24, 512] buffers and imh = 8 gives
the restatement's bits for xyz, normal, lvis, alpha and rgb with the key on, and the present host values with it off."""
from os.path import join

import numpy as np
import pytest

from tests import resize_cases as rc
from tests import synth_scene

pytestmark = pytest.mark.gpu


def _view(cfg):
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    ds = get_dataset_class('nerf_shape')(cfg, 'vali', device='cpu')
    id_, rayo, rayd, rgb, alpha, xyz, normal, lvis = ds._process_example_precache(ds.files[0])
    return id_, {'rgb': rgb, 'alpha': alpha, 'xyz': xyz, 'normal': normal, 'lvis': lvis}


def test_reader_with_the_key_on_and_off(tmp_path, nfx_lib, cuda):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets.nerf import load_rgba, resize
    root = str(tmp_path)
    data_root, nerf_root = synth_scene.write_scene(root, imh=16, imw=24, n_train=1, n_val=1, n_test=1)
    kw = dict(data_root=data_root, data_nerf_root=nerf_root, outroot=join(root, 'out'), imh=8, n_rays_per_step=32)
    id_, on = _view(make_config('shape', resize_on_device='True', **kw))
    _, off = _view(make_config('shape', **kw))
    rgba = load_rgba(join(data_root, id_, 'rgba.png'))
    raw = {'rgb': rgba[:, :, :3], 'alpha': rgba[:, :, 3], 'xyz': np.load(join(nerf_root, id_, 'xyz.npy')),
           'normal': np.load(join(nerf_root, id_, 'normal.npy')), 'lvis': np.load(join(nerf_root, id_, 'lvis.npy'))}
    assert raw['lvis'].shape == (16, 24, 512)

    def finish(name, a):                                  # what the reader does after the resize
        if name == 'normal':
            a = a / np.maximum(np.linalg.norm(a, axis=2, keepdims=True), 1e-12)
        if name == 'lvis':
            a = np.clip(a, 0, 1)
        return a.astype(np.float32)

    for name, a in raw.items():
        a = a.astype(np.float32)
        restated = rc.resize(a.reshape(16, 24, -1), 8, 12).reshape((8, 12) + a.shape[2:])
        assert on[name].shape == restated.shape == off[name].shape, name
        assert np.array_equal(on[name].view(np.int32), finish(name, restated).view(np.int32)), name
        assert np.array_equal(off[name].view(np.int32), finish(name, resize(a, 8)).view(np.int32)), name
    assert not np.array_equal(on['lvis'], off['lvis'])          # two filters: the key is not a no-op
