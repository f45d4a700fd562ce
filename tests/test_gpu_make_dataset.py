"""nerf_real.make_dataset with the resize kernel on the scene of tests/make_dataset_scene.py: its PNGs
are exactly the float32 restatement of the kernel on the decoded photographs through the truncating writer, within one level
on at most 0.5 % of the values of what the reference's driver wrote, and its JSON files are the reference's."""
from os.path import basename, join

import numpy as np
import pytest

from tests import make_dataset_scene as sc
from tests import resize_cases as rc

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-5
PNG_LEVELS, PNG_FRACTION = 1, 0.005


def test_driver_on_the_gpu_equals_restatement_and_reference(tmp_path, nfx_lib, cuda):
    from nerfactor_amd.data_gen.nerf_real import make_dataset
    from nerfactor_amd.data_gen.util import read_image
    scene_dir, outroot = sc.write(str(tmp_path / 'scene')), str(tmp_path / 'out')
    ret = make_dataset.main(['--scene_dir', scene_dir, '--outroot', outroot, '--h', str(sc.OUT_H), '--n_vali', str(sc.N_VALI),
                             '--bound_factor', str(sc.BOUND_FACTOR)])
    jsons, pngs = sc.read_dataset(outroot)
    want_jsons, want_pngs = sc.load_golden()
    worst = sc.compare_jsons(jsons, want_jsons)
    print('largest pose / angle difference from the reference:', worst)
    assert worst <= POSE_BOUND
    levels, fraction = sc.compare_pngs(pngs, want_pngs)
    print('kernel vs reference PNGs: largest level difference %d, fraction differing %.2e' % (levels, fraction))
    assert levels <= PNG_LEVELS and fraction <= PNG_FRACTION
    # bit for bit: the restatement on the same decoded bytes, an all-one alpha appended
    new_w = int(sc.IM_W / sc.IM_H * sc.OUT_H)
    restated = {}
    for i in range(sc.N_VIEWS):
        img = read_image(join(scene_dir, 'images', 'img_%d.jpg' % i))
        restated[i] = np.dstack((rc.quantize(rc.resize(img, sc.OUT_H, new_w)), np.full((sc.OUT_H, new_w, 1), 255, np.uint8)))
    for name, meta in jsons.items():
        if name.startswith(('train_', 'val_')):
            view = int(basename(meta['original_path'])[len('img_'):-len('.jpg')])
            assert np.array_equal(pngs[name.replace('metadata.json', 'rgba.png')], restated[view]), name
    for i, nn in enumerate(ret['nn']):
        assert np.array_equal(pngs['test_%03d/nn.png' % i], restated[nn]), i
