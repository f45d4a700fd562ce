"""The dataset drivers on the CPU: nerf_real.make_dataset --device cpu on the scene of
tests/make_dataset_scene.py writes what the reference's own driver wrote (tests/golden/reference_real.npz), the directory
loads through datasets.nerf.Dataset, EXIF orientation is honoured, images of two sizes are refused; dtu_mvs.make_dataset
writes the closed-form poses of cameras built from known K, R, t and scale matrix."""
import json
from os.path import basename, join

import numpy as np
import pytest

from tests import make_dataset_scene as sc
from tests import resize_cases as rc

POSE_BOUND = 1e-5            # absolute; entries are O(1) (cameras on a unit sphere): about a hundred float32 ulps
PNG_LEVELS, PNG_FRACTION = 1, 0.005


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    from nerfactor_amd.data_gen.nerf_real import make_dataset
    root = tmp_path_factory.mktemp('real')
    scene_dir, outroot = sc.write(str(root / 'scene')), str(root / 'out')
    ret = make_dataset.main(['--scene_dir', scene_dir, '--outroot', outroot, '--h', str(sc.OUT_H), '--n_vali', str(sc.N_VALI),
                             '--bound_factor', str(sc.BOUND_FACTOR), '--device', 'cpu'])
    return scene_dir, outroot, ret


def test_layout_poses_split_and_neighbours_equal_the_reference(written):
    """Measured: the largest difference of any matrix entry or camera angle from the reference's is 0.0 (the same float32 and
    float64 operations in the same order)."""
    _, outroot, ret = written
    jsons, pngs = sc.read_dataset(outroot)
    want_jsons, want_pngs = sc.load_golden()
    worst = sc.compare_jsons(jsons, want_jsons)          # layout, every key, the split through original_path
    print('largest pose / angle difference from the reference:', worst)
    assert worst <= POSE_BOUND
    assert sum(n.startswith('test_') for n in pngs) == 120 and len(jsons) == 3 + 7 + 120
    assert ret['ind_vali'].tolist() == [0, 3] and ret['ind_train'].tolist() == [1, 2, 4, 5, 6]
    # nearest neighbours: the reference's nn.png is the image of one input view; ours must be the same view's
    by_view = {basename(want_jsons[n]['original_path']): want_pngs[n.replace('metadata.json', 'rgba.png')]
               for n in want_jsons if n.startswith(('train_', 'val_'))}
    views = ['img_%d.jpg' % i for i in range(sc.N_VIEWS)]
    for i, nn in enumerate(ret['nn']):
        assert np.array_equal(want_pngs['test_%03d/nn.png' % i], by_view[views[nn]]), i
    assert len(set(ret['nn'])) > 1


def test_pngs_within_one_level_of_the_reference(written):
    _, outroot, _ = written
    _, pngs = sc.read_dataset(outroot)
    _, want = sc.load_golden()
    worst, fraction = sc.compare_pngs(pngs, want)
    print('host filter vs reference PNGs: largest level difference %d, fraction differing %.2e' % (worst, fraction))
    assert worst <= PNG_LEVELS and fraction <= PNG_FRACTION
    assert all((p[:, :, 3] == 255).all() for p in pngs.values())


def test_float32_restatement_stays_under_the_cap(written):
    """What the GPU driver is held to: the float32 restatement of the kernel on the decoded photographs, quantised as the
    writer does, against the reference's float64 filter."""
    from nerfactor_amd.data_gen.util import read_image
    scene_dir, _, _ = written
    want_jsons, want = sc.load_golden()
    differ = total = 0
    for name, meta in want_jsons.items():
        if not name.startswith(('train_', 'val_')):
            continue
        img = read_image(join(scene_dir, 'images', basename(meta['original_path'])))
        got = rc.quantize(rc.resize(img, sc.OUT_H, int(sc.IM_W / sc.IM_H * sc.OUT_H)))
        d = np.abs(got.astype(np.int32) - want[name.replace('metadata.json', 'rgba.png')][:, :, :3].astype(np.int32))
        assert d.max() <= PNG_LEVELS
        differ, total = differ + int((d != 0).sum()), total + d.size
    print('float32 restatement vs reference PNGs: fraction differing %.2e' % (differ / total))
    assert differ / total <= PNG_FRACTION


def test_directory_loads_through_the_nerf_dataset(written):
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    _, outroot, _ = written
    cfg = make_config('nerf', data_root=outroot, outroot=join(outroot, 'trained'), imh=sc.OUT_H, n_rays_per_step=16)
    tr = get_dataset_class('nerf')(cfg, 'train', device='cpu')
    assert tr.get_n_views() == 5
    batch = next(iter(tr.build_pipeline(no_batch=True, seed=0)))
    assert batch[2].shape == (16, 3) and batch[4].shape == (16, 3) and batch[1][0].tolist() == [12, 16]
    assert float(batch[4].min()) >= 0. and float(batch[4].max()) <= 1.
    te = get_dataset_class('nerf')(cfg, 'test', device='cpu')
    assert te.get_n_views() == 120
    b = next(iter(te.build_pipeline(no_batch=True, no_shuffle=True)))
    assert b[0][0] == 'test_000' and b[2].shape == (12 * 16, 3)


def test_exif_orientation_is_honoured(tmp_path):
    from PIL import Image

    from nerfactor_amd.data_gen.util import load_and_resize, read_image
    img = sc.noise_images()[0]
    exif = Image.Exif()
    exif[0x0112] = 6                                     # the camera was held rotated: display turned 90 degrees clockwise
    plain, turned = str(tmp_path / 'plain.jpg'), str(tmp_path / 'turned.JPG')
    Image.fromarray(img).save(plain, quality=95)
    Image.fromarray(img).save(turned, quality=95, exif=exif)
    a, b = read_image(plain), read_image(turned)
    assert a.shape == (48, 64, 3) and b.shape == (64, 48, 3)
    assert np.array_equal(b, np.rot90(a, -1))
    imgs, factor = load_and_resize([turned], 16, 'cpu')
    assert imgs.shape == (1, 16, 12, 4) and factor == 4.


def test_images_of_two_sizes_are_refused(tmp_path):
    from PIL import Image

    from nerfactor_amd.data_gen.nerf_real import make_dataset
    scene_dir = sc.write(str(tmp_path / 'scene'))
    Image.fromarray(sc.noise_images()[0][:40]).save(join(scene_dir, 'images', 'img_3.jpg'))
    with pytest.raises(ValueError, match='varying sizes'):
        make_dataset.main(['--scene_dir', scene_dir, '--outroot', str(tmp_path / 'out'), '--h', '12', '--device', 'cpu'])


def test_extension_is_matched_in_any_case_and_debug_takes_four(tmp_path):
    from nerfactor_amd.data_gen.nerf_real import make_dataset
    scene_dir = sc.write(str(tmp_path / 'scene'), ext='JPG')
    ret = make_dataset.main(['--scene_dir', scene_dir, '--outroot', str(tmp_path / 'out'), '--h', '12', '--device', 'cpu', '--debug'])
    assert sorted(ret['ind_train'].tolist() + ret['ind_vali'].tolist()) == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------------- DTU
def _dtu_scene(root, n=5, h=24, w=32):
    """cameras.npz and image/<i>.png from known K, R, t and scale matrix -> the closed-form OpenGL poses [n, 3, 4] and
    focal lengths in the normalised frame."""
    import os

    from PIL import Image
    os.makedirs(join(root, 'image'))
    rng = np.random.default_rng(7)
    scale_mat = np.diag([3., 3., 3., 1.])
    scale_mat[:3, 3] = [0.5, -0.25, 1.]
    cams, poses, focals = {}, [], []
    for i in range(n):
        lng = 0.9 * i
        centre = np.array([6. * np.cos(lng), 6. * np.sin(lng), 2. + 0.3 * i]) + scale_mat[:3, 3]
        fwd = scale_mat[:3, 3] - centre
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0., 0., 1.])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd], 0)                       # world to camera, computer-vision axes
        t = -R @ centre
        K = np.array([[50. + i, 0.3, w / 2 + 0.5], [0., 52. + i, h / 2 - 0.25], [0., 0., 1.]])
        world_mat = np.eye(4)
        world_mat[:3] = 1.7 * K @ np.hstack((R, t[:, None]))        # a projection matrix has no scale
        cams['world_mat_%d' % i], cams['scale_mat_%d' % i] = world_mat, scale_mat
        c = (centre - scale_mat[:3, 3]) / 3.
        flip = np.diag([1., -1., -1.])
        poses.append(np.hstack((flip @ R.T @ flip, (flip @ c)[:, None])))
        focals.append((K[0, 0] + K[1, 1]) / 2)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.int64).astype(np.uint8)).save(join(root, 'image', '%d.png' % i))
    np.savez(join(root, 'cameras.npz'), **cams)
    return cams, np.array(poses), np.array(focals)


def test_dtu_decomposition_and_poses_by_construction(tmp_path):
    """pose_from_mats against the closed form to 1e-12; the written matrices against the closed-form poses sent through the
    same normalisation (measured: 0.0, the same operations on the same float32 poses)."""
    from nerfactor_amd.data_gen import util
    from nerfactor_amd.data_gen.dtu_mvs import make_dataset
    from nerfactor_amd.mesh import decompose_projection
    root = str(tmp_path / 'scan')
    cams, poses, focals = _dtu_scene(root)
    for i in range(len(poses)):
        K, R, t = decompose_projection(cams['world_mat_%d' % i][:3])
        assert (np.diag(K) > 0).all() and abs(np.linalg.det(R) - 1.) < 1e-12 and np.abs(np.tril(K, -1)).max() == 0.
        pose = make_dataset.pose_from_mats(cams['world_mat_%d' % i], cams['scale_mat_%d' % i], 2., (12, 16))
        assert np.abs(pose[:, :4] - poses[i]).max() <= 1e-12 and pose[:, 4].tolist() == [12., 16., pytest.approx(focals[i] / 2., abs=1e-12)]
    outroot = str(tmp_path / 'out')
    ret = make_dataset.main(['--scene_dir', root, '--outroot', outroot, '--h', '12', '--n_vali', '2', '--device', 'cpu'])
    # the written poses: the closed-form ones through the same normalisation
    hwf = np.tile(np.array([[12.], [16.], [0.]]), (len(poses), 1, 1))
    hwf[:, 2, 0] = focals / 2.
    want, _ = util.spherify_poses(util.recenter_poses(np.concatenate([poses, hwf], 2).astype(np.float32)))
    jsons, pngs = sc.read_dataset(outroot)
    order = [('val', 0), ('train', 0), ('val', 1), ('train', 1), ('train', 2)]          # views 0 and 2 are held out
    assert ret['ind_vali'].tolist() == [0, 2]
    worst = 0.
    for view, (mode, k) in enumerate(order):
        meta = jsons['%s_%03d/metadata.json' % (mode, k)]
        assert basename(meta['original_path']) == '%d.png' % view and (meta['imh'], meta['imw']) == (12, 16)
        worst = max(worst, float(np.abs(sc.matrix_of(meta)[:3] - want[view][:, :4]).max()))
        assert abs(meta['cam_angle_x'] - 2 * np.arctan2(8., np.float32(focals[0] / 2.))) <= POSE_BOUND
    print('largest difference of a written DTU pose from the closed form:', worst)
    assert worst <= POSE_BOUND
    # the images went through the host filter and the truncating writer
    from PIL import Image

    from nerfactor_amd.nerfactor.util.light import resize_antialias
    src = np.array(Image.open(join(root, 'image', '1.png'))).astype(np.float32) / np.float32(255)
    assert np.array_equal(pngs['train_000/rgba.png'][:, :, :3], util.quantize_uint8(resize_antialias(src, new_h=12)))
    with open(join(outroot, 'transforms_test.json')) as h:
        assert len(json.load(h)['frames']) == 120
