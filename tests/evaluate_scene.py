"""A 24 x 24 run directory for the evaluate driver, written with PIL: what test.py leaves for two views (pred_rgb.png,
pred_albedo.png, two probe images each), a vis_vali epoch for the albedo scales, and ground truth for the first view only
(and not for its second probe).  A helper, not a test.

write_scene(root) -> {'ckpt', 'vis_dir', 'pred_rgb', 'expected': {pair: (pred uint8, gt uint8, mask or None)}}: `expected`
restates what evaluate.py documents for every pair, from the arrays that were written."""
import json
import os
from os.path import join

import numpy as np
from PIL import Image

H = W = 24
PROBES = ('city', 'sunset')


def _img(rng, smooth, channels=3):
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.4 * np.sin(0.3 * yy[..., None] + smooth + np.arange(channels)) * np.cos(0.2 * xx[..., None])
    return (np.clip(base + 0.05 * rng.standard_normal((H, W, channels)), 0, 1) * 255).astype(np.uint8)


def _alpha():
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.hypot(yy - 11.5, xx - 11.5)
    return (np.clip((10. - r) / 3., 0, 1) * 255).astype(np.uint8)         # a soft-edged disc


def _save(arr, *path):
    os.makedirs(os.path.dirname(join(*path)), exist_ok=True)
    Image.fromarray(arr).save(join(*path))


def _quantise(x):
    return (np.clip(x, 0., 1.) * 255.).astype(np.uint8)


def write_scene(root, white_bg=True):
    rng = np.random.default_rng(11)
    data_root, run = join(root, 'data'), join(root, 'out', 'lr1e-3')
    ckpt = join(run, 'checkpoints', 'ckpt-2')
    vis_dir = join(run, 'vis_test', 'ckpt-2')
    envmaps = join(root, 'envmaps')
    os.makedirs(envmaps)
    os.makedirs(run)
    for name in PROBES:
        open(join(envmaps, name + '.hdr'), 'wb').close()          # the driver only lists them
    with open(run + '.ini', 'w') as h:
        h.write("[DEFAULT]\ndata_root = %s\nwhite_bg = %s\ntest_envmap_dir = %s\n" % (data_root, white_bg, envmaps))
    alpha = _alpha()
    written = {}
    for i, view in enumerate(('test_000', 'test_001')):
        bdir = join(vis_dir, 'batch%09d' % i)
        os.makedirs(bdir)
        with open(join(bdir, 'metadata.json'), 'w') as h:
            json.dump({'id': view}, h)
        for name, arr in (('pred_rgb.png', _img(rng, 0.1 * i)), ('pred_albedo.png', _img(rng, 1. + i)),
                          ('pred_rgb_probes/0000.png', _img(rng, 2. + i)), ('pred_rgb_probes/0001.png', _img(rng, 3. + i))):
            _save(arr, bdir, name)
            written[(i, name)] = arr
    # ground truth of view 0: rgba.png at the prediction's size, rgba_city.png at twice the size, albedo.png; no rgba_sunset.png
    gt_rgb = np.dstack((_img(rng, 0.05), alpha))
    gt_albedo = np.dstack((_img(rng, 1.05), alpha))
    gt_city = np.asarray(Image.fromarray(np.dstack((_img(rng, 2.05), alpha))).resize((2 * W, 2 * H), Image.BILINEAR))
    _save(gt_rgb, data_root, 'test_000', 'rgba.png')
    _save(gt_city, data_root, 'test_000', 'rgba_city.png')
    _save(gt_albedo, data_root, 'test_000', 'albedo.png')
    # the validated epoch compute_rgb_scales reads, and its view's ground-truth albedo
    vdir = join(run, 'vis_vali', 'epoch000000002', 'batch000000000')
    os.makedirs(vdir)
    with open(join(vdir, 'metadata.json'), 'w') as h:
        json.dump({'id': 'val_000'}, h)
    _save(_img(rng, 1.2), vdir, 'pred_albedo.png')
    _save(np.dstack((_img(rng, 1.25), alpha)), data_root, 'val_000', 'albedo.png')

    # ---- what the driver is documented to score
    from nerfactor_amd.nerfactor.datasets.nerf import resize
    from nerfactor_amd.nerfactor.test import compute_rgb_scales
    bg = 1. if white_bg else 0.
    f32 = lambda a: a.astype(np.float32) / 255.

    def on_bg(rgba):
        return rgba[:, :, :3] * rgba[:, :, 3:] + bg * (1. - rgba[:, :, 3:])

    expected = {'rgb': (written[(0, 'pred_rgb.png')], _quantise(on_bg(f32(gt_rgb))), None),
                'relight_city': (written[(0, 'pred_rgb_probes/0000.png')], _quantise(on_bg(resize(f32(gt_city), H))), None)}
    scales = compute_rgb_scales(ckpt, alpha_thres=0.9).numpy()
    fg = f32(gt_albedo)[:, :, 3] > 0.9
    pred = np.clip(f32(written[(0, 'pred_albedo.png')]) ** 2.2 * scales[None, None, :], 0., 1.) ** (1 / 2.2)
    gt = np.clip(f32(gt_albedo)[:, :, :3], 0., 1.) ** (1 / 2.2)
    expected['albedo'] = (_quantise(np.where(fg[..., None], pred, 1.)), _quantise(np.where(fg[..., None], gt, 1.)), fg.astype(np.uint8))
    return {'ckpt': ckpt, 'vis_dir': vis_dir, 'pred_rgb': written[(0, 'pred_rgb.png')], 'expected': expected}
