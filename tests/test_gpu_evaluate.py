"""The evaluate driver on the GPU: on the 24 x 24 run directory of tests/evaluate_scene.py it writes
both metrics.json files, the per-pair numbers are metrics.PSNR / SSIM('uint8') of the arrays it is documented to build, the
view without ground truth is counted as skipped, and a second run writes the same bytes."""
import json
from os.path import exists, join

import numpy as np
import pytest

from tests import image_metric_cases as imc
from tests.evaluate_scene import write_scene

pytestmark = pytest.mark.gpu


def test_evaluate_writes_the_metrics_of_the_metric_classes(nfx_lib, cuda, tmp_path, capsys):
    from nerfactor_amd import metrics
    from nerfactor_amd.nerfactor import evaluate
    scene = write_scene(str(tmp_path))
    path = evaluate.main(['--ckpt', scene['ckpt']])
    assert path == join(scene['vis_dir'], 'metrics.json')
    out = capsys.readouterr().out
    assert 'PSNR (dB)' in out and 'relight_city' in out and 'albedo' in out and path in out
    summary = json.load(open(path))
    per_view = json.load(open(join(scene['vis_dir'], 'batch000000000', 'metrics.json')))
    assert not exists(join(scene['vis_dir'], 'batch000000001', 'metrics.json'))
    assert {k: (v['n_views'], v['n_skipped']) for k, v in summary.items()} == {
        'rgb': (1, 1), 'albedo': (1, 1), 'relight': (1, 3), 'relight_city': (1, 1), 'relight_sunset': (0, 2)}
    psnr, ssim = metrics.PSNR('uint8'), metrics.SSIM('uint8')
    for key, (pred, gt, mask) in scene['expected'].items():
        want_psnr, want_ssim = psnr(pred, gt, mask=mask), ssim(pred, gt)
        assert per_view[key] == {'psnr': float('%.6f' % want_psnr), 'ssim': float('%.6f' % want_ssim),
                                 'n_px': 24 * 24 if mask is None else int(mask.sum())}
        assert summary[key]['psnr'] == per_view[key]['psnr'] and summary[key]['ssim'] == per_view[key]['ssim']
        # ... which are the float64 oracle's numbers: six decimals hide the 2^-40 quantum
        ref = imc.oracle64(pred, gt, 255., True, mask)
        assert abs(want_psnr - ref['psnr']) <= 4 * imc.MEASURED['psnr'] and abs(want_ssim - ref['ssim']) <= 4 * imc.MEASURED['ssim']
    # the classes take a batch and device tensors as well
    import torch
    pred, gt, _ = scene['expected']['rgb']
    both = psnr(torch.from_numpy(np.stack((pred, gt))).to(cuda), torch.from_numpy(np.stack((gt, gt))).to(cuda))
    assert both.shape == (2,) and both[0] == psnr(pred, gt) and both[1] == float('inf')
    pred, gt, mask = scene['expected']['albedo']
    assert psnr(pred, gt, mask=mask[..., None].astype(bool)) == psnr(pred, gt, mask=mask) != psnr(pred, gt)    # H x W x 1, logical
    assert ssim(gt[:, :, 0], gt[:, :, 0]) == 1.0 and ssim(gt[:, :, :1], gt[:, :, :1]) == 1.0
    first = open(path, 'rb').read(), open(join(scene['vis_dir'], 'batch000000000', 'metrics.json'), 'rb').read()
    evaluate.main(['--ckpt', scene['ckpt'], '--vis_dir', scene['vis_dir']])
    assert first == (open(path, 'rb').read(), open(join(scene['vis_dir'], 'batch000000000', 'metrics.json'), 'rb').read())
