"""The image metrics without a GPU: the two CPU restatements of tests/image_metric_cases.py against
SciPy, against each other and against the reference's own PSNR; the argument contract of metrics.PSNR / SSIM; the C-ABI's
refusals, reached with null pointers so that nothing is launched; and the pairing and summary logic of the evaluate driver
on a directory written with PIL, with the scoring function replaced by the float64 oracle."""
import json
import os

import numpy as np
import pytest
from PIL import Image

from tests import image_metric_cases as imc
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_metrics.npz')
MEASURED = imc.MEASURED       # measured on the GPU; the emulation has the kernel's bits, so the same figures hold here


def test_weights_and_tile(nfx_lib):
    from nerfactor_amd import ops
    assert tuple(ops.IMAGE_METRICS_TILE) == imc.TILE and ops.IMAGE_METRICS_SCALE == imc.SCALE
    assert ops.IMAGE_METRICS_WEIGHTS == imc.weights()
    g = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    np.testing.assert_allclose(ops.IMAGE_METRICS_WEIGHTS, g / g.sum(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(np.outer(imc.weights(), imc.weights()), imc.weights_2d(), rtol=1e-14, atol=0)
    header = open(os.path.join(ROOT, 'include', 'nfx.h')).read()
    assert '#define NFX_IMAGE_METRICS_TILE_Y %d\n' % imc.TILE[0] in header and '#define NFX_IMAGE_METRICS_TILE_X %d\n' % imc.TILE[1] in header


def test_oracle_fields_equal_scipy_correlate1d():
    from scipy.ndimage import correlate1d
    g = np.asarray(imc.weights())
    for shape in imc.shapes():
        a, b, _ = imc.images(shape, 'uint8', 1)
        x, y = a[0, :, :, 0].astype(np.float64), b[0, :, :, 0].astype(np.float64)
        for f, got in zip((x, y, x * y, x * x + y * y), imc.oracle_fields(x, y)):
            want = correlate1d(correlate1d(f, g, axis=0), g, axis=1)[5:-5, 5:-5]        # the VALID part
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_emulation_against_the_oracle():
    worst = {'ssim': 0., 'map': 0., 'psnr': 0.}
    for shape, dtype, C, luma, mask_kind in imc.all_cases():
        for i in range(3):
            emu, ref = imc.reference(shape, dtype, C, luma, mask_kind, i)
            worst['ssim'] = max(worst['ssim'], abs(emu['ssim'] - ref['ssim']))
            worst['map'] = max(worst['map'], float(np.abs(emu['map'] - ref['map']).max()))
            if mask_kind == 'zero':
                assert np.isnan(emu['psnr']) and np.isnan(ref['psnr']) and emu['totals'][6] == 0
            elif ref['mse'] > 0:
                worst['psnr'] = max(worst['psnr'], abs(emu['psnr'] - ref['psnr']))
            else:
                assert emu['psnr'] == float('inf') and emu['mse'] == 0.
    print('emulate vs oracle64:', worst)
    for k, v in worst.items():
        assert v <= 4 * MEASURED[k], (k, v)


def test_psnr_oracle_equals_the_reference():
    """tests/golden/reference_metrics.npz holds xm.metric.PSNR('uint8') of the reference itself on the case images
    (make_reference_metrics_golden.py).  xm.metric.SSIM needs TensorFlow (tf.image.ssim) and cannot be run where the
    fixtures are made: SSIM is pinned to the formula of DESIGN.md section 3.12 — tf.image.ssim's documented defaults — and
    not to a run of the reference."""
    gold = np.load(GOLD)
    n = 0
    for shape in imc.shapes():
        for C, layouts in ((1, ('hw', 'c1')), (3, ('c3',))):
            a, b, mask = imc.images(shape, 'uint8', C)
            for layout in layouts:
                for masked in (False, True):
                    want = gold['psnr_%dx%d_%s_%s' % (shape + (layout, 'mask' if masked else 'nomask'))]
                    for i in range(3):
                        for fn in (imc.oracle64, imc.emulate):
                            got = fn(a[i], b[i], 255., True, mask[i] if masked else None)['psnr']
                            if np.isinf(want[i]):
                                assert got == want[i]
                            else:
                                # oracle: the same float64 formula; emulation: within the 2^-40 quantum of the integer sum
                                assert abs(got - want[i]) <= (1e-12 if fn is imc.oracle64 else 4 * MEASURED['psnr']), (shape, layout, masked, i)
                            n += 1
    assert n == 6 * 3 * 2 * 3 * 2 and len(gold.files) == 36


def test_metric_classes_argument_contract(nfx_lib):
    """Everything here is decided before an image goes to the device."""
    from nerfactor_amd import metrics
    assert metrics.PSNR('uint8').drange == 255. and metrics.SSIM('float32').drange == 1. and metrics.PSNR(np.uint8).dtype == np.uint8
    with pytest.raises(NotImplementedError):
        metrics.PSNR('int32')
    with pytest.raises(NotImplementedError):
        metrics.SSIM('float64')
    im = np.zeros((12, 12, 3), np.uint8)
    with pytest.raises(AssertionError, match='different from what was specified'):
        metrics.PSNR('uint8')(im.astype(np.float32), im.astype(np.float32))
    with pytest.raises(AssertionError, match='different from what was specified'):
        metrics.SSIM('float32')(im, im)
    with pytest.raises(AssertionError, match='dynamic range'):
        f = np.zeros((12, 12), np.float32)
        f[0, 0] = 1.5
        metrics.PSNR('float32')(f, f)
    with pytest.raises(AssertionError, match='same shape'):
        metrics.PSNR('uint8')(im, im[:, :11])
    with pytest.raises(AssertionError, match='1 or 3 channels'):
        metrics.PSNR('uint8')(np.zeros((12, 12, 2), np.uint8), np.zeros((12, 12, 2), np.uint8))
    with pytest.raises(ValueError, match='5D'):
        metrics.SSIM('uint8')(np.zeros((1, 1, 12, 12, 3), np.uint8), np.zeros((1, 1, 12, 12, 3), np.uint8))
    with pytest.raises(NotImplementedError, match='MS-SSIM'):
        metrics.SSIM('uint8')(im, im, multiscale=True)
    x = np.array([-0.5, 0., 0.999 / 255, 1. / 255, 0.5, 254.999 / 255, 1., 2.], np.float32)
    want = (np.clip(x, 0, 1) * 255).astype(np.uint8)
    assert metrics.to_uint8(x).tolist() == want.tolist() == [0, 0, 0, 1, 127, 254, 255, 255]
    import torch
    assert metrics.to_uint8(torch.from_numpy(x)).tolist() == want.tolist()


def test_capi_refuses_bad_arguments_without_a_gpu(nfx_lib):
    """Null images: every refusal below is decided before a pointer is read or anything is launched."""
    lib = nfx_lib.lib

    def call(batch=1, h=12, w=12, c=3, max_val=255., luma=1, is_float=0):
        return lib.nfx_image_metrics(None, None, is_float, batch, h, w, c, max_val, luma, None, None, None, None, None, 0, None)
    for kw, text in (({'h': 10}, '10 x 12'), ({'w': 10}, '12 x 10'), ({'c': 2}, 'c = 2'), ({'c': 4}, 'c = 4'), ({'max_val': 0.}, 'max_val = 0'),
                     ({'max_val': -1.}, 'max_val = -1'), ({'max_val': float('nan')}, 'max_val'), ({'h': 2048, 'w': 2049}, '4196352 pixels'),
                     ({'batch': 0}, 'batch = 0'), ({'batch': 65536, 'c': 1}, 'batch = 65536'), ({'batch': 21846, 'luma': 0}, 'batch = 21846'),
                     ({'is_float': 2}, 'is_float = 2'), ({}, 'null pointer')):
        assert call(**kw) == -1 and text in nfx_lib.last_error(), (kw, nfx_lib.last_error())
    size = lib.nfx_image_metrics_workspace_bytes
    assert size(1, 11, 11, 3, 1) == 32 and size(1, 11, 11, 3, 0) == 96 and size(2, 27, 43, 1, 0) == 2 * 2 * 2 * 32
    assert size(1, 2048, 2048, 3, 0) == 3 * 128 * 64 * 32
    assert size(1, 10, 11, 3, 1) == size(1, 11, 11, 2, 1) == size(0, 11, 11, 3, 1) == size(1, 2048, 2049, 1, 1) == size(21846, 11, 11, 3, 0) == 0
    assert size(21845, 11, 11, 3, 0) == 65535 * 32 and size(65535, 11, 11, 3, 1) == 65535 * 32


# ---------------------------------------------------------------------------------------------- the driver
def _oracle_score(pred, gt, mask):
    out = []
    for i in range(pred.shape[0]):
        r = imc.oracle64(pred[i], gt[i], 255., True, None if mask is None else mask[i])
        out.append({'psnr': r['psnr'], 'ssim': r['ssim'], 'n_px': int(pred[i].shape[0] * pred[i].shape[1] if mask is None else mask[i].sum())})
    return out


def test_evaluate_pairs_and_summarises(nfx_lib, tmp_path):
    from nerfactor_amd.nerfactor import evaluate
    from tests.evaluate_scene import write_scene
    scene = write_scene(str(tmp_path))
    summary, path = evaluate.evaluate(scene['ckpt'], score_fn=_oracle_score)
    assert path == os.path.join(scene['vis_dir'], 'metrics.json') and json.load(open(path)) == summary
    # view 0 has ground truth for everything but the second probe, view 1 for nothing
    assert {k: (v['n_views'], v['n_skipped']) for k, v in summary.items()} == {
        'rgb': (1, 1), 'albedo': (1, 1), 'relight': (1, 3), 'relight_city': (1, 1), 'relight_sunset': (0, 2)}
    assert summary['relight_sunset']['psnr'] is None and summary['relight'] == dict(summary['relight_city'], n_skipped=3)
    per_view = json.load(open(os.path.join(scene['vis_dir'], 'batch000000000', 'metrics.json')))
    assert sorted(per_view) == ['albedo', 'relight_city', 'rgb']
    assert not os.path.exists(os.path.join(scene['vis_dir'], 'batch000000001', 'metrics.json'))
    # the numbers are the oracle's on the arrays the driver is documented to build
    for key in ('rgb', 'relight_city', 'albedo'):
        pred, gt, mask = scene['expected'][key]
        want = imc.oracle64(pred, gt, 255., True, mask)
        assert per_view[key]['psnr'] == float('%.6f' % want['psnr']) and per_view[key]['ssim'] == float('%.6f' % want['ssim'])
        assert per_view[key]['n_px'] == (24 * 24 if mask is None else int(mask.sum()))
        assert summary[key]['psnr'] == per_view[key]['psnr']
    assert 0 < per_view['albedo']['n_px'] < 24 * 24
    # the vis_dir argument, --debug (first view only) and byte-identical output of a second run
    first = open(path, 'rb').read(), open(os.path.join(scene['vis_dir'], 'batch000000000', 'metrics.json'), 'rb').read()
    s2, _ = evaluate.evaluate(scene['ckpt'], vis_dir=scene['vis_dir'], debug=True, score_fn=_oracle_score)
    assert s2['rgb'] == dict(summary['rgb'], n_skipped=0)
    evaluate.evaluate(scene['ckpt'], score_fn=_oracle_score)
    assert first == (open(path, 'rb').read(), open(os.path.join(scene['vis_dir'], 'batch000000000', 'metrics.json'), 'rb').read())
    table = evaluate.format_table(summary)
    assert 'relight_city' in table and 'PSNR' in table and len(table.splitlines()) == 6
    # every existing file of the view is as it was
    assert json.load(open(os.path.join(scene['vis_dir'], 'batch000000000', 'metadata.json'))) == {'id': 'test_000'}
    assert np.array_equal(np.asarray(Image.open(os.path.join(scene['vis_dir'], 'batch000000000', 'pred_rgb.png'))), scene['pred_rgb'])
