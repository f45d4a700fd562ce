"""Generates tests/golden/reference_metrics.npz by running the REAL reference metric on the images of the metric tests.

    python tests/golden/make_reference_metrics_golden.py        (build container only: needs the reference checkout)

third_party/xiuminglib/xiuminglib/metric.py:PSNR is imported from the reference unmodified, the way
make_reference_merl_golden.py imports xiuminglib (absl from tests/golden/tf_shim, a stand-in module for the absent OpenCV
that no call here reaches), and called as PSNR('uint8')(im1, im2[, mask=]) on the uint8 images of
tests/image_metric_cases.images at every shape of the case list: H x W (the first channel), H x W x 1 and H x W x 3, with
and without the case's random mask.  xm.metric.SSIM calls tf.image.ssim and cannot run without TensorFlow: no SSIM is stored.

Keys: psnr_<H>x<W>_<hw|c1|c3>_<nomask|mask> -> float64 [3], one value per image of the case's batch.  Numbers only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('NERFACTOR_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(HERE, 'tf_shim'), REF, os.path.join(REF, 'nerfactor'), REPO]
sys.modules.setdefault('cv2', types.ModuleType('cv2'))

from third_party.xiuminglib import xiuminglib as xm  # noqa: E402

from tests import image_metric_cases as imc  # noqa: E402


def main():
    psnr = xm.metric.PSNR('uint8')
    out = {}
    for shape in imc.shapes():
        for C, layouts in ((1, ('hw', 'c1')), (3, ('c3',))):
            a, b, mask = imc.images(shape, 'uint8', C)
            for layout in layouts:
                for masked in (False, True):
                    vals = []
                    for i in range(a.shape[0]):
                        x, y = (a[i, :, :, 0], b[i, :, :, 0]) if layout == 'hw' else (a[i], b[i])
                        with np.errstate(divide='ignore'):
                            vals.append(psnr(x, y, mask=mask[i].astype(bool)) if masked else psnr(x, y))
                    out['psnr_%dx%d_%s_%s' % (shape + (layout, 'mask' if masked else 'nomask'))] = np.array(vals, np.float64)
    path = os.path.join(HERE, 'reference_metrics.npz')
    np.savez_compressed(path, **out)
    print(path, len(out), 'arrays')


if __name__ == '__main__':
    main()
