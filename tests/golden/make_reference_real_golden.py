"""Generates tests/golden/reference_real.npz by running the REAL reference driver of real captures on a small scene.

    python tests/golden/make_reference_real_golden.py        (build container only: needs the reference checkout)

data_gen/nerf_real/make_dataset.py is imported from the reference unmodified (absl from tests/golden/tf_shim, a stand-in
module for the absent OpenCV that no call here reaches) and its main() runs with --h 12 --n_vali 2 --bound_factor 0.75 on the
scene of tests/make_dataset_scene.py, which this script writes: 7 cameras on a hemisphere and 48 x 64 JPEGs of uniform-random
uint8 noise, encoded with PIL.  Everything after the resize is the reference's own code: its pose conversion, gen_data,
recenter_poses, spherify_poses and its truncating PNG writer.

The one stand-in: the driver resizes with xm.img.resize(method='tf'), which is tf.image.resize(bilinear, antialias=True);
TensorFlow is not available and tf_shim refuses a real resize, so for this run xm.img.resize is bound to the float64
restatement of that filter (tests/resize_cases.resize64: the documented triangle filter applied in float64), returned as
float32 as TensorFlow returns it.  The PNGs are therefore the reference's writer on an exact filter, not TensorFlow's own
float32 arithmetic; the tests allow one level on at most 0.5 % of the values for that.

Keys: jpeg_<i> uint8 (the bytes of the scene's files), jsons (a JSON text: {path relative to the output root: the parsed
metadata.json or transforms_*.json}), png_names (a JSON list) and pngs uint8 [127, 12, 16, 4] (every rgba.png and nn.png)."""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('NERFACTOR_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(HERE, 'tf_shim'), REF, os.path.join(REF, 'nerfactor'), REPO]
sys.modules.setdefault('cv2', types.ModuleType('cv2'))

from third_party.xiuminglib import xiuminglib as xm  # noqa: E402

from tests import make_dataset_scene as scene  # noqa: E402
from tests import resize_cases as rc  # noqa: E402


def resize_stand_in(arr, new_h=None, new_w=None, method='tf'):
    assert method == 'tf', method
    h, w = arr.shape[:2]
    if new_h is None:
        new_h = int(h / w * new_w)
    if new_w is None:
        new_w = int(w / h * new_h)
    return rc.resize64(arr, new_h, new_w).astype(np.float32)


def main():
    xm.img.resize = resize_stand_in
    from data_gen.nerf_real import make_dataset as ref_driver
    jpegs = scene.encode_jpegs()
    with tempfile.TemporaryDirectory() as tmp:
        scene_dir, outroot = scene.write(os.path.join(tmp, 'scene'), jpegs), os.path.join(tmp, 'out')
        flags = ref_driver.FLAGS
        flags.scene_dir, flags.h, flags.n_vali, flags.bound_factor = scene_dir, scene.OUT_H, scene.N_VALI, scene.BOUND_FACTOR
        flags.outroot, flags.debug = outroot, False
        ref_driver.main(None)
        jsons, pngs = scene.read_dataset(outroot)
    assert sum(n.startswith('test_') and n.endswith('nn.png') for n in pngs) == 120
    names = sorted(pngs)
    out = {'jpeg_%d' % i: np.frombuffer(b, np.uint8) for i, b in enumerate(jpegs)}
    out['jsons'] = np.array(json.dumps(jsons, sort_keys=True))
    out['png_names'] = np.array(json.dumps(names))
    out['pngs'] = np.stack([pngs[n] for n in names], 0)
    np.savez_compressed(scene.GOLDEN, **out)
    print(scene.GOLDEN, os.path.getsize(scene.GOLDEN), 'bytes,', len(jsons), 'JSON files,', len(names), 'PNGs')


if __name__ == '__main__':
    main()
