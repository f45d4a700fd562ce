"""Generates tests/golden/reference_sphere.npz by running the REAL reference sphere renderer and MERL coordinate code.

    python tests/golden/make_reference_sphere_golden.py        (build container only: needs the reference checkout)

brdf/renderer.py:SphereRenderer and brdf/merl/merl.py:MERL are imported from the reference unmodified; the prior is the
reference's models/brdf.py on tests/golden/tf_shim (the NumPy stand-in for TensorFlow of the other generators) with the
seeded glorot weights of golden_inputs.brdf_net().  OpenCV is not installed: the one call the reference makes here,
cv2.LUT in xiuminglib's gamma_correct, is a table lookup and is stood in for by `table[im]`.

Scenes: (ims, spp) = (16, 1) 'a' and (6, 4) 'b', envmap_h = None (16 x 32 lights; any other value resizes with OpenCV),
probes 'point' x 40 and 'white'.  Both scenes have an EVEN number of samples per side: with an odd number the centre
column is exactly coplanar with the view direction and phi_d sits on the 0 / pi wrap, where the reference's own value
is decided by rounding."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('NERFACTOR_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(HERE, 'tf_shim'), REF, os.path.join(REF, 'nerfactor'), REPO]

cv2 = types.ModuleType('cv2')
cv2.LUT = lambda im, table: table[im]
sys.modules.setdefault('cv2', cv2)

import tensorflow as tf  # noqa: E402  (the shim)
from nerfactor.util import io as ioutil  # noqa: E402
from nerfactor.models.brdf import Model as BrdfModel  # noqa: E402
from brdf.renderer import SphereRenderer, load_light  # noqa: E402
from brdf.merl.merl import MERL  # noqa: E402

from tests.golden import golden_inputs as gi  # noqa: E402

SCENES = {'a': (16, 1), 'b': (6, 4)}
PROBES = {'point': 40., 'white': 1.}
Z_ROW = 1     # the latent code of golden_inputs.latent_codes() the prior is rendered with


def prior(tmp):
    root = os.path.join(tmp, 'merl_npz')
    os.makedirs(root)
    for name in gi.BRDF_NAMES:
        open(os.path.join(root, 'train_%s.npz' % name), 'wb').close()
    cfg = ioutil.read_config(os.path.join(REF, 'nerfactor', 'config', 'brdf.ini'))
    cfg.set('DEFAULT', 'data_root', root)
    model = BrdfModel(cfg)
    net = gi.brdf_net()
    for part in ('brdf_mlp', 'brdf_out'):
        for layer, (k, b) in zip(model.net[part].layers, net[part]):
            layer.set_weights([k, b])
    return model


def main():
    out = {}
    merl = MERL()
    cslice_rusink = merl.get_characterstic_slice_rusink()
    out['cslice_rusink'] = cslice_rusink
    for name, inten in PROBES.items():
        out['light_' + name] = load_light(name, envmap_inten=inten)
    z = gi.latent_codes()[Z_ROW]
    out['prior_z'] = z
    with tempfile.TemporaryDirectory() as tmp:
        model = prior(tmp)
        for s, (ims, spp) in SCENES.items():
            rows = rusink = None
            for name, inten in PROBES.items():
                r = SphereRenderer(name, tmp, envmap_inten=inten, envmap_h=None, ims=ims, spp=spp)
                fg, lvis = r.is_fg, r.lvis.astype(bool)
                if rusink is None:
                    out[s + '_is_fg'] = fg
                    out['cam_loc'] = np.asarray(r.cam.loc, dtype=np.float64)
                    out[s + '_xyz'], out[s + '_normal'] = r.xyz[fg], r.normal[fg]
                    out[s + '_lvis'] = np.packbits(lvis[fg], axis=None)
                    full = MERL.dir2rusink(r.ldir, r.vdir)
                    rusink = full[lvis]
                    out[s + '_rusink'] = rusink.astype(np.float32)
                    out[s + '_rusink_sum'] = np.where(lvis[..., None], full, 0.).sum(2)[fg]
                    # the reference's test set: the slice's 90 x 90 coordinates, then the front-lit rows (float32 on disk)
                    coords = np.vstack((cslice_rusink.reshape(-1, 3), rusink)).astype(np.float32)
                    zs = np.tile(z[None, :], (coords.shape[0], 1)).astype(np.float32)
                    pred, _ = model._eval_brdf_at(tf.convert_to_tensor(zs), tf.convert_to_tensor(coords))
                    pred = np.asarray(pred)
                    n_c = 90 * 90
                    cimg = MERL.characteristic_slice_as_img(pred[:n_c].reshape(90, 90))
                    if 'prior_cslice' in out:
                        assert np.array_equal(out['prior_cslice_img'], cimg)
                    out['prior_cslice'], out['prior_cslice_img'] = pred[:n_c].reshape(90, 90), cimg
                    rows = pred[n_c:]
                    out[s + '_prior_rows'] = rows[:, 0]
                    print(s, 'foreground samples', int(fg.sum()), 'front-lit rows', rusink.shape[0],
                          'min distance of phi_d to the wrap %.3e' % min(rusink[:, 0].min(), np.pi - rusink[:, 0].max()))
                else:
                    assert np.array_equal(out[s + '_is_fg'], fg) and np.array_equal(rusink, MERL.dir2rusink(r.ldir, r.vdir)[lvis])
                key = s + '_' + name
                out[key + '_lcontrib_sum'] = r.lcontrib.sum(2)[fg]
                analytic = np.zeros_like(r.lcontrib)
                analytic[lvis] = (0.1 + np.cos(rusink[:, 1]) ** 8)[:, None]
                out[key + '_render_analytic'] = r.render(analytic)
                brdf = np.zeros_like(r.lcontrib)
                brdf[lvis] = rows
                out[key + '_render_prior'] = r.render(brdf)
                lit = (r.lcontrib.sum(3) != 0).any(2)
                print(key, 'foreground samples without a lit front-facing light:', int((fg & ~lit).sum()))
    path = os.path.join(HERE, 'reference_sphere.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 1 << 20


if __name__ == '__main__':
    main()
