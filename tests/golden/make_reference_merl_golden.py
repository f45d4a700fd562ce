"""Generates tests/golden/reference_merl.npz by running the REAL reference MERL code on synthetic tables.

    python tests/golden/make_reference_merl_golden.py        (build container only: needs the reference checkout and SciPy)

brdf/merl/merl.py:MERL (its SciPy k-d tree included), third_party/nielsen2015on/merlFunctions.py:{readMERLBRDF,
saveMERLBRDF}, brdf/renderer.py:SphereRenderer and data_gen/merl/make_dataset.py:main are imported from the reference
unmodified, the way make_reference_sphere_golden.py does; absl comes from tests/golden/tf_shim.  OpenCV is not installed:
cv2.LUT (xiuminglib's gamma_correct) is a table lookup and is stood in for by `table[im]`; cv2.resize is called by
load_light with the probe's own size (envmap_h = 16 on a 16 x 32 probe), where OpenCV's area interpolation is the identity,
and is stood in for by exactly that (any other size raises).

No MERL file exists here, so the material is tests/merl_cases.synthetic_cube(0), written with the reference's
saveMERLBRDF.  Stored:
  tiny_bytes / tiny_cube          a 5 x 4 x 3 `.binary` with one negative value, and what readMERLBRDF returns for it
  tbl_n, tbl_rows                 MERL(path).tbl: its row count and every 997th row
  ds_*                            make_dataset.main at ims = 16: train / vali row counts, every 997th row of the four arrays,
                                  test.npz's row count and every 997th row
  q_<set>_{idx,dist,gap}          per query set of merl_cases.query_sets: the k-d tree's nearest entry as a flat cube index, its
                                  distance (float64) and the second neighbour's distance minus it (float32); the queries are
                                  the float32 arrays of merl_cases, given to the tree as float64
  <scene>_ref_idx                 the tree's entry for the float64 rows MERL.dir2rusink(ldir, vdir)[lvis] of scenes a and b
  <scene>_<probe>_render[_achromatic]   the reference's float64 render of the material (make_dataset.py:129-138)
and it prints the conditions that the GPU tests rest on (tests/test_cpu_merl.py asserts them from the file alone)."""
import glob
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('NERFACTOR_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(HERE, 'tf_shim'), REF, os.path.join(REF, 'nerfactor'), REPO]


def _same_size_resize(arr, size, interpolation=None):
    if (arr.shape[1], arr.shape[0]) != tuple(size):
        raise NotImplementedError("cv2.resize stand-in: only a resize to the array's own size (the identity)")
    return arr


cv2 = types.ModuleType('cv2')
cv2.LUT = lambda im, table: table[im]
cv2.INTER_LINEAR, cv2.INTER_AREA = 1, 3
cv2.resize = _same_size_resize
sys.modules.setdefault('cv2', cv2)

from absl import flags  # noqa: E402  (the shim)
from third_party.xiuminglib import xiuminglib as xm  # noqa: E402
from third_party.nielsen2015on import merlFunctions  # noqa: E402
from brdf.renderer import SphereRenderer  # noqa: E402
from brdf.merl.merl import MERL  # noqa: E402
from data_gen.merl import make_dataset  # noqa: E402

from tests import merl_cases as mc  # noqa: E402

SCENES = {'a': (16, 1), 'b': (6, 4)}
PROBES = {'point': 40., 'white': 1.}
STRIDE = 997
NAME = 'synth0'


def main():
    out = {}
    sphere = np.load(os.path.join(HERE, 'reference_sphere.npz'))
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the reader on a tiny file
        rng = np.random.RandomState(0)
        vals = rng.uniform(0.5, 300., size=5 * 4 * 3 * 3)
        vals[7] = -0.25
        tiny = os.path.join(tmp, 'tiny.binary')
        with open(tiny, 'wb') as h:
            np.array((5, 4, 3), dtype=np.int32).tofile(h)
            vals.astype(np.float64).tofile(h)
        out['tiny_bytes'] = np.frombuffer(open(tiny, 'rb').read(), dtype=np.uint8)
        out['tiny_cube'] = merlFunctions.readMERLBRDF(tiny)
        assert (out['tiny_cube'] == -1).sum() == 1

        # ---- the synthetic material through the reference's writer, reader and table
        indir = os.path.join(tmp, 'in')
        os.makedirs(indir)
        path = os.path.join(indir, NAME + '.binary')
        merlFunctions.saveMERLBRDF(path, mc.synthetic_cube(0))
        brdf = MERL(path=path)
        tbl = brdf.tbl
        out['tbl_n'] = np.int64(tbl.shape[0])
        out['tbl_rows'] = tbl[::STRIDE]
        valid = (brdf.flat_rgb > 0).all(axis=1)
        flat_of_row = np.nonzero(valid)[0]
        assert flat_of_row.size == tbl.shape[0] and (brdf.flat_rgb[valid] > 0).all()

        # ---- the driver
        outdir = os.path.join(tmp, 'out')
        F = flags.FLAGS
        F.indir, F.outdir, F.ims, F.overwrite = indir, outdir, 16, True
        make_dataset.main(None)
        train = np.load(os.path.join(outdir, 'train_%s.npz' % NAME), allow_pickle=True)
        vali = np.load(os.path.join(outdir, 'vali_%s.npz' % NAME), allow_pickle=True)
        test = np.load(os.path.join(outdir, 'test.npz'), allow_pickle=True)
        out['ds_train_n'], out['ds_vali_n'] = np.int64(train['rusink'].shape[0]), np.int64(vali['rusink'].shape[0])
        for split, data in (('train', train), ('vali', vali)):
            for key in ('rusink', 'refl'):
                out['ds_%s_%s' % (split, key)] = data[key][::STRIDE]
        out['ds_test_n'], out['ds_test_rusink'] = np.int64(test['rusink'].shape[0]), test['rusink'][::STRIDE]
        out['ds_files'] = np.array(sorted(os.path.relpath(p, outdir) for p in glob.glob(os.path.join(outdir, '**', '*'), recursive=True)
                                          if os.path.isfile(p)))
        print('tbl rows', tbl.shape[0], 'train', int(out['ds_train_n']), 'vali', int(out['ds_vali_n']), 'test', int(out['ds_test_n']))
        print('files', list(out['ds_files']))

        # ---- the lookups
        brdf.query(np.zeros((1, 3)))          # builds the tree
        first_cell_invalid = {}
        for name, q in mc.query_sets(sphere['a_rusink']).items():
            q64 = q.astype(np.float64)
            d, ind = brdf.kdtree.query(q64, k=2)
            out['q_%s_idx' % name] = flat_of_row[ind[:, 0]].astype(np.int32)
            out['q_%s_dist' % name] = d[:, 0]
            out['q_%s_gap' % name] = (d[:, 1] - d[:, 0]).astype(np.float32)
            inv = ~valid[mc.nearest_cell(q64)]
            first_cell_invalid[name] = int(inv.sum())
            agree = flat_of_row[ind[:, 0]][~inv] == mc.nearest_cell(q64)[~inv]
            print('query set %-8s rows %6d  invalid first cell %5d  second neighbour within 2e-6: %5d (%.3f %%)  per-axis cell == tree '
                  'where valid: %d of %d' % (name, q.shape[0], inv.sum(), (d[:, 1] - d[:, 0] < 2e-6).sum(),
                                             100. * (d[:, 1] - d[:, 0] < 2e-6).mean(), agree.sum(), agree.size))

        # ---- the renders
        sphere_invalid = 0
        for s, (ims, spp) in SCENES.items():
            rows = None
            for probe, inten in PROBES.items():
                r = SphereRenderer(probe, tmp, envmap_inten=inten, envmap_h=None, ims=ims, spp=spp)
                lvis = r.lvis.astype(bool)
                qrusink = MERL.dir2rusink(r.ldir, r.vdir)[lvis]
                if rows is None:
                    assert np.array_equal(qrusink.astype(np.float32), sphere[s + '_rusink'])
                    _, ind = brdf.kdtree.query(qrusink)
                    rows = brdf.tbl[ind, 3:]
                    out[s + '_ref_idx'] = flat_of_row[ind].astype(np.int32)
                    inv = int((~valid[mc.nearest_cell(qrusink)]).sum())
                    sphere_invalid += inv
                    print('scene', s, 'rows', qrusink.shape[0], 'invalid first cell', inv)
                for achro in (False, True):
                    rgb = np.zeros_like(r.lcontrib)
                    rgb[lvis] = rows
                    if achro:
                        rgb = np.tile(xm.img.rgb2lum(rgb)[:, :, :, None], (1, 1, 1, 3))
                    out['%s_%s_render%s' % (s, probe, '_achromatic' if achro else '')] = r.render(rgb)
        print('sphere rows with an invalid first cell:', sphere_invalid, '(>= 100 wanted)   uniform:', first_cell_invalid['uniform'],
              '(>= 1000 wanted)')
        assert sphere_invalid >= 100 and first_cell_invalid['uniform'] >= 1000
    path = os.path.join(HERE, 'reference_merl.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 1 << 20


if __name__ == '__main__':
    main()
