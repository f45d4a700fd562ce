"""From MERL `.binary` files to the data directory that `trainvali --config brdf.ini` reads, with the reference's flags and
output layout (data_gen/merl/make_dataset.py):

    python -m nerfactor_amd.data_gen.merl.make_dataset --indir '<dir>/*.binary' --outdir <data_root> \\
        [--vali_frac 0.01] [--envmap_path point] [--envmap_h 16] [--envmap_inten 40] [--slice_percentile 80] \\
        [--ims 128] [--spp 1] [--overwrite]

    <outdir>/test.npz                       envmap_h, ims, spp, rusink: the 90 x 90 coordinates of the characteristic slice, then
                                            dir2rusink(ldir, vdir)[lvis] of the sphere render
    <outdir>/{train,vali}_<name>.npz        i, name, envmap_h, ims, spp, rusink [M, 3], refl [M, 1] (the luminance); every
                                            int(1 / vali_frac)-th valid entry is a validation row
    <outdir>/vis/{cslice,cslice_achromatic,render,render_achromatic}/<name>.png

`--indir` is a glob, or a directory whose files are taken (what the reference's flag means); files that do not end in
`.binary` are skipped.  The tables and the split are host-side NumPy; the renders are one fused launch each
(MERL.render_sphere), where the reference builds a k-d tree per material and queries it per (sample, light) pair."""
import argparse
import glob
import os
import shutil
import sys
from os.path import isdir, join

import numpy as np

from ...brdf.merl import MERL, rgb2lum
from ...brdf.renderer import SphereRenderer


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--indir', required=True, help="glob of (or directory with) the downloaded MERL binary files")
    ap.add_argument('--vali_frac', type=float, default=0.01, help="fraction of data used for validation")
    ap.add_argument('--envmap_path', default='point', help="light probe path or a special string like 'point'")
    ap.add_argument('--envmap_h', type=int, default=16, help="light probe height")
    ap.add_argument('--envmap_inten', type=float, default=40., help="light probe intensity")
    ap.add_argument('--slice_percentile', type=float, default=80, help="clip percentile for visualizing characteristic slice")
    ap.add_argument('--ims', type=int, default=128, help="render size during visualization")
    ap.add_argument('--spp', type=int, default=1, help="samples per pixel for BRDF rendering")
    ap.add_argument('--outdir', required=True, help="output directory")
    ap.add_argument('--overwrite', action='store_true', help="whether to remove output folder if it already exists")
    return ap.parse_args(argv)


def save_npz(data, path):
    with open(path, 'wb') as h:
        np.savez(h, **data)


def test_coordinates(renderer):
    """float32 [8100 + rows, 3]: the characteristic slice's coordinates, then the front-lit rows of the render (make_dataset.py:54-66)."""
    cslice_rusink = np.reshape(MERL().get_characterstic_slice_rusink(), (-1, 3))
    render_rusink = MERL.dir2rusink(renderer.ldir, renderer.vdir)[renderer.lvis.astype(bool)]
    return np.vstack((cslice_rusink, render_rusink)).astype(np.float32)


def split_material(brdf, vali_frac):
    """(train_rusink, train_refl, vali_rusink, vali_refl) float32 of a material's valid entries (make_dataset.py:80-94); the
    split is a mask, not the reference's quadratic `x not in vali_ind`."""
    tbl = brdf.tbl
    rusink, refl = tbl[:, :3], rgb2lum(tbl[:, 3:])[:, None]
    is_vali = np.zeros(tbl.shape[0], dtype=bool)
    is_vali[::int(1 / vali_frac)] = True
    f32 = lambda a: a.astype(np.float32)
    return f32(rusink[~is_vali]), f32(refl[~is_vali]), f32(rusink[is_vali]), f32(refl[is_vali])


def _write_png(arr_uint8, path):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr_uint8).save(path)


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("make_dataset renders every material on the GPU and needs an MI355X: libnfx has no CPU path")
    if args.overwrite and isdir(args.outdir):
        shutil.rmtree(args.outdir)
    os.makedirs(args.outdir, exist_ok=True)

    renderer = SphereRenderer(args.envmap_path, envmap_inten=args.envmap_inten, envmap_h=args.envmap_h, ims=args.ims, spp=args.spp)
    common = {'envmap_h': args.envmap_h, 'ims': args.ims, 'spp': args.spp}
    save_npz(dict(common, rusink=test_coordinates(renderer)), join(args.outdir, 'test.npz'))

    # `i` is the material's row in the prior's latent table (models/brdf.py), so only the tables are counted: the reference
    # counts every globbed path, which is the same number when the directory holds nothing but tables
    paths = [p for p in sorted(glob.glob(join(args.indir, '*') if isdir(args.indir) else args.indir)) if p.endswith('.binary')]
    vis_dir = join(args.outdir, 'vis')
    for i, path in enumerate(paths):
        brdf = MERL(path=path)
        train_rusink, train_refl, vali_rusink, vali_refl = split_material(brdf, args.vali_frac)
        save_npz(dict(common, i=i, name=brdf.name, rusink=train_rusink, refl=train_refl), join(args.outdir, 'train_%s.npz' % brdf.name))
        save_npz(dict(common, i=i, name=brdf.name, rusink=vali_rusink, refl=vali_refl), join(args.outdir, 'vali_%s.npz' % brdf.name))
        for achro in (False, True):
            suffix = '_achromatic' if achro else ''
            cslice = brdf.get_characterstic_slice()
            if achro:
                cslice = np.tile(rgb2lum(cslice)[:, :, None], (1, 1, 3))
            _write_png(brdf.characteristic_slice_as_img(cslice, clip_percentile=args.slice_percentile),
                       join(vis_dir, 'cslice' + suffix, brdf.name + '.png'))
            render = brdf.render_sphere(renderer, achromatic=achro).cpu().numpy()
            _write_png((np.clip(render, 0, 1) * 255).astype(np.uint8), join(vis_dir, 'render' + suffix, brdf.name + '.png'))
    print("[make_dataset] %d material(s) written to\n\t%s" % (len(paths), args.outdir), flush=True)
    return args.outdir


if __name__ == '__main__':
    main(sys.argv[1:])
