"""Looks at what the BRDF prior learned: every seen material and the seeded walk between materials as a sphere under a
light probe (render.png), the characteristic slice (cslice.png) and the latent code (metadata.json), in the reference's
output layout (nerfactor/explore_brdf_space.py:34-86):

    python -m nerfactor_amd.nerfactor.explore_brdf_space --ckpt=<outdir>/checkpoints/ckpt-N \\
        [--envmap point] [--envmap_inten 40] [--envmap_h 16] [--ims 128] [--spp 1] [--batch 32] [--merl_dir DIR]

    <config>/vis_test/<ckpt>/batch?????????/{metadata.json,cslice.png,render.png[,render_measured.png]}

The ids are the ones the brdf_merl test split builds (datasets/brdf_merl.py:split_test_identities).  Unlike the reference, which
evaluates one Rusinkiewicz row per front-lit (sample, light) pair of a `test*.npz` rendered in advance, nothing is read
from disk: light, image size and samples per pixel are flags, and `--batch` identities are rendered per launch
(Model.render_spheres).  A batch directory that already holds its three files is skipped.  The bar plots, the HTML and the
video of the reference are not produced.

With `--merl_dir DIR`, every seen material whose DIR/<name>.binary exists also gets render_measured.png — the measured
table itself under the same light (brdf.merl.MERL.render_sphere, achromatic like the prior, which is trained on the
luminance) — and metadata.json gains 'psnr_measured', the PSNR between the two renders clipped to [0, 1]."""
import argparse
import sys
from os.path import basename, exists, join

import torch

from .. import dist as nfx_dist
from . import models
from .datasets.brdf_merl import split_test_identities
from .util import config as configutil

EXPECTS = ('metadata.json', 'cslice.png', 'render.png')


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', required=True, help="path to checkpoint")
    ap.add_argument('--debug', action='store_true')
    ap.add_argument('--envmap', default='point', help="'point', 'white' or the path of a light probe")
    ap.add_argument('--envmap_inten', type=float, default=40.)
    ap.add_argument('--envmap_h', type=int, default=16)
    ap.add_argument('--ims', type=int, default=128)
    ap.add_argument('--spp', type=int, default=1)
    ap.add_argument('--batch', type=int, default=32, help="identities per launch")
    ap.add_argument('--merl_dir', default=None, help="directory with <material>.binary files to render next to the learned spheres")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("explore_brdf_space needs an MI355X: libnfx has no CPU path")
    device = nfx_dist.local_device()
    config_ini = configutil.get_config_ini(args.ckpt)
    config = configutil.read_config(config_ini)
    outroot = join(config_ini[:-4], 'vis_test', basename(args.ckpt))
    Model = models.get_model_class(config.get('DEFAULT', 'model'))
    model = Model(config, debug=args.debug).to(device)
    configutil.restore_model(model, args.ckpt)
    model.to(device)

    ids = split_test_identities(model.brdf_names)
    measured_path = lambda id_: (join(args.merl_dir, id_ + '.binary') if args.merl_dir is not None and id_ in model.brdf_names
                                 and exists(join(args.merl_dir, id_ + '.binary')) else None)
    expects = lambda id_: EXPECTS + (('render_measured.png',) if measured_path(id_) else ())
    todo = [(i, id_) for i, id_ in enumerate(ids)
            if not all(exists(join(outroot, 'batch{i:09d}'.format(i=i), x)) for x in expects(id_))]
    if args.debug:
        todo = todo[:1]
    for k in range(0, len(todo), max(1, args.batch)):
        chunk = todo[k:k + max(1, args.batch)]
        with torch.no_grad():
            z = torch.cat([model.z_of_id(id_) for _, id_ in chunk], 0)
            renders = model.render_spheres(z, args.envmap, args.envmap_inten, args.envmap_h, args.ims, args.spp)
            cslices = model.characteristic_slices(z)
        for j, (i, id_) in enumerate(chunk):
            measured = None
            if measured_path(id_):
                from ..brdf.merl import MERL
                scene = model._sphere_scene(args.envmap, args.envmap_inten, args.envmap_h, args.ims, args.spp, device)
                measured = MERL(measured_path(id_)).render_sphere(scene['renderer'], achromatic=True, device=device)
            model.write_sphere_vis(join(outroot, 'batch{i:09d}'.format(i=i)), id_, z[j], cslices[j], renders[j], measured=measured)
    print("[explore_brdf_space] %d of %d identities rendered into\n\t%s" % (len(todo), len(ids), outroot), flush=True)
    return outroot


if __name__ == '__main__':
    main(sys.argv[1:])
