"""Render and relight a trained NeRFactor straight from camera rays — geometry_from_nerf + test.py without the surface
buffers on disk:

    [torchrun --nproc-per-node N] python -m nerfactor_amd.nerfactor.render_from_nerf \\
        --ckpt=<nerfactor outdir>/checkpoints/ckpt-N --trained_nerf=<nerf outdir> \\
        [--color_correct_albedo] [--tgt_albedo ...] [--tgt_brdf ...] [--sv_axis_i/min/max] \\
        [--scene_bbox x0,x1,y0,y1,z0,z1] [--occu_thres 0] [--mlp_chunk ...] [--split test] [--debug]
        [--occupancy_grid R [--grid_margin 10] [--grid_dilate 2] [--grid_probes 4] [--grid_check K]]

For every shape_mode but 'nerf' NeRFactor's test-mode call reads only alpha, xyz and rayo of the surface buffers; those
are marched per view from the NeRF (nerfactor/surface.py: geometry_from_nerf's march ending in nfx_nerf_surface_fwd) —
no depth gradient, no normals, no shadow rays, no 1.3 GB lvis.npy per 800 x 800 view.  Cameras: <data_root>/<split>_???
/metadata.json of the NeRFactor config, rays at its imh; the NeRF checkpoint is the latest under --trained_nerf.  The
editing / relighting flags mean what they mean in test.py (probes on every view, OLAT on the last); images go to
<outdir>/vis_test/ckpt-N_from_nerf[_<edit>]/batch%09d/.  With N ranks each rank marches and renders only its contiguous
ray range of every view; uint8 rows travel to rank 0 (util/shard.py).  --occupancy_grid R: the march's density passes
evaluate only the samples an R^3 grid baked from the NeRF lists (occupancy.py; geometry_from_nerf's flags)."""
import argparse
import glob
import json
import sys
from os.path import basename, dirname, join

import numpy as np
import torch

from .. import dist as nfx_dist
from . import models, occupancy
from . import test as test_driver
from .datasets.nerf import gen_rays
from .geometry_from_nerf import latest_checkpoint
from .surface import march_surface, nerfactor_test_batch
from .util import config as configutil

REFUSE_NERF_MODE = ("render_from_nerf: shape_mode = nerf renders with the normals and light visibility of the surface "
                    "buffers; write them with geometry_from_nerf, then render with test.py")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', required=True, help="path to the NeRFactor checkpoint")
    ap.add_argument('--trained_nerf', required=True, help="trained NeRF up to (and including) the learning rate folder")
    ap.add_argument('--color_correct_albedo', action='store_true')
    ap.add_argument('--sv_axis_i', type=int, default=0, help="along which axis we do spatially-varying edits")
    ap.add_argument('--sv_axis_min', type=float, default=-1.5)
    ap.add_argument('--sv_axis_max', type=float, default=1.5)
    ap.add_argument('--tgt_albedo', default=None, help="albedo edit name")
    ap.add_argument('--tgt_brdf', default=None, help="BRDF edit name")
    ap.add_argument('--scene_bbox', default=None, help="x_min,x_max,y_min,y_max,z_min,z_max")
    ap.add_argument('--occu_thres', type=float, default=0., help="occupancy threshold surface points have to pass")
    ap.add_argument('--mlp_chunk', type=int, default=1 << 25, help="density samples per kernel launch")
    ap.add_argument('--split', default='test', help="cameras: <data_root>/<split>_???")
    ap.add_argument('--debug', action='store_true')
    occupancy.add_arguments(ap)
    return ap.parse_args(argv)


def parse_bbox(scene_bbox):
    if not scene_bbox:
        return None
    bbox = [float(x) for x in scene_bbox.split(',')]
    if len(bbox) != 6:
        raise ValueError("scene_bbox: x_min,x_max,y_min,y_max,z_min,z_max")
    return bbox


def view_metadata(config, split, debug=False):
    """metadata.json of the views of `split`, in test.py's order (datasets/nerf_shape.py with --debug: view 002 only)."""
    root = config.get('DEFAULT', 'data_root')
    pattern = '%s_002' % split if debug else '%s_???' % split
    return sorted(glob.glob(join(root, pattern, 'metadata.json')))


def view_rays(config, metadata_path):
    """(id, (h, w), rayo[h w, 3], rayd[h w, 3]) float32 of one view at the config's imh (datasets/nerf.py:_read_camera,
    _gen_rays — what datasets/nerf_shape.py and geometry_from_nerf use)."""
    imh = config.getint('DEFAULT', 'imh')
    with open(metadata_path) as h:
        meta = json.load(h)
    imw = int(imh / meta['imh'] * meta['imw'])
    c2w = np.array([float(x) for x in meta['cam_transform_mat'].split(',')]).reshape(4, 4)
    rayo, rayd = gen_rays(c2w, meta['cam_angle_x'], imh, imw)
    return (basename(dirname(metadata_path)), (imh, imw), rayo.astype(np.float32).reshape(-1, 3),
            rayd.astype(np.float32).reshape(-1, 3))


def check_config(config):
    """Refusals that need no GPU: shape_mode = nerf, and scenes without ray cameras."""
    if config.get('DEFAULT', 'shape_mode') == 'nerf':
        raise ValueError(REFUSE_NERF_MODE)
    if config.get('DEFAULT', 'dataset') != 'nerf_shape':
        raise ValueError("render_from_nerf: the cameras of a '%s' scene give no rays (datasets/nerf_shape.py scenes only)"
                         % config.get('DEFAULT', 'dataset'))


def load_nerf(trained_nerf, device):
    """(model, config) of the latest NeRF checkpoint under `trained_nerf`."""
    ckpt = latest_checkpoint(trained_nerf)
    config = configutil.read_config(configutil.get_config_ini(ckpt))
    model = models.get_model_class(config.get('DEFAULT', 'model'))(config).to(device)
    configutil.restore_model(model, ckpt)
    model.to(device)
    return model, config


def main(argv=None):
    args = parse_args(argv)
    config_ini = configutil.get_config_ini(args.ckpt)
    config = configutil.read_config(config_ini)
    check_config(config)
    bbox = parse_bbox(args.scene_bbox)
    occupancy.check_arguments(args)
    if not torch.cuda.is_available():
        raise RuntimeError("render_from_nerf needs an MI355X: libnfx has no CPU path")
    device = nfx_dist.local_device()
    rank, ws = nfx_dist.init_from_env(device=device)
    nerf_model, nerf_config = load_nerf(args.trained_nerf, device)
    grid = occupancy.from_arguments(args, nerf_model, bbox, config.get('DEFAULT', 'data_root'))
    model = models.get_model_class(config.get('DEFAULT', 'model'))(config, debug=args.debug).to(device)
    configutil.restore_model(model, args.ckpt)
    model.to(device)
    outroot = join(config_ini[:-4], 'vis_test', basename(args.ckpt) + '_from_nerf')
    outroot, albedo_scales, brdf_z_override = test_driver.edit_setup(args, model, outroot)
    metas = view_metadata(config, args.split, args.debug)
    with torch.no_grad():
        for batch_i, meta in enumerate(metas):
            id_, hw, rayo, rayd = view_rays(config, meta)
            lo, hi = nfx_dist.shard_range(rayo.shape[0], rank, ws)      # this rank's rays only
            rayo = torch.from_numpy(rayo[lo:hi]).to(device)
            rayd = torch.from_numpy(rayd[lo:hi]).to(device)
            alpha, xyz = march_surface(nerf_model, rayo, rayd, nerf_config, bbox=bbox, occu_thres=args.occu_thres,
                                       mlp_chunk=args.mlp_chunk, grid=grid)
            occupancy.log_view(grid, id_, 'render_from_nerf')
            test_driver.render_test_view(model, nerfactor_test_batch(id_, hw, rayo, rayd, alpha, xyz),
                                         join(outroot, 'batch{i:09d}'.format(i=batch_i)), args,
                                         relight_olat=batch_i == len(metas) - 1, albedo_scales=albedo_scales,
                                         brdf_z_override=brdf_z_override, sharded=True)
            if args.debug:
                break
    nfx_dist.barrier()
    if rank == 0:
        view_at = model.compile_batch_vis(sorted(glob.glob(join(outroot, 'batch?????????'))), outroot, mode='test')
        print("[render_from_nerf] Compilation available for viewing at\n\t%s" % view_at, flush=True)
    return outroot


if __name__ == '__main__':
    main(sys.argv[1:])
