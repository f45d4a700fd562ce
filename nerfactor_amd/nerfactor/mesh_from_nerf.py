"""A triangle mesh from a trained NeRF: the iso-surface of its raw density.

    python -m nerfactor_amd.nerfactor.mesh_from_nerf --trained_nerf=<outroot>/<xname>
        [--scene_bbox x0,x1,y0,y1,z0,z1] [--res 256] [--iso 10] [--network coarse|fine] [--nonormals] [--out mesh.ply]
        [--keep_largest K] [--min_faces M]

Three steps, all on libnfx: the network's raw density (before the relu) on a lattice of res^3 points over the box — the
probe lattice of the occupancy grid, evaluated in chunks with nfx_nerf_sigma_fwd in the model's precision, as
occupancy.OccupancyGrid.bake does; its iso-surface by marching tetrahedra (ops.isosurface: closed wherever the surface
stays inside the box, inside = density above iso, faces wound so that their normals leave the object); per-vertex normals
-normalize(grad sigma) from nfx_nerf_sigma_grad (the face normals' sum where that gradient is zero).  The PLY
(mesh.write_ply, float x y z nx ny nz) loads back through mesh.TriMesh.load, whose ray casts (mesh.RayMeshIntersector)
then run against the NeRF's geometry.
--keep_largest K / --min_faces M (opt-in): the mesh's connected components are labelled on the GPU
(ops.mesh_components) and only the K with the most triangles / those with at least M triangles are written — a fitted
density has floaters, and every one of them casts shadows; the normals are then evaluated at the surviving vertices only.
With several ranks rank 0 alone extracts; the others wait."""
import argparse
import sys
import time
from os.path import join

import numpy as np
import torch

from .. import dist as nfx_dist
from .. import mesh as nfx_mesh
from .. import ops
from . import occupancy

NETWORKS = {'coarse': 'coarse_', 'fine': 'fine_'}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--trained_nerf', required=True, help="trained NeRF up to (and including) the learning rate folder")
    ap.add_argument('--data_root', default='', help="input data root (defaults to the one NeRF was trained on)")
    ap.add_argument('--scene_bbox', default=None,
                    help="x_min,x_max,y_min,y_max,z_min,z_max of the lattice (default: the cameras' box, occupancy.cameras_box)")
    ap.add_argument('--res', type=int, default=256, help="lattice points per axis")
    ap.add_argument('--iso', type=float, default=10.,
                    help="raw-density level of the surface; 10 is common NeRF practice and has not been measured on a real "
                         "scene here: a network whose density peaks lower needs a lower level")
    ap.add_argument('--network', choices=sorted(NETWORKS), default='fine')
    ap.add_argument('--nonormals', action='store_true', help="write no per-vertex normals")
    ap.add_argument('--keep_largest', type=int, default=0, help="keep only the K connected components with the most triangles (0: all)")
    ap.add_argument('--min_faces', type=int, default=0, help="keep only the connected components with at least M triangles (0: all)")
    ap.add_argument('--out', default=None, help="output PLY (default: <trained_nerf>/mesh_<network>_res<R>_iso<iso>.ply, with "
                                                "_largest<K> and _min<M> before .ply when the components are filtered)")
    return ap.parse_args(argv)


def check_lattice(box, res, iso, keep_largest=0, min_faces=0):
    """Refusals that need no GPU; returns the box as six floats."""
    if int(keep_largest) < 0 or int(min_faces) < 0:
        raise ValueError("mesh_from_nerf: keep_largest = %s and min_faces = %s must not be negative" % (keep_largest, min_faces))
    box = [float(v) for v in box]
    if len(box) != 6:
        raise ValueError("mesh_from_nerf: box = x_min,x_max,y_min,y_max,z_min,z_max, got %d numbers" % len(box))
    if not all(np.isfinite(box)) or not all(box[2 * k] < box[2 * k + 1] for k in range(3)):
        raise ValueError("mesh_from_nerf: box = %s must be finite with min < max on every axis" % (box,))
    if int(res) < 2:
        raise ValueError("mesh_from_nerf: res = %s (at least 2 lattice points per axis)" % res)
    if int(res) ** 3 >= ops.ISOSURFACE_MAX_POINTS:
        raise ValueError("mesh_from_nerf: res^3 = %d lattice points (fewer than 2^31: res <= 1290)" % int(res) ** 3)
    if not np.isfinite(float(iso)):
        raise ValueError("mesh_from_nerf: iso = %r must be finite" % (iso,))
    return box


def lattice_frame(box, res):
    """(origin, spacing) of the res^3 lattice over `box`: point i of an axis at lo + (i + 0.5) / res (hi - lo)."""
    spacing = [(box[2 * k + 1] - box[2 * k]) / res for k in range(3)]
    return [box[2 * k] + 0.5 * spacing[k] for k in range(3)], spacing


def eval_lattice(nerf_model, box, res, network='fine'):
    """float32 [res, res, res] on the device: the network's raw density on the lattice of occupancy.probe_rays(box, res, 1)."""
    device = next(nerf_model.parameters()).device
    rayo, rayd, zrow = occupancy.probe_rays(box, res, 1, device)
    blob = nerf_model._nerf_geom_blob(NETWORKS[network])
    field = torch.empty((res * res, res), dtype=torch.float32, device=device)
    rays = max(1, (1 << 24) // res)
    with torch.no_grad():
        for lo in range(0, res * res, rays):
            o, d = rayo[lo:lo + rays], rayd[lo:lo + rays]
            z = zrow[None].expand(o.shape[0], res).contiguous()
            field[lo:lo + rays] = ops.nerf_sigma_fwd(o, d, z, blob, nerf_model.precision)
    return field.view(res, res, res)


def face_normal_sums(vertices, faces):
    """float32 [nv, 3] (NumPy, summed in float64 in face order): per vertex the normalised sum of the unit normals of its
    faces; zeros where it has none or they cancel."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, length, out=np.zeros_like(n), where=length > 0)
    total = np.zeros((np.asarray(vertices).shape[0], 3))
    np.add.at(total, np.asarray(faces, dtype=np.int64).reshape(-1), np.repeat(n, 3, axis=0))
    length = np.linalg.norm(total, axis=1, keepdims=True)
    return np.divide(total, length, out=np.zeros_like(total), where=length > 0).astype(np.float32)


def gradient_normals(nerf_model, vertices, network='fine', chunk=1 << 22):
    """float32 [nv, 3] on the device: -normalize(grad sigma) of the network at the vertices (nfx_nerf_sigma_grad: the
    gradient of relu(sigma), so zero where the density at the vertex is not positive)."""
    blob = nerf_model._nerf_geom_blob(NETWORKS[network])
    normals = torch.empty_like(vertices)
    with torch.no_grad():
        for lo in range(0, vertices.shape[0], chunk):
            p = vertices[lo:lo + chunk].contiguous()
            z = torch.zeros((p.shape[0], 1), dtype=torch.float32, device=p.device)
            normals[lo:lo + chunk] = ops.nerf_sigma_grad(p, torch.zeros_like(p), z, blob, nerf_model.precision)[0][:, 0]
    return normals


def extract(nerf_model, box, res, iso=10., network='fine', normals=True, times=None, keep_largest=0, min_faces=0, info=None):
    """(vertices float32 [nv, 3], faces int32 [nf, 3], normals float32 [nv, 3] or None) as NumPy arrays: the surface
    sigma_raw = iso of the `network` of a tuned NeRF over `box`, sampled at res points per axis.  With keep_largest or
    min_faces only the components that pass (mesh.filter_by_labels), filtered on the device before the normals; the dict
    `info` then receives the filter's counts."""
    if network not in NETWORKS:
        raise ValueError("mesh_from_nerf: network = %r (coarse, fine)" % (network,))
    box, res = check_lattice(box, res, iso, keep_largest, min_faces), int(res)
    occupancy.require_tuned(nerf_model)
    device = next(nerf_model.parameters()).device
    clock = _Clock(device, times)
    field = eval_lattice(nerf_model, box, res, network)
    clock.lap('lattice')
    origin, spacing = lattice_frame(box, res)
    vertices, faces = ops.isosurface(field, float(iso), origin, spacing)
    clock.lap('isosurface')
    if keep_largest or min_faces:
        vertices, faces, _, found = ops.mesh_filter_components(vertices, faces, keep_largest, min_faces)
        if info is not None:
            info.update(found)
        clock.lap('components')
    nrm = gradient_normals(nerf_model, vertices, network).cpu().numpy() if normals else None
    vertices, faces = vertices.cpu().numpy(), faces.cpu().numpy()
    if normals:      # where the gradient is zero: the normalised sum of the adjacent face normals
        missing = (nrm == 0).all(1)
        if missing.any():
            nrm[missing] = face_normal_sums(vertices, faces)[missing]
    clock.lap('normals')
    return vertices, faces, nrm


class _Clock:
    def __init__(self, device, times):
        self.device, self.times = device, times
        self.t0 = self._now()

    def _now(self):
        torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def lap(self, name):
        t = self._now()
        if self.times is not None:
            self.times[name] = t - self.t0
        self.t0 = t


def default_out(trained_nerf, network, res, iso, keep_largest=0, min_faces=0):
    suffix = ('_largest%d' % keep_largest if keep_largest else '') + ('_min%d' % min_faces if min_faces else '')
    return join(trained_nerf, 'mesh_%s_res%d_iso%g%s.ply' % (network, res, iso, suffix))


def main(argv=None):
    from . import models
    from .geometry_from_nerf import latest_checkpoint
    from .util import config as configutil
    args = parse_args(argv)
    bbox = None
    if args.scene_bbox:
        try:
            bbox = [float(x) for x in args.scene_bbox.split(',')]
        except ValueError:
            raise ValueError("--scene_bbox %s: x_min,x_max,y_min,y_max,z_min,z_max" % args.scene_bbox) from None
    check_lattice(bbox if bbox is not None else [0., 1.] * 3, args.res, args.iso, args.keep_largest, args.min_faces)
    if not torch.cuda.is_available():
        raise RuntimeError("mesh_from_nerf needs an MI355X: libnfx has no CPU path")
    device = nfx_dist.local_device()
    rank, _ = nfx_dist.init_from_env(device=device)
    out = args.out or default_out(args.trained_nerf, args.network, args.res, args.iso, args.keep_largest, args.min_faces)
    if rank == 0:
        ckpt = latest_checkpoint(args.trained_nerf)
        config = configutil.read_config(configutil.get_config_ini(ckpt))
        if args.data_root:
            config.set('DEFAULT', 'data_root', args.data_root)
        model = models.get_model_class(config.get('DEFAULT', 'model'))(config).to(device)
        configutil.restore_model(model, ckpt)
        model.to(device)
        box = bbox if bbox is not None else occupancy.cameras_box(config.get('DEFAULT', 'data_root'))
        times, found = {}, {}
        vertices, faces, normals = extract(model, box, args.res, args.iso, args.network, not args.nonormals, times,
                                           args.keep_largest, args.min_faces, found)
        nfx_mesh.write_ply(out, vertices, faces, normals=normals)
        filtered = "; " + nfx_mesh.filter_clause(found, times['components']) if found else ""
        print("[mesh_from_nerf] %d^3 lattice over %s, iso %g (%s network): %d vertices, %d triangles%s; lattice %.3f s, "
              "iso-surface %.3f s, normals %.3f s -> %s" % (args.res, [round(v, 6) for v in box], args.iso, args.network,
                                                           vertices.shape[0], faces.shape[0], filtered, times['lattice'],
                                                           times['isosurface'], times['normals'], out), flush=True)
    nfx_dist.barrier()
    return out


if __name__ == '__main__':
    main(sys.argv[1:])
