"""The surface a NeRFactor test view reads, marched straight from camera rays (no surface buffers on disk).

For every shape_mode but 'nerf', NeRFactor's test-mode call reads three things of the buffers geometry_from_nerf writes:
alpha (the mask), xyz and rayo (models/nerfactor.py; reference nerfactor/models/nerfactor.py:186-232) — its normals and
light visibility come from its own networks.  march_surface computes exactly those: geometry_from_nerf's march
(coarse pass, inverse-CDF, fine densities) ending in ONE kernel (nfx_nerf_surface_fwd) that composites, reduces and
applies process_view's epilogue, instead of the [n, S] weights, the torch sums and the blend — and skips the depth
gradient, the normals and the shadow rays (≈ 99 % of the stage).  nerfactor_test_batch wraps the result in the tuple
datasets/nerf_shape.py yields in test mode."""
import numpy as np
import torch

from .. import ops
from .geometry_from_nerf import _sample_counts


def march_surface(nerf_model, rayo, rayd, config, bbox=None, occu_thres=0., mlp_chunk=1 << 25, quantize_alpha=True,
                  full=False, grid=None):
    """(alpha[n], xyz[n, 3]) of the rays rayo + t rayd, as geometry_from_nerf writes them to alpha.png / xyz.npy.

    `config` is the NeRF's own (near, far, sample counts, lin_in_disp); `bbox` (x_min, x_max, ..., z_max) zeroes the
    density outside it, as in geometry_from_nerf.  quantize_alpha: alpha as alpha.png read back gives it
    (floor(255 alpha + 0.5) / 255); xyz always carries the unquantised alpha, as xyz.npy does.
    full = True: (alpha, xyz, occu, depth) with the raw occupancy and expected depth of compute_depth_and_normal.
    grid (occupancy.OccupancyGrid): both density passes evaluate only the samples it lists."""
    n_coarse, n_fine, lin_in_disp = _sample_counts(config)
    near, far = config.getfloat('DEFAULT', 'near'), config.getfloat('DEFAULT', 'far')
    rays_per_call = max(1, mlp_chunk // (n_coarse + n_fine))       # compute_depth_and_normal's chunking
    rayo = rayo.contiguous()
    rayd = torch.nn.functional.normalize(rayd, dim=1, eps=1e-12)    # process_view
    n = rayo.shape[0]
    alpha = torch.empty(n, device=rayo.device)
    xyz = torch.empty((n, 3), device=rayo.device)
    occu = torch.empty(n, device=rayo.device) if full else None
    depth = torch.empty(n, device=rayo.device) if full else None
    for lo in range(0, n, rays_per_call):
        hi = min(n, lo + rays_per_call)
        o, d = rayo[lo:hi].contiguous(), rayd[lo:hi].contiguous()
        # geometry_from_nerf._march: coarse pass, importance samples, fine densities
        z = nerf_model.gen_z(near, far, n_coarse, o.shape[0], lin_in_disp=lin_in_disp, perturb=False, device=o.device)
        w = nerf_model.accumulate_sigma(nerf_model.eval_sigma(o, d, z, use_fine=False, bbox=bbox, grid=grid), z, d)
        z = nerf_model.gen_z_fine(z, w, n_fine, perturb=False)
        sigma = nerf_model.eval_sigma(o, d, z, use_fine=True, bbox=bbox, grid=grid)
        a, x, dep, occ = ops.nerf_surface(sigma, z, o, d, occu_thres=occu_thres, quantize_alpha=quantize_alpha,
                                          want_occu=full)
        alpha[lo:hi] = a
        xyz[lo:hi] = x
        if full:
            occu[lo:hi] = occ
            depth[lo:hi] = dep
    if full:
        return alpha, xyz, occu, depth
    return alpha, xyz


def nerfactor_test_batch(id_, hw, rayo, rayd, alpha, xyz):
    """The batch datasets/nerf_shape.py yields for the rays of a test view — (id_, hw, rayo, rayd, rgb = 0, alpha[n, 1],
    xyz, normal, lvis) — with normal = lvis = None: NeRFactor predicts both itself (shape_mode != 'nerf')."""
    n = rayo.shape[0]
    ids = [id_] * n
    hw = torch.as_tensor(np.tile(np.asarray(hw, np.int32)[None], (n, 1)), device=rayo.device)
    rgb = torch.zeros((n, 3), dtype=torch.float32, device=rayo.device)
    return (ids, hw, rayo, rayd, rgb, alpha.reshape(n, 1), xyz, None, None)
