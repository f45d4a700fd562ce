"""Occupancy grid of the NeRF density marches: an opt-in bit grid, baked once from the trained
NeRF, that lets the density passes of geometry_from_nerf's march, its shadow rays and march_surface evaluate only the
samples whose cell may hold density (ops.occgrid_select, then the density kernel's list form) and write 0 for the rest.

Contract: if no skipped sample has sigma_raw > 0 in the full evaluation, every output of the march is bit-identical to
the march without the grid — relu makes such a sample 0 either way, and the inverse-CDF placement, the compositing and the
fp32-class re-evaluation of every ray's last sample see the same values.  The grid itself is a heuristic (densities probed
on a lattice, a margin, a dilation); check mode (`check_every = k`) proves it on the user's own scene: every k-th density
pass of each network also runs the full pass and raises when an output differs.

Samples outside the grid's box are always evaluated, so the box only decides how much is skipped, never the result."""
import glob
import json
from os.path import join

import numpy as np
import torch

from .. import ops

STAGES = ('coarse_', 'fine_')


class OccupancyMiss(RuntimeError):
    """Check mode found skipped samples with a density: the grid is not sound on this scene."""


def cameras_box(data_root):
    """(x_min, x_max, y_min, y_max, z_min, z_max): the default box of the grid when no --scene_bbox is given, from the
    cameras of every view under `data_root` (<split>_???/metadata.json) — a cube around the point their optical axes pass
    closest to (least squares; the cameras look along -z of cam_transform_mat), reaching the farthest camera.  A captured
    object sits where the cameras look, and cameras on one hemisphere (the usual orbit) still give a box around it."""
    pos, axis = [], []
    for path in sorted(glob.glob(join(data_root, '*_???', 'metadata.json'))):
        with open(path) as h:
            meta = json.load(h)
        c2w = np.array([float(x) for x in meta['cam_transform_mat'].split(',')]).reshape(4, 4)
        pos.append(c2w[:3, 3])
        axis.append(-c2w[:3, 2] / np.linalg.norm(c2w[:3, 2]))
    if len(pos) < 2:
        raise ValueError("occupancy grid: %d camera(s) under %s give no box; pass --scene_bbox" % (len(pos), data_root))
    a, b = np.zeros((3, 3)), np.zeros(3)
    for c, d in zip(pos, axis):
        proj = np.eye(3) - np.outer(d, d)
        a += proj
        b += proj @ c
    centre = np.linalg.lstsq(a, b, rcond=None)[0] if np.linalg.cond(a) < 1e6 else np.mean(pos, 0)
    half = max(float(np.linalg.norm(np.asarray(pos) - centre, axis=1).max()), 1e-3)
    return [float(v) for k in range(3) for v in (centre[k] - half, centre[k] + half)]


def check_bake_arguments(res, probes, dilate):
    """The bake's limits (nfx.h), refused before anything is allocated: 1 <= res <= 1024, 1 <= probes <= 16,
    (res probes)^3 <= 2^30 lattice points (4 GiB of densities per network), 0 <= dilate <= 16."""
    if not 1 <= int(res) <= ops.OCCGRID_MAX_RES:
        raise ValueError("occupancy grid: res = %s (1 .. %d)" % (res, ops.OCCGRID_MAX_RES))
    if not 1 <= int(probes) <= 16:
        raise ValueError("occupancy grid: probes = %s per axis (1 .. 16)" % probes)
    if (int(res) * int(probes)) ** 3 > ops.OCCGRID_MAX_PROBES:
        raise ValueError("occupancy grid: (res probes)^3 = %d probe points (at most 2^30): lower res or probes"
                         % (int(res) * int(probes)) ** 3)
    if not 0 <= int(dilate) <= 16:
        raise ValueError("occupancy grid: dilate = %s (0 .. 16)" % dilate)


def probe_rays(box, res, probes, device):
    """(rayo[M^2, 3], rayd[M^2, 3], z[M]) whose samples are the probe lattice of nfx_occgrid_bake, M = res probes:
    ray (a, b) runs along z through (x_a, y_b), and its sample c, at z[c], is the lattice point (a, b, c)."""
    m = res * probes
    t = (np.arange(m, dtype=np.float64) + 0.5) / m
    axes = [torch.as_tensor((box[2 * k] + t * (box[2 * k + 1] - box[2 * k])).astype(np.float32), device=device)
            for k in range(3)]
    x, y = torch.meshgrid(axes[0], axes[1], indexing='ij')
    rayo = torch.stack((x.reshape(-1), y.reshape(-1), torch.zeros_like(x).reshape(-1)), 1).contiguous()
    rayd = torch.zeros_like(rayo)
    rayd[:, 2] = 1.
    return rayo, rayd, axes[2]


class OccupancyGrid:
    """One bit grid per network (coarse, fine) over one box, and the counters of what the marches evaluated.

    eval_sigma(..., grid=self) calls `sigma_raw`; read `take_counts()` once per view (one host read) for the log."""

    def __init__(self, box, res, bits, check_every=0):
        box = [float(v) for v in box]
        if len(box) != 6 or not all(box[2 * k] < box[2 * k + 1] for k in range(3)):
            raise ValueError("occupancy grid: box = (x_min, x_max, y_min, y_max, z_min, z_max) with min < max")
        if int(res) <= 0:
            raise ValueError("occupancy grid: res = %s (> 0)" % res)
        if int(check_every) < 0:
            raise ValueError("occupancy grid: check_every = %s (0 = off, k = every k-th density pass)" % check_every)
        self.box, self.res, self.bits, self.check_every = box, int(res), dict(bits), int(check_every)
        device = next(iter(self.bits.values())).device
        self._evaluated = torch.zeros(1, dtype=torch.int64, device=device)
        self._seen = 0
        self._passes = {pref: 0 for pref in STAGES}      # density passes per network (check mode counts each on its own)

    @classmethod
    def bake(cls, nerf_model, box, res, probes=4, margin=10., dilate=2, check_every=0):
        """The grids of both networks of a tuned NeRF: each network's raw density on the probe lattice (probes^3 points per
        cell, nfx_nerf_sigma_fwd in the model's precision), a cell set when a probe has sigma_raw > -margin, dilated by
        `dilate` cells.  Deterministic: every rank bakes the same grid."""
        check_bake_arguments(res, probes, dilate)
        require_tuned(nerf_model)
        device = next(nerf_model.parameters()).device
        rayo, rayd, zrow = probe_rays(box, int(res), int(probes), device)
        m = zrow.shape[0]
        rays = max(1, (1 << 24) // m)
        bits = {}
        with torch.no_grad():
            for pref in STAGES:
                blob = nerf_model._nerf_geom_blob(pref)
                sigma = torch.empty((m * m, m), dtype=torch.float32, device=device)
                for lo in range(0, m * m, rays):
                    o, d = rayo[lo:lo + rays], rayd[lo:lo + rays]
                    z = zrow[None].expand(o.shape[0], m).contiguous()
                    sigma[lo:lo + rays] = ops.nerf_sigma_fwd(o, d, z, blob, nerf_model.precision)
                bits[pref] = ops.occgrid_bake(sigma, int(res), int(probes), float(margin), int(dilate))
        return cls(box, res, bits, check_every)

    def occupied_fraction(self, pref='fine_'):
        """The fraction of the cells whose bit is set (one host read)."""
        b = self.bits[pref]
        n = int(torch.bitwise_and(b[:, None] >> torch.arange(32, device=b.device), 1).sum())
        return n / self.res ** 3

    def sigma_raw(self, rayo, rayd, z, pref, blob, precision, bbox=None):
        """sigma_raw[N, S] of the network `pref` at the listed samples, 0.0 elsewhere."""
        out, count = ops.nerf_sigma_fwd_grid(rayo, rayd, z, blob, self.bits[pref], self.res, self.box, bbox, precision)
        self._seen += out.numel()
        self._evaluated += count
        return out

    def check_due(self, pref):
        """True on every check_every-th density pass of the network `pref` (its first one included) when check mode is on.
        Each network keeps its own count: a march alternates coarse and fine passes, and one shared count would check only
        one of them for an even check_every."""
        due = self.check_every > 0 and self._passes[pref] % self.check_every == 0
        self._passes[pref] += 1
        return due

    @staticmethod
    def verify(sigma_grid, sigma_full, pref):
        """Raises OccupancyMiss when the march's densities with the grid differ from the full pass's (a skipped sample
        with sigma_raw > 0: the listed ones are bit-identical)."""
        differ = sigma_grid != sigma_full
        n = int(differ.sum())
        if n:
            worst = float(sigma_full[differ].max())
            raise OccupancyMiss("occupancy grid check (%s network): %d skipped samples have a density, the largest "
                                "relu(sigma) = %.6g; bake with a larger --grid_margin / --grid_dilate / --grid_probes "
                                "or a finer grid" % (pref.rstrip('_'), n, worst))

    def take_counts(self):
        """(samples seen, samples evaluated) since the last call (one host read), and resets both."""
        seen, evaluated = self._seen, int(self._evaluated.item())
        self._seen = 0
        self._evaluated.zero_()
        return seen, evaluated


def require_tuned(nerf_model):
    if not getattr(nerf_model, 'tuned', False):
        raise NotImplementedError(
            "occupancy grid: the grid's list form exists for the tuned density kernels (mlp_width = 256, enc_depth = 8, "
            "relu, use_views, n_freqs 10 / 4); this network runs on the runtime-shaped kernels")


def add_arguments(ap):
    """The grid's flags of geometry_from_nerf and render_from_nerf."""
    ap.add_argument('--occupancy_grid', type=int, default=0,
                    help="occupancy grid resolution R (R^3 cells; 0 = off: every density sample is evaluated)")
    ap.add_argument('--grid_margin', type=float, default=10.,
                    help="a cell is occupied when a probe has sigma_raw > -margin (sigma_raw units of the NeRF)")
    ap.add_argument('--grid_dilate', type=int, default=2, help="cells the occupied set is grown by on every axis")
    ap.add_argument('--grid_probes', type=int, default=4, help="density probes per cell and axis (probes^3 per cell)")
    ap.add_argument('--grid_check', type=int, default=0,
                    help="check mode: every K-th density pass of each network also runs the full pass and raises on a "
                         "difference (0 = off)")


def check_arguments(args):
    """Refusals that need no GPU."""
    if args.occupancy_grid < 0:
        raise ValueError("--occupancy_grid %d: the resolution R must be > 0 (0 = off)" % args.occupancy_grid)
    if args.occupancy_grid == 0:
        return
    if args.grid_dilate < 0:
        raise ValueError("--grid_dilate %d: must be >= 0" % args.grid_dilate)
    if args.grid_probes <= 0:
        raise ValueError("--grid_probes %d: must be > 0" % args.grid_probes)
    try:
        check_bake_arguments(args.occupancy_grid, args.grid_probes, args.grid_dilate)
    except ValueError as e:
        raise ValueError("--occupancy_grid %d --grid_probes %d --grid_dilate %d: %s" % (
            args.occupancy_grid, args.grid_probes, args.grid_dilate, e)) from None
    if args.grid_check < 0:
        raise ValueError("--grid_check %d: must be >= 0 (0 = off)" % args.grid_check)
    if not np.isfinite(args.grid_margin):
        raise ValueError("--grid_margin must be finite")


def from_arguments(args, nerf_model, bbox, data_root):
    """The grid the flags ask for, or None (--occupancy_grid 0: today's path).  Box: --scene_bbox if given, else the
    cameras' box (cameras_box)."""
    check_arguments(args)
    if args.occupancy_grid == 0:
        return None
    require_tuned(nerf_model)
    box = list(bbox) if bbox is not None else cameras_box(data_root)
    return OccupancyGrid.bake(nerf_model, box, args.occupancy_grid, probes=args.grid_probes, margin=args.grid_margin,
                              dilate=args.grid_dilate, check_every=args.grid_check)


def log_view(grid, view_id, tag):
    """One log line per view: the fraction of density samples evaluated."""
    if grid is None:
        return None
    seen, evaluated = grid.take_counts()
    frac = evaluated / seen if seen else 0.
    print("[%s] %s: occupancy grid evaluated %d of %d density samples (%.4f)" % (tag, view_id, evaluated, seen, frac),
          flush=True)
    return frac
