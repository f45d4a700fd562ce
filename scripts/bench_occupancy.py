#!/usr/bin/env python
"""Per-view cost of the density marches with and without the occupancy grid: the shadow rays of
geometry_from_nerf (compute_light_visibility over the view's surface points x 512 lights) and march_surface, for one
800 x 800 view of the NeRF fitted to a scene (tests/golden/nerf_trained_fp16.npz: a unit sphere — a best case, no
self-occlusion).  Reports pairs/s and seconds per view, the march's ms, the fraction of density samples evaluated, the bake
time and how many output elements differ (0 when the grid is sound).  One JSON line.

    python scripts/bench_occupancy.py [--imh 800] [--reps 3] [--lvis-points 0] [--res 128] [--probes 4] [--margin 10]
                                      [--dilate 2] [--grid-only]

--grid-only: the grid route alone, one pass of each march (e.g. under a profiler)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--imh', type=int, default=800)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--lvis-points', type=int, default=0, help="surface points of the shadow-ray march (0: all of the view's)")
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--probes', type=int, default=4)
    ap.add_argument('--margin', type=float, default=10.)
    ap.add_argument('--dilate', type=int, default=2)
    ap.add_argument('--box', default='-2.5,2.5,-2.5,2.5,-2.5,2.5',
                    help="grid box (no scene bbox: every shadow-ray sample, up to lvis_far = 1 off the sphere, lies inside)")
    ap.add_argument('--grid-only', action='store_true', help="the grid route only, once (e.g. under a profiler)")
    args = ap.parse_args()
    from nerfactor_amd import build, synth
    build.build()
    from bench_render_from_nerf import timed_ms
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid
    from nerfactor_amd.nerfactor.surface import march_surface
    from tests.golden import golden_inputs as gi
    dev = torch.device('cuda', 0)
    h = w = args.imh
    cfg = make_config('nerf')
    nerf = get_model_class('nerf')(cfg)
    with torch.no_grad():
        for pref, net in zip(('coarse_', 'fine_'), gi.trained_nerf_nets()):
            for part in ('enc', 'sigma_out', 'bottleneck', 'rgb_out'):
                for layer, (k, b) in zip(nerf.net[pref + part].layers, net[part]):
                    layer.kernel.copy_(torch.from_numpy(np.asarray(k, np.float32)))
                    layer.bias.copy_(torch.from_numpy(np.asarray(b, np.float32)))
    nerf = nerf.to(dev)
    box = [float(x) for x in args.box.split(',')]
    rayo_h, rayd_h = synth.camera_rays(h, w)
    rayo, rayd = torch.from_numpy(rayo_h).to(dev), torch.from_numpy(rayd_h).to(dev)
    out = {"workload": "one %d x %d view: NeRF fitted to a unit sphere (tests/golden/nerf_trained_fp16.npz; 128 coarse + 320 "
                       "fine-network density samples per ray), occupancy grid %d^3 over %s, %d^3 probes per cell, margin %g, "
                       "dilate %d" % (h, w, args.res, args.box, args.probes, args.margin, args.dilate),
           "reps": args.reps}
    with torch.no_grad():
        OccupancyGrid.bake(nerf, box, args.res, args.probes, args.margin, args.dilate)          # warm-up (packing)
        bake_ms, grid = once_ms(lambda: OccupancyGrid.bake(nerf, box, args.res, args.probes, args.margin, args.dilate))
        out["grid"] = {"bake_ms": bake_ms, "occupied_cells_coarse": grid.occupied_fraction('coarse_'),
                       "occupied_cells_fine": grid.occupied_fraction('fine_')}
        if args.grid_only:
            march_surface(nerf, rayo, rayd, cfg, grid=grid)
            d = torch.nn.functional.normalize(rayd, dim=1, eps=1e-12)
            occu, depth, normal = G.compute_depth_and_normal(nerf, rayo, d, cfg, grid=grid)
            hit = torch.nonzero(occu.clamp(0., 1.) > 0)[:, 0]
            hit = hit[torch.linspace(0, hit.numel() - 1, args.lvis_points or 4096, device=dev).long()]
            G.compute_light_visibility(nerf, (rayo[hit] + d[hit] * depth[hit, None]).contiguous(), normal[hit].contiguous(),
                                       cfg, grid=grid)
            torch.cuda.synchronize()
            seen, evaluated = grid.take_counts()
            out["grid_only"] = {"evaluated_fraction": evaluated / seen}
            print(json.dumps(out))
            return
        # ---- march_surface
        plain_ms, (a0, x0) = timed_ms(lambda: march_surface(nerf, rayo, rayd, cfg), args.reps)
        grid.take_counts()
        grid_ms, (a1, x1) = timed_ms(lambda: march_surface(nerf, rayo, rayd, cfg, grid=grid), args.reps)
        seen, evaluated = grid.take_counts()
        out["march_surface"] = {"plain_ms": plain_ms, "grid_ms": grid_ms, "speedup": plain_ms / grid_ms,
                                "evaluated_fraction": evaluated / seen,
                                "differing_elements": int((a0 != a1).sum()) + int((x0 != x1).sum())}
        # ---- shadow rays of the view's surface points
        d = torch.nn.functional.normalize(rayd, dim=1, eps=1e-12)
        occu, depth, normal = G.compute_depth_and_normal(nerf, rayo, d, cfg)
        hit = torch.nonzero(occu.clamp(0., 1.) > 0)[:, 0]
        n_hit = hit.numel()
        if args.lvis_points:
            hit = hit[torch.linspace(0, hit.numel() - 1, args.lvis_points, device=dev).long()]
        surf = (rayo[hit] + d[hit] * depth[hit, None]).contiguous()
        nrm = normal[hit].contiguous()
        G.compute_light_visibility(nerf, surf[:256], nrm[:256], cfg)
        G.compute_light_visibility(nerf, surf[:256], nrm[:256], cfg, grid=grid)
        grid.take_counts()
        lvis_grid_ms, lvis1 = once_ms(lambda: G.compute_light_visibility(nerf, surf, nrm, cfg, grid=grid))
        seen, evaluated = grid.take_counts()
        lvis_plain_ms, lvis0 = once_ms(lambda: G.compute_light_visibility(nerf, surf, nrm, cfg))
        pairs = int(((torch.nn.functional.normalize(
            torch.as_tensor(G.gen_light_xyz(16, 32)[0].reshape(-1, 3), dtype=torch.float32, device=dev)[None] - surf[:, None],
            dim=2) * nrm[:, None]).sum(-1) > 0).sum())
        scale = n_hit / max(1, hit.numel())
        out["shadow_rays"] = {
            "surface_points": int(hit.numel()), "view_surface_points": n_hit, "front_lit_pairs": pairs,
            "plain_ms": lvis_plain_ms, "grid_ms": lvis_grid_ms, "speedup": lvis_plain_ms / lvis_grid_ms,
            "plain_pairs_per_s": pairs / lvis_plain_ms * 1e3, "grid_pairs_per_s": pairs / lvis_grid_ms * 1e3,
            "plain_s_per_view": lvis_plain_ms * scale / 1e3, "grid_s_per_view": lvis_grid_ms * scale / 1e3,
            "evaluated_fraction": evaluated / seen, "differing_elements": int((lvis0 != lvis1).sum())}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
