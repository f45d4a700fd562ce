#!/usr/bin/env python
"""Per-view cost of rendering a trained NeRFactor from camera rays: the direct route (render_from_nerf.py:
nerfactor/surface.py:march_surface, then Model.call(mode='test', relight_probes=True)) against what the disk route
computes for the same view (geometry_from_nerf's compute_depth_and_normal and compute_light_visibility over the view's
surface points, then the same render).  One 800 x 800 view of the NeRF fitted to a scene (tests/golden/
nerf_trained_fp16.npz, a unit sphere), a nerfactor_microfacet model (random weights, 8 probes).  One JSON line.

    python scripts/bench_render_from_nerf.py [--imh 800] [--reps 3] [--lvis-points 0] [--skip-geometry]

The disk route's file writes (xyz / normal / lvis .npy, 1.3 GB per 800 x 800 view) and test.py's reads are not timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn, reps):
    """(median ms of `reps` calls after one warm-up call, last result)."""
    out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--imh', type=int, default=800)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--lvis-points', type=int, default=0, help="surface points of the shadow-ray march (0: all of the view's)")
    ap.add_argument('--skip-geometry', action='store_true', help="the direct route only (e.g. under a profiler)")
    args = ap.parse_args()
    from nerfactor_amd import build, synth
    build.build()
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.surface import march_surface, nerfactor_test_batch
    from tests.golden import golden_inputs as gi
    dev = torch.device('cuda', 0)
    h = w = args.imh
    nerf_cfg = make_config('nerf')
    nerf = get_model_class('nerf')(nerf_cfg)
    with torch.no_grad():
        for pref, net in zip(('coarse_', 'fine_'), gi.trained_nerf_nets()):
            for part in ('enc', 'sigma_out', 'bottleneck', 'rgb_out'):
                for layer, (k, b) in zip(nerf.net[pref + part].layers, net[part]):
                    layer.kernel.copy_(torch.from_numpy(np.asarray(k, np.float32)))
                    layer.bias.copy_(torch.from_numpy(np.asarray(b, np.float32)))
    nerf = nerf.to(dev)
    torch.manual_seed(5)
    name = 'nerfactor_microfacet'
    model = get_model_class(name)(make_config(name, shape_mode='finetune', shape_model_ckpt='none', brdf_model_ckpt='none',
                                              test_envmap_dir='', xyz_jitter_std='0')).to(dev)
    for i, p in enumerate(synth.probes(8, seed=20)):
        model.add_probe('p%d' % i, p)
    rayo_h, rayd_h = synth.camera_rays(h, w)
    rayo, rayd = torch.from_numpy(rayo_h).to(dev), torch.from_numpy(rayd_h).to(dev)
    out = {"workload": "one %d x %d view: NeRF fitted to a unit sphere (tests/golden/nerf_trained_fp16.npz; 128 coarse + 320 "
                       "fine-network density samples per ray), nerfactor_microfacet render with 8 probes" % (h, w),
           "reps": args.reps}
    with torch.no_grad():
        march_ms, (alpha, xyz) = timed_ms(lambda: march_surface(nerf, rayo, rayd, nerf_cfg), args.reps)
        batch = nerfactor_test_batch('view', (h, w), rayo, rayd, alpha, xyz)
        render_ms, pred = timed_ms(lambda: model(batch, mode='test', relight_probes=True)[0], args.reps)
        n_fg = int((alpha > 0).sum())
        out.update({"foreground_rays": n_fg, "finite": bool(torch.isfinite(pred['rgb']).all()),
                    "direct": {"march_surface_ms": march_ms, "render_ms": render_ms,
                               "per_view_ms": march_ms + render_ms}})
        if not args.skip_geometry:
            d = torch.nn.functional.normalize(rayd, dim=1, eps=1e-12)
            dn_ms, (occu, depth, normal) = timed_ms(lambda: G.compute_depth_and_normal(nerf, rayo, d, nerf_cfg),
                                                    max(1, min(args.reps, 2)))
            hit = torch.nonzero(occu.clamp(0., 1.) > 0)[:, 0]          # process_view: the shadow rays of alpha > 0
            n_hit = hit.numel()
            if args.lvis_points:
                hit = hit[torch.linspace(0, hit.numel() - 1, args.lvis_points, device=dev).long()]
            surf = (rayo[hit] + d[hit] * depth[hit, None]).contiguous()
            nrm = normal[hit].contiguous()
            G.compute_light_visibility(nerf, surf[:256], nrm[:256], nerf_cfg)           # warm-up (packing)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            G.compute_light_visibility(nerf, surf, nrm, nerf_cfg)
            torch.cuda.synchronize()
            lvis_ms = (time.perf_counter() - t0) * 1e3
            full = not args.lvis_points
            lvis_view_ms = lvis_ms if full else lvis_ms * n_hit / max(1, hit.numel())
            out["disk_route"] = {
                "depth_normal_ms": dn_ms, "lvis_points": int(hit.numel()), "lvis_ms": lvis_ms,
                "lvis_ms_per_view": lvis_view_ms, "lvis_per_view_measured": bool(full), "render_ms": render_ms,
                "per_view_ms_without_file_io": dn_ms + lvis_view_ms + render_ms}
            out["speedup"] = out["disk_route"]["per_view_ms_without_file_io"] / out["direct"]["per_view_ms"]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
