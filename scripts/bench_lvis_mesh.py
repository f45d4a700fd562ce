#!/usr/bin/env python
"""Measures DESIGN.md section 3.11 on the GPU, on the NeRF fitted to a unit sphere (tests/golden), fine network, box +-1.5,
iso 0 — the set-up of scripts/bench_mesh_from_nerf.py:

  labelling   per res (128, 256): nfx_mesh_components alone (three launches into preallocated outputs) and the whole
              ops.mesh_filter_components (pre-check, labelling, read-back, selection and re-indexing in torch), next to the
              byte floor — faces read once plus labels written, over 8.0 TB/s (specification) and 6.3 TB/s (achievable);
              the number of components the fitted field really has; where scipy imports, scipy.sparse.csgraph.
              connected_components on the host for the same mesh.
  lvis        per 800 x 800 view (light_h = 16): compute_light_visibility (the density march) without and with the occupancy
              grid, and compute_light_visibility_mesh on the --keep_largest=1 mesh of each res; the host BVH build and the
              upload, paid once per process, listed separately.
  agreement   over the front-lit pairs of the view's hit pixels, march against the mesh route on the filtered and the
              unfiltered mesh: mean |difference|, the share of pairs with |difference| > 0.5, the share shadowed by one route
              only (march < 0.5 against mesh = 0) — also over the pixels with alpha > 0.5 alone.

Every GPU step is warmed up; a timed region is `inner` calls between two device events around a synchronised stretch, sized
to about a third of a second; `--reps` regions, median and spread (max - min) / median, per call.  The march of a whole view
takes tens of seconds: one call per region, `--march-reps` regions.  Nothing is asserted.  One JSON line; --out FILE also
writes it there.

    python scripts/bench_lvis_mesh.py [--res 128 256] [--imh 800] [--reps 5] [--march-reps 3] [--out profiles/lvis_mesh/bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
GRID_BOX = [-2.5, 2.5, -2.5, 2.5, -2.5, 2.5]      # scripts/bench_occupancy.py's: every shadow-ray sample lies inside
HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def region_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed(fn, reps, warm=3, inner=None):
    for _ in range(warm):
        fn()
    if inner is None:
        inner = max(1, int(300. / max(region_ms(fn, 2), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_call': med, 'spread': (ms[-1] - ms[0]) / med, 'calls_per_region': inner, 'regions': reps}


def host_timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {'ms_per_call': ms[len(ms) // 2], 'spread': (ms[-1] - ms[0]) / ms[len(ms) // 2], 'regions': reps}


def note(text):
    print('[bench_lvis_mesh] ' + text, file=sys.stderr, flush=True)


def agreement(march, mesh_lvis, front, rows=None):
    if rows is not None:
        march, mesh_lvis, front = march[rows], mesh_lvis[rows], front[rows]
    a, b = march[front], mesh_lvis[front]
    diff = (a - b).abs()
    return {'pairs': int(front.sum()), 'mean_abs_diff': float(diff.mean()), 'share_diff_above_half': float((diff > 0.5).float().mean()),
            'share_shadowed_by_march_only': float(((a < 0.5) & (b != 0)).float().mean()),
            'share_shadowed_by_mesh_only': float(((a >= 0.5) & (b == 0)).float().mean()),
            'march_mean': float(a.mean()), 'mesh_mean': float(b.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--imh', type=int, default=800)
    ap.add_argument('--light_h', type=int, default=16)
    ap.add_argument('--iso', type=float, default=0.)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--march-reps', type=int, default=3)
    ap.add_argument('--grid-res', type=int, default=128)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_lvis_mesh.py measures on an MI355X: no GPU is visible")
    from nerfactor_amd import build, synth
    build.build()
    from nerfactor_amd import _capi, mesh, ops
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor import mesh_from_nerf
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from nerfactor_amd.nerfactor.occupancy import OccupancyGrid
    from tests.golden import golden_inputs as gi
    from tests.test_gpu_render_from_nerf import fill_nerf
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cfg = make_config('nerf')
    model = get_model_class('nerf')(cfg)
    fill_nerf(model, gi.trained_nerf_nets())
    model = model.to(dev)
    result = {'device': torch.cuda.get_device_name(0), 'iso': args.iso, 'box': BOX, 'light_h': args.light_h, 'imh': args.imh,
              'labelling': {}, 'lvis': {}, 'agreement': {}}
    meshes = {}
    with torch.no_grad():
        # ---------------------------------------------------------------------------------------- 1. labelling
        for res in args.res:
            field = mesh_from_nerf.eval_lattice(model, BOX, res, 'fine')
            v, f = ops.isosurface(field, args.iso, *mesh_from_nerf.lattice_frame(BOX, res))
            nv, nf = int(v.shape[0]), int(f.shape[0])
            label = torch.empty((nv,), dtype=torch.int32, device=dev)
            ws = torch.empty((4,), dtype=torch.int32, device=dev)

            def raw():
                _capi.check(_capi.lib.nfx_mesh_components(f.data_ptr(), nf, nv, label.data_ptr(), ws.data_ptr(), 16,
                                                          torch.cuda.current_stream().cuda_stream), 'nfx_mesh_components')
            row = {'vertices': nv, 'triangles': nf}
            row['nfx_mesh_components'] = timed(raw, args.reps)
            row['mesh_filter_components'] = timed(lambda: ops.mesh_filter_components(v, f, keep_largest=1), args.reps)
            v1, f1, _, info = ops.mesh_filter_components(v, f, keep_largest=1)
            sizes = sorted((k[1] for k in mesh.filter_by_labels(v, f, label, min_faces=1)[3]['kept']), reverse=True)
            floor = 12 * nf + 4 * nv
            row.update(components=info['n_components'], largest_components_faces=sizes[:8], kept_vertices=int(v1.shape[0]),
                       kept_triangles=int(f1.shape[0]), floor_bytes=floor, floor_ms_at_spec=floor / HBM_SPEC * 1e3,
                       floor_ms_achievable=floor / HBM_ACHIEVABLE * 1e3,
                       floor_bytes_per_s=floor / (row['nfx_mesh_components']['ms_per_call'] * 1e-3))
            fh = f.cpu().numpy()
            if connected_components is not None:
                def host():
                    e = np.concatenate((fh[:, [0, 1]], fh[:, [1, 2]]))
                    g = coo_matrix((np.ones(e.shape[0], dtype=np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv))
                    return connected_components(g, directed=False)
                row['scipy_connected_components_host'] = host_timed(host, args.reps)
                row['scipy_components_with_unreferenced'] = int(host()[0])
            else:
                row['scipy_connected_components_host'] = 'not measured: scipy does not import'
            result['labelling'][str(res)] = row
            note('labelling at res %d: %s' % (res, json.dumps(row, sort_keys=True)))
            meshes[res] = {'whole': mesh.TriMesh(v.cpu().numpy(), fh), 'largest': mesh.TriMesh(v1.cpu().numpy(), f1.cpu().numpy())}
            del field
        # ---------------------------------------------------------------------------------------- 2. the view
        h = w = args.imh
        rayo_h, rayd_h = synth.camera_rays(h, w)
        rayo, rayd = torch.from_numpy(rayo_h).to(dev), torch.from_numpy(rayd_h).to(dev)
        d = torch.nn.functional.normalize(rayd, dim=1, eps=1e-12)
        occu, depth, normal = G.compute_depth_and_normal(model, rayo, d, cfg)
        alpha = occu.clamp(0., 1.)
        hit = torch.nonzero(alpha > 0)[:, 0]
        surf = (rayo[hit] + d[hit] * depth[hit, None]).contiguous()
        nrm = normal[hit].contiguous()
        lxyz = torch.as_tensor(G.gen_light_xyz(args.light_h, 2 * args.light_h)[0].reshape(-1, 3).astype(np.float32), device=dev)
        front = torch.cat([((torch.nn.functional.normalize(lxyz[None] - surf[lo:lo + 4096, None], dim=2, eps=1e-12)
                             * nrm[lo:lo + 4096, None]).sum(-1) > 0) for lo in range(0, surf.shape[0], 4096)])
        lv = result['lvis']
        lv.update(surface_points=int(hit.numel()), front_lit_pairs=int(front.sum()), lights=int(lxyz.shape[0]))
        grid = OccupancyGrid.bake(model, GRID_BOX, args.grid_res, 4, 10., 2)
        G.compute_light_visibility(model, surf[:256], nrm[:256], cfg, light_h=args.light_h)
        G.compute_light_visibility(model, surf[:256], nrm[:256], cfg, light_h=args.light_h, grid=grid)
        lv['march'] = timed(lambda: G.compute_light_visibility(model, surf, nrm, cfg, light_h=args.light_h), args.march_reps, warm=0, inner=1)
        note('march: %s' % json.dumps(lv['march']))
        lv['march_occupancy_grid'] = timed(lambda: G.compute_light_visibility(model, surf, nrm, cfg, light_h=args.light_h, grid=grid),
                                           args.march_reps, warm=0, inner=1)
        note('march with the grid: %s' % json.dumps(lv['march_occupancy_grid']))
        lv['occupancy_grid'] = {'res': args.grid_res, 'box': GRID_BOX}
        march = G.compute_light_visibility(model, surf, nrm, cfg, light_h=args.light_h, grid=grid).clamp(0., 1.)
        solid = alpha[hit] > 0.5
        lv['surface_points_alpha_above_half'] = int(solid.sum())
        for res in args.res:
            for which in ('largest', 'whole'):
                tri = meshes[res][which]
                vf, ff = tri.vertices.astype(np.float32), tri.faces
                key = 'res%d_%s' % (res, which)
                if which == 'largest':
                    build_ms = host_timed(lambda: ops.mesh_bvh_build(vf, ff, 4), 3)
                    blob = ops.mesh_bvh_build(vf, ff, 4)
                    upload = timed(lambda: torch.from_numpy(blob).to(dev), args.reps)
                    lv[key + '_bvh'] = {'host_build': build_ms, 'upload': upload, 'blob_bytes': int(blob.size)}
                inter = mesh.RayMeshIntersector(tri, device=dev)
                fn = lambda: G.compute_light_visibility_mesh(inter, surf, nrm, light_h=args.light_h, eps=0.1)
                if which == 'largest':
                    lv[key] = timed(fn, args.reps)
                    lv[key]['speedup_over_march'] = lv['march']['ms_per_call'] / lv[key]['ms_per_call']
                    lv[key]['speedup_over_march_occupancy_grid'] = lv['march_occupancy_grid']['ms_per_call'] / lv[key]['ms_per_call']
                by_mesh = fn()
                result['agreement'][key] = {'hit_pixels': agreement(march, by_mesh, front),
                                            'alpha_above_half': agreement(march, by_mesh, front, solid)}
                del by_mesh
                note('%s: %s %s' % (key, json.dumps(lv.get(key)), json.dumps(result['agreement'][key])))
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
