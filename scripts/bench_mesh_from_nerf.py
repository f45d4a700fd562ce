#!/usr/bin/env python
"""Times the three steps of nerfactor/mesh_from_nerf.py on the NeRF fitted to a unit sphere
(tests/golden), box +-1.5, iso 0, fine network, at res 128 and 256, on the GPU:

  lattice     the network's raw density on the res^3 lattice (nfx_nerf_sigma_fwd in chunks, mesh_from_nerf.eval_lattice);
  count       nfx_isosurface_count (four launches) on that lattice;
  emit        nfx_isosurface_emit into preallocated outputs;
  isosurface  ops.isosurface as the driver calls it: the finiteness pass, count, the host read of the totals, the two
              allocations, emit;
  normals     nfx_nerf_sigma_grad at the vertices (mesh_from_nerf.gradient_normals).

Every step is warmed up; a timed region is `inner` calls between two device events around a synchronised stretch, sized to
about a third of a second; `--reps` regions, median and spread (max - min) / median, per call.  Next to count + emit the byte
floor: (lattice bytes x 2 passes + output bytes) over 8.0 TB/s (specification) and 6.3 TB/s (achievable), and the bytes the
two passes really move (the workspace written by count and read by emit included).  No threshold is asserted: nothing
earlier exists to compare with.  One JSON line; --out FILE also writes it there.

    python scripts/bench_mesh_from_nerf.py [--res 128 256] [--precision bf16] [--reps 5] [--out profiles/mesh_from_nerf/bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
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


def timed(fn, reps):
    for _ in range(3):
        fn()
    inner = max(1, int(300. / max(region_ms(fn, 2), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_call': med, 'spread': (ms[-1] - ms[0]) / med, 'calls_per_region': inner, 'regions': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--iso', type=float, default=0.)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mesh_from_nerf.py measures on an MI355X: no GPU is visible")
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import ops
    from nerfactor_amd.nerfactor import mesh_from_nerf
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    from tests.golden import golden_inputs as gi
    from tests.test_gpu_render_from_nerf import fill_nerf
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = get_model_class('nerf')(make_config('nerf', precision=args.precision))
    fill_nerf(model, gi.trained_nerf_nets())
    model = model.to(dev)
    result = {'device': torch.cuda.get_device_name(0), 'precision': args.precision, 'iso': args.iso, 'box': BOX, 'res': {}}
    for res in args.res:
        row = {}
        row['lattice'] = timed(lambda: mesh_from_nerf.eval_lattice(model, BOX, res, 'fine'), args.reps)
        field = mesh_from_nerf.eval_lattice(model, BOX, res, 'fine')
        origin, spacing = mesh_from_nerf.lattice_frame(BOX, res)
        ws = ops.isosurface_workspace(field.shape, dev)
        row['count'] = timed(lambda: ops.isosurface_count(field, args.iso, ws), args.reps)
        nv, nf, overflow = ws[:3].tolist()
        assert not overflow
        v = torch.empty((nv, 3), device=dev)
        f = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        row['emit'] = timed(lambda: ops.isosurface_emit(field, args.iso, origin, spacing, ws, nv, nf, v, f), args.reps)
        row['isosurface'] = timed(lambda: ops.isosurface(field, args.iso, origin, spacing), args.reps)
        row['normals'] = timed(lambda: mesh_from_nerf.gradient_normals(model, v, 'fine'), args.reps)
        n = res ** 3
        floor_bytes = 2 * 4 * n + 12 * nv + 12 * nf
        moved_bytes = floor_bytes + 2 * 10 * n      # count writes, emit reads: two offsets and two bytes per point
        both = row['count']['ms_per_call'] + row['emit']['ms_per_call']
        row.update(points=n, vertices=nv, triangles=nf, workspace_bytes=ws.numel() * 4, floor_bytes=floor_bytes, moved_bytes=moved_bytes,
                   floor_ms_at_spec=floor_bytes / HBM_SPEC * 1e3, floor_ms_achievable=floor_bytes / HBM_ACHIEVABLE * 1e3,
                   count_plus_emit_ms=both, moved_bytes_per_s=moved_bytes / (both * 1e-3))
        result['res'][str(res)] = row
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
