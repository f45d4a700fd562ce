#!/usr/bin/env python
"""Times the two measured-BRDF kernels at the size make_dataset runs them, on the GPU:

  query    nfx_merl_query over the render rows of a 128^2, 512-light test.npz (about 2 M rows: every front-lit (sample,
           light) pair; the 8100 slice coordinates in front);
  sphere   one fused nfx_merl_sphere_fwd render of the same scene under the 'white' probe, so that every light is lit.

The material is the seeded synthetic table of tests/merl_cases.py (no MERL file ships with the repository).  Every shape is
warmed up, a timed region is `inner` launches between two device events around a synchronised stretch and is sized to
about a third of a second; `--reps` regions, median and spread (max - min) / median, per launch.

The yardstick is the reference's route on the CPU of the same machine, when SciPy is there (else null): cKDTree build +
query of the same rows, and the host renderer's sum over lights of the looked-up rows (SphereRenderer.render).  No ratio is
asserted.  One JSON line; --out FILE also writes it there.

    python scripts/bench_merl.py [--ims 128] [--reps 5] [--out profiles/merl/bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    inner = max(1, int(300. / max(region_ms(fn, 5), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_launch': med, 'spread': (ms[-1] - ms[0]) / med, 'launches_per_region': inner, 'regions': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ims', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_merl.py measures on an MI355X: no GPU is visible")
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import ops
    from nerfactor_amd.brdf import merl
    from nerfactor_amd.brdf.renderer import SphereRenderer
    from nerfactor_amd.data_gen.merl import make_dataset
    from tests import merl_cases as mc
    dev = torch.device('cuda', 0)
    m = merl.MERL()
    m.cube_rgb = mc.synthetic_cube(0)
    table = m.device_table(dev)
    r = SphereRenderer('white', envmap_inten=1., envmap_h=16, ims=args.ims, spp=1)
    scene = r.device_scene(dev)
    rows = make_dataset.test_coordinates(r)
    q = torch.as_tensor(rows, device=dev)
    result = {'ims': args.ims, 'lights': int(scene['lxyz'].shape[0]), 'samples': int(scene['xyz'].shape[0]), 'rows': int(rows.shape[0]),
              'device': torch.cuda.get_device_name(0)}
    result['query'] = timed(lambda: ops.merl_query(table, q), args.reps)
    result['query']['rows_per_s'] = rows.shape[0] / (result['query']['ms_per_launch'] * 1e-3)
    result['sphere'] = timed(lambda: ops.merl_sphere_fwd(scene['xyz'], scene['normal'], r.cam_loc, table, scene['lxyz'], scene['lweight']),
                             args.reps)
    result['sphere']['rows_per_s'] = (rows.shape[0] - 8100) / (result['sphere']['ms_per_launch'] * 1e-3)
    # the two routes compute the same picture
    fused = m.render_sphere(r, device=dev).cpu().numpy()
    lvis = r.lvis.astype(bool)
    brdf = np.zeros(r.lcontrib.shape)
    brdf[lvis] = ops.merl_query(table, q[8100:]).cpu().numpy()
    result['max_abs_fused_minus_rows'] = float(np.abs(fused - r.render(brdf)).max())
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        result['cpu_reference'] = None
    else:
        tbl = m.tbl
        t0 = time.perf_counter()
        tree = cKDTree(tbl[:, :3])
        t1 = time.perf_counter()
        _, ind = tree.query(rows.astype(np.float64))
        t2 = time.perf_counter()
        brdf[lvis] = tbl[ind[8100:], 3:]
        t3 = time.perf_counter()
        r.render(brdf)
        t4 = time.perf_counter()
        result['cpu_reference'] = {'kdtree_build_ms': (t1 - t0) * 1e3, 'kdtree_query_ms': (t2 - t1) * 1e3,
                                   'render_sum_ms': (t4 - t3) * 1e3, 'runs': 1,
                                   'what': "scipy.spatial.cKDTree over the valid entries, one thread; SphereRenderer.render of the looked-up rows"}
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
