#!/usr/bin/env python
"""Times the explore_brdf_space workload: `--iden` identities (309 = the test split of the 100 MERL
materials) rendered on spheres of ims = 128, spp 1 and 4, under the 'point' probe (16 of 512 lights lit) and a full HDR
probe (every light lit), two ways in one process:

  fused     nfx_brdf_sphere_fwd: rows, cosine weighting and the sum over lights in one kernel, all identities per launch;
  composed  what the library offered before: per identity nfx_brdf_spec_fwd into an [n, L] buffer, then a torch reduction
            sum_l S * cos * lweight (cos [n, L] prepared once, outside the timing).  A measurement reference only.

The two alternate A/B/A/B, device events around synchronised regions, `--reps` regions each; median and spread (max - min)
/ median.  One JSON line; --out FILE also writes it there.

    python scripts/bench_brdf_spheres.py [--iden 309] [--ims 128] [--reps 5] [--out profiles/brdf_spheres/bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_ROW = 2 * (18 * 128 + 128 * 128 + 128 * 128 + (128 + 18) * 128 + 128)     # [z | pe2(rusink)] 18 -> 128 x 4 (skip) -> 1
MFMA_PEAK = 2.5e15                                                                 # bf16, dense


def region_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iden', type=int, default=309)
    ap.add_argument('--ims', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import _capi, ops
    from nerfactor_amd.brdf.renderer import SphereRenderer
    from oracle import nerfactor_ref as R
    dev = torch.device('cuda', 0)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    layers, out = R.init_mlp128(rng, 18, 1)
    ks = [k for k, _ in layers] + [out[0][0]]
    bs = [rng.uniform(-.2, .2, size=b.shape).astype(np.float32) for _, b in layers] + [out[0][1]]
    blob = ops.pack_mlp128_weights(ks, bs, _capi.IN_Z_RUSINK, 1, z_dim=3).to(dev)
    z = f32(rng.normal(0, .6, (args.iden, 3)))
    hdr = np.exp(np.random.default_rng(7).normal(size=(16, 32, 3)))
    result = {'iden': args.iden, 'ims': args.ims, 'reps': args.reps, 'flop_per_row': FLOP_PER_ROW, 'cases': []}
    for spp in (1, 4):
        base = SphereRenderer('white', ims=args.ims, spp=spp)
        fg = base.is_fg.reshape(-1)
        xyz, normal = f32(base.xyz.reshape(-1, 3)[fg]), f32(base.normal.reshape(-1, 3)[fg])
        n = xyz.shape[0]
        lxyz = f32(base.lxyz.reshape(-1, 3))
        L = lxyz.shape[0]
        cam = f32(np.broadcast_to(base.cam_loc, (n, 3)))
        lvis = base.lvis.reshape(fg.size, L)[fg] > 0
        cos = f32(np.where(lvis, base.lcos.reshape(fg.size, L)[fg], 0.))
        for probe in ('point', 'hdr'):
            light = (40. * (SphereRenderer('point', envmap_inten=1., ims=2).light) if probe == 'point' else hdr).reshape(L, 3)
            lweight = f32(light * base.lareas.reshape(L, 1))
            lit = (light != 0).any(1)
            rows_fused = int((lvis & lit[None, :]).sum()) * args.iden
            rows_composed = int(lvis.sum()) * args.iden

            def fused():
                return ops.brdf_sphere_fwd(xyz, normal, base.cam_loc, z, lxyz, lweight, blob)

            def composed():
                rgb = torch.empty((args.iden, n, 3), device=dev)
                for b in range(args.iden):
                    S = ops.brdf_spec_fwd(xyz, cam, normal, z[b:b + 1].expand(n, -1), lxyz, blob)
                    rgb[b] = (S * cos) @ lweight
                return rgb
            a, b = fused(), composed()                 # warm-up, and the two routes against each other
            scale = float(b.abs().max())
            diff = float((a - b).abs().max())
            tf, tc = [], []
            for _ in range(args.reps):
                tf.append(region_ms(fused)[0])
                tc.append(region_ms(composed)[0])
            case = {'spp': spp, 'probe': probe, 'fg_samples': n, 'lights': L, 'lit_lights': int(lit.sum()),
                    'max_abs_diff_fused_vs_composed': diff, 'max_abs_value': scale}
            for name, t, rows in (('fused', tf, rows_fused), ('composed', tc, rows_composed)):
                med = float(np.median(t))
                case[name] = {'ms': [round(v, 3) for v in t], 'median_ms': med, 'spread': (max(t) - min(t)) / med,
                              'ms_per_identity': med / args.iden, 'rows_evaluated': rows,
                              'tflops_on_evaluated_rows': rows * FLOP_PER_ROW / (med * 1e-3) / 1e12,
                              'share_of_mfma_peak': rows * FLOP_PER_ROW / (med * 1e-3) / MFMA_PEAK}
            case['speedup_fused_over_composed'] = case['composed']['median_ms'] / case['fused']['median_ms']
            result['cases'].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
