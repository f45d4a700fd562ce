#!/usr/bin/env python
"""Times DESIGN.md section 3.12 on the GPU: ONE nfx_image_metrics call (its two launches) scoring 64 pairs of 800 x 800 uint8
RGB images on the luma, into preallocated totals and workspace, next to its byte floor — both images read once, 2 B H W C
bytes, over 8.0 TB/s (specification) and 6.3 TB/s (achievable).  Also the same call with the SSIM map written, the
float32 and per-channel forms, and the whole ops.image_metrics (allocation, the B x 8 read-back and the host arithmetic).

Every step is warmed up; a timed region is `inner` calls between two device events around a synchronised stretch, sized to
about a third of a second; `--reps` regions, median and spread (max - min) / median, per call.  Nothing is asserted.  One
JSON line; --out FILE also writes it there.

    python scripts/bench_image_metrics.py [--batch 64] [--imh 800] [--reps 5] [--out profiles/image_metrics/bench.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    inner = max(1, int(300. / max(region_ms(fn, 2), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_call': med, 'spread': (ms[-1] - ms[0]) / med, 'calls_per_region': inner, 'regions': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--imh', type=int, default=800)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import _capi, ops
    dev = torch.device('cuda:0')
    B, H, W, C = args.batch, args.imh, args.imh, 3
    gen = torch.Generator(device='cpu').manual_seed(0)
    a8 = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=gen).to(dev)
    b8 = (a8.to(torch.int16) + torch.randint(-8, 9, (B, H, W, C), dtype=torch.int16, generator=gen).to(dev)).clamp(0, 255).to(torch.uint8)
    g = (ctypes.c_double * 11)(*ops.IMAGE_METRICS_WEIGHTS)
    totals = torch.empty((B, 8), dtype=torch.int64, device=dev)
    smap = torch.empty((B, H - 10, W - 10, 3), dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(a, b, luma, with_map):
        nbytes = _capi.lib.nfx_image_metrics_workspace_bytes(B, H, W, C, int(luma))
        ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
        is_float, max_val = int(a.dtype == torch.float32), 1. if a.dtype == torch.float32 else 255.
        m = ctypes.c_void_p(smap.data_ptr()) if with_map else None

        def call():
            _capi.check(_capi.lib.nfx_image_metrics(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), is_float, B, H, W, C,
                                                    max_val, int(luma), None, m, ctypes.cast(g, ctypes.c_void_p),
                                                    ctypes.c_void_p(totals.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes, stream),
                        'nfx_image_metrics')
        return call

    floor_bytes = 2 * B * H * W * C
    res = {'shape': [B, H, W, C], 'byte_floor': {'bytes': floor_bytes, 'ms_at_spec': floor_bytes / HBM_SPEC * 1e3,
                                                'ms_at_achievable': floor_bytes / HBM_ACHIEVABLE * 1e3}}
    res['uint8_luma'] = timed(raw(a8, b8, True, False), args.reps)
    res['uint8_luma']['times_floor_at_achievable'] = res['uint8_luma']['ms_per_call'] / res['byte_floor']['ms_at_achievable']
    res['uint8_luma_with_map'] = timed(raw(a8, b8, True, True), args.reps)
    res['uint8_per_channel'] = timed(raw(a8, b8, False, False), args.reps)
    af, bf = a8.float() / 255., b8.float() / 255.
    res['float32_luma'] = timed(raw(af, bf, True, False), args.reps)
    del af, bf
    res['ops_image_metrics_uint8_luma'] = timed(lambda: ops.image_metrics(a8, b8, 255.), args.reps)
    out = ops.image_metrics(a8, b8, 255.)
    res['mean_psnr'], res['mean_ssim'] = float(out['psnr'].mean()), float(out['ssim'].mean())
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
