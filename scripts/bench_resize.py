#!/usr/bin/env python
"""Times DESIGN.md section 3.13 on the GPU: nfx_resize_antialias on the two workloads it was written for, next to their byte
floors (input bytes plus output bytes over 6.3 TB/s, the achievable HBM rate) and next to the host paths they replace.

    buffer    one [1, 800, 800, 512] float32 light-visibility buffer -> 512 x 512 float32 (what nerf_shape / mvs_shape do when
              imh is below the buffers' resolution)
    photos    sixteen [3024, 4032, 3] uint8 photographs -> [512, 682] uint8 (nerf_real.make_dataset), one launch per
              photograph as the driver does, and as one batched launch

Per workload: `kernel` — the launch alone into a preallocated output, a timed region of calls between two device events, the
median of --reps regions; `floor` — bytes, the time at 6.3 TB/s and the fraction of that rate the kernel reaches; `end_to_end`
— upload, launch and download of host arrays (wall clock, synchronised); `host_pil` — datasets.nerf.resize, the per-channel
PIL loop that is the readers' present path, on the same arrays; `host_einsum` — util.light.resize_antialias, the host filter
of --device cpu, timed on --host-slice channels / photographs only because it takes minutes on the whole (its cost is linear in
them; `scaled_s` is the measured time times the ratio, `measured_on` says what was run).  Nothing is asserted.  One JSON line;
--out FILE also writes it there.

    python scripts/bench_resize.py [--reps 5] [--host-slice 32] [--out profiles/resize/bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12


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
    inner = max(1, int(200. / max(region_ms(fn, 2), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_call': med, 'spread': (ms[-1] - ms[0]) / med, 'calls_per_region': inner, 'regions': reps}


def wall(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return sorted(out)[len(out) // 2]


def floor_of(in_bytes, out_bytes, kernel_ms):
    ms = (in_bytes + out_bytes) / HBM_ACHIEVABLE * 1e3
    return {'bytes': in_bytes + out_bytes, 'ms_at_achievable': ms, 'fraction_of_achievable': ms / kernel_ms}


def say(msg):
    print('# ' + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-slice', type=int, default=32, help="channels of the buffer the einsum host filter is timed on")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import ops
    from nerfactor_amd.nerfactor.datasets.nerf import resize as host_pil
    from nerfactor_amd.nerfactor.util.light import resize_antialias as host_einsum
    res = {'hbm_achievable': HBM_ACHIEVABLE}
    rng = np.random.default_rng(0)

    # ---- the light-visibility buffer
    buf = rng.random((800, 800, 512), dtype=np.float32)
    x = torch.from_numpy(buf).cuda()[None]
    out = torch.empty((1, 512, 512, 512), dtype=torch.float32, device='cuda')
    w = {'shape': [1, 800, 800, 512], 'to': [512, 512], 'dtype': 'float32'}
    w['kernel'] = timed(lambda: ops.resize_antialias(x, 512, 512, out=out), args.reps)
    w['floor'] = floor_of(x.numel() * 4, out.numel() * 4, w['kernel']['ms_per_call'])
    say('buffer kernel %.3f ms' % w['kernel']['ms_per_call'])
    w['end_to_end_s'] = wall(lambda: ops.resize_antialias(torch.from_numpy(buf).cuda(), 512, 512).cpu().numpy())
    del x, out
    torch.cuda.empty_cache()
    t = time.perf_counter()
    host_pil(buf, 512)
    w['host_pil_s'] = time.perf_counter() - t
    say('buffer host PIL %.2f s' % w['host_pil_s'])
    n = min(args.host_slice, 512)
    part = np.ascontiguousarray(buf[:, :, :n])
    t = time.perf_counter()
    host_einsum(part, 512, 512)
    dt = time.perf_counter() - t
    w['host_einsum'] = {'measured_on': '%d of 512 channels' % n, 'measured_s': dt, 'scaled_s': dt * 512 / n}
    say('buffer host einsum %.2f s on %d channels' % (dt, n))
    w['speedup_end_to_end_vs_host_pil'] = w['host_pil_s'] / w['end_to_end_s']
    res['buffer'] = w
    del buf, part

    # ---- the photographs
    photos = rng.integers(0, 256, (16, 3024, 4032, 3), dtype=np.uint8)
    x = torch.from_numpy(photos).cuda()
    out = torch.empty((16, 512, 682, 3), dtype=torch.uint8, device='cuda')
    w = {'shape': [16, 3024, 4032, 3], 'to': [512, 682], 'dtype': 'uint8 -> uint8'}

    def one_by_one():
        for i in range(16):
            ops.resize_antialias(x[i], 512, 682, out_uint8=True, out=out[i])

    w['kernel'] = timed(one_by_one, args.reps)
    w['kernel_batched'] = timed(lambda: ops.resize_antialias(x, 512, 682, out_uint8=True, out=out), args.reps)
    w['floor'] = floor_of(x.numel(), out.numel(), w['kernel']['ms_per_call'])
    w['floor_batched'] = floor_of(x.numel(), out.numel(), w['kernel_batched']['ms_per_call'])
    say('photos kernel %.3f ms, batched %.3f ms' % (w['kernel']['ms_per_call'], w['kernel_batched']['ms_per_call']))
    assert int(ops.resize_antialias(x[0], new_h=512).shape[1]) == 682
    del x, out
    torch.cuda.empty_cache()

    def driver_route():
        for i in range(16):
            ops.resize_antialias(torch.from_numpy(photos[i]).cuda(), new_h=512, out_uint8=True).cpu().numpy()

    w['end_to_end_s'] = wall(driver_route)
    t = time.perf_counter()
    for i in range(16):
        host_pil(photos[i].astype(np.float32) / np.float32(255), 512)
    w['host_pil_s'] = time.perf_counter() - t
    say('photos host PIL %.2f s' % w['host_pil_s'])
    t = time.perf_counter()
    host_einsum(photos[0].astype(np.float32) / np.float32(255), new_h=512)
    dt = time.perf_counter() - t
    w['host_einsum'] = {'measured_on': '1 of 16 photographs', 'measured_s': dt, 'scaled_s': dt * 16}
    w['speedup_end_to_end_vs_host_pil'] = w['host_pil_s'] / w['end_to_end_s']
    res['photos'] = w
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
