"""Timed loops (device events) of the training backward ops whose kernels share csrc/bwd_tile.hpp and csrc/mlp128_bwd_ring.hpp,
one op call per repetition, for A/B builds selected with NFX_LIB_PATH (profiles/bwd_tile/ab_times.txt), in the manner of
time_row_kernels.py:
    NFX_LIB_PATH=... python scripts/time_bwd_kernels.py
Shapes of a 1024-ray training step of bench.py: the light-visibility backward on 2048 points x 512 lights = 1 048 576 rows,
the NeRF backward on 1024 rays x 192 samples, the learned-BRDF backward on 2048 points x 512 lights.
Prints one JSON line: name -> [ms of every repetition]."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
assert os.environ.get('NFX_LIB_PATH')
from nerfactor_amd import _capi, ops  # noqa: E402
from tests import bwd_probes as bp  # noqa: E402
from tests.test_gpu_bwd_row_probes import buffers, dev as to_dev  # noqa: E402

dev = torch.device('cuda:0')
REPS = 7


def timed(fn, reps=REPS, warm=2, **kw):
    for k, v in kw.items():
        _capi.set_option(k, v)
    try:
        for _ in range(warm):
            fn()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(round(a.elapsed_time(b), 4))
        return out
    finally:
        for k in kw:
            _capi.unset_option(k)


res = {}
rng = np.random.default_rng(2)
N, L = 2048, 512
f = {k: to_dev(v, dev) for k, v in bp.ldir_fill(N, L).items()}

# light visibility: IN_XYZ_LDIR, one sigmoid output
ks, bs = bp.net128(bp.LDIR_SEED, 90, 1)
blob = ops.pack_mlp128_train_weights(ks, bs, _capi.IN_XYZ_LDIR, 1).to(dev)
_, dks, dbs = buffers(ks, bs, dev)
dout = to_dev(rng.normal(size=(N, L)), dev)
lvis = lambda: ops.mlp128_bwd(_capi.IN_XYZ_LDIR, f['xyz'], dout, blob, dks, dbs, out_act='sigmoid', lxyz=f['lxyz'], xyz_dir=f['xyz_dir'])
res['mlp128_bwd lvis default (mlp128_bwd_fused_kernel<1, *>, text identical)'] = timed(lvis)
res['mlp128_bwd lvis wgrad_fused 0 (mlp128_bwd_ring_kernel<1> + GEMMs)'] = timed(lvis, wgrad_fused=0)
res['mlp128_bwd lvis wgrad_fused 0 m128_bwd 0 (mlp128_bwd_kernel<1> + GEMMs)'] = timed(lvis, wgrad_fused=0, m128_bwd=0)

# one xyz head: IN_XYZ, three linear outputs, on the step's 2048 points and on as many rows as the light-visibility call
for n in (N, N * L):
    x = to_dev(rng.uniform(-1, 1, size=(n, 3)), dev)
    kx, bx = bp.net128(83, 63, 3)
    xblob = ops.pack_mlp128_train_weights(kx, bx, _capi.IN_XYZ, 3).to(dev)
    _, xdk, xdb = buffers(kx, bx, dev)
    xdout = to_dev(rng.normal(size=(n, 3)), dev)
    head = lambda: ops.mlp128_bwd(_capi.IN_XYZ, x, xdout, xblob, xdk, xdb, xyz_scale=bp.XYZ_SCALE)
    res['mlp128_bwd xyz %d rows default (mlp128_bwd_fused_kernel<0, *>, text identical)' % n] = timed(head)
    res['mlp128_bwd xyz %d rows wgrad_fused 0 (mlp128_bwd_ring_kernel<0> + GEMMs)' % n] = timed(head, wgrad_fused=0)
    res['mlp128_bwd xyz %d rows wgrad_fused 0 m128_bwd 0 (mlp128_bwd_kernel<0> + GEMMs)' % n] = timed(head, wgrad_fused=0, m128_bwd=0)

# NeRF: 1024 rays x (64 + 128) samples; half of the points carry no gradient, as behind the composite
R, S = 1024, 192
nk, nb = bp.nerf_layers()
nblob = ops.pack_nerf_train_weights(nk, nb).to(dev)
_, ndk, ndb = buffers(nk, nb, dev)
nf = {k: to_dev(v, dev) for k, v in bp.nerf_fill(R, S).items()}
d = to_dev(rng.normal(size=(R, S, 4)) * (rng.uniform(size=(R, S, 1)) < .5), dev)
nerf = lambda: ops.nerf_mlp_bwd(nf['rayo'], nf['rayd'], nf['z'], d, nblob, ndk, ndb)
res['nerf_mlp_bwd default (nerf_bwd_ring_kernel<8, true>, text identical)'] = timed(nerf)
res['nerf_mlp_bwd nerf_bwd_rows 0 (nerf_bwd_ring_kernel<8, false>, text identical)'] = timed(nerf, nerf_bwd_rows=0)
res['nerf_mlp_bwd nerf_bwd_nw 4 (nerf_bwd_ring_kernel<4, true>, text identical)'] = timed(nerf, nerf_bwd_nw=4)
res['nerf_mlp_bwd nerf_bwd 0 (nerf_bwd_kernel, text identical)'] = timed(nerf, nerf_bwd=0)

# learned BRDF: 2048 points x 512 lights, 60 % of the rows with a gradient
ZD = 3
kb, bb = bp.net128(700 + ZD, ZD + 15, 1)
tblob = ops.pack_brdf_train_weights(kb, bb, ZD).to(dev)
g = {k: to_dev(v, dev) for k, v in bp.brdf_spec_fill(N, L, ZD).items()}
dspec = to_dev(rng.normal(size=(N, L)) * (rng.uniform(size=(N, L)) < .6), dev)
brdf = lambda: ops.brdf_spec_bwd(g['xyz'], g['cam'], g['normal'], g['z'], g['lxyz'], tblob, dspec)
res['brdf_spec_bwd default (brdf_spec_bwd_kernel<true>, text identical)'] = timed(brdf)
res['brdf_spec_bwd brdf_bwd_rows 0 (brdf_spec_bwd_kernel<false>, text identical)'] = timed(brdf, brdf_bwd_rows=0)
print(json.dumps({'lib': os.environ['NFX_LIB_PATH'], 'ms': res}), flush=True)
