"""Timed loops (device events) of the learned-BRDF row kernels that fill their operand through csrc/brdf_row.hpp, one launch
per repetition, for A/B builds selected with NFX_LIB_PATH (profiles/brdf_row/ab_times.txt):
    NFX_LIB_PATH=... python scripts/time_row_kernels.py
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
from tests import bwd_probes as bp, row_mlp_cases as rc  # noqa: E402
from tests.test_gpu_bwd_row_probes import buffers  # noqa: E402
from tests.test_gpu_nerfactor import dev as to_dev, pack  # noqa: E402

dev = torch.device('cuda:0')
REPS = 7


def timed(fn, reps=REPS, warm=2):
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


def with_options(fn, **kw):
    for k, v in kw.items():
        _capi.set_option(k, v)
    try:
        return timed(fn)
    finally:
        for k in kw:
            _capi.unset_option(k)


res = {}
rng = np.random.default_rng(1)
N, L, ZD = 384000, 512, 3                 # 60 % of an 800 x 800 view, 512 lights: the surface batch of bench.py's nerfactor leg
d = rng.normal(size=(L, 3))
nr = rng.normal(size=(N, 3))
f = {'xyz': rng.uniform(-.3, .3, size=(N, 3)), 'cam': np.broadcast_to(rc.CAM, (N, 3)), 'normal': nr / np.linalg.norm(nr, axis=1, keepdims=True),
     'z': rng.normal(size=(N, ZD)), 'lxyz': 5. * d / np.linalg.norm(d, axis=1, keepdims=True)}
f = {k: to_dev(v, dev) for k, v in f.items()}
blob = {p: pack(*rc.brdf_net(ZD), _capi.IN_Z_RUSINK, 1, dev, z_dim=ZD, prec=p) for p in ('bf16', 'fp32')}
fwd = lambda p='bf16': ops.brdf_spec_fwd(f['xyz'], f['cam'], f['normal'], f['z'], f['lxyz'], blob[p], prec=p)
res['brdf_spec_fwd default (compact<4,1,4>, text identical)'] = timed(fwd)
for v in (2, 3, 4):
    res['brdf_spec_fwd brdf_variant %d (resident128<%d,1,4>)' % (v, v)] = with_options(fwd, brdf_variant=v)
res['brdf_spec_fwd brdf_variant 6 brdf_ct 3 (compact<3,1,4>)'] = with_options(fwd, brdf_variant=6, brdf_ct=3)
res['brdf_spec_fwd brdf_variant 0 (brdf_spec_kernel)'] = with_options(fwd, brdf_variant=0)
res['brdf_spec_fwd prec fp32 (mlp128_x3_kernel<2>)'] = timed(lambda: fwd('fp32'))

NB = 8192                                 # backward: 8192 points x 512 lights, 60 % of the rows with a gradient
ks, bs = bp.net128(700 + ZD, ZD + 15, 1)
tblob = ops.pack_brdf_train_weights(ks, bs, ZD).to(dev)
g = {k: (v if k == 'lxyz' else v[:NB].contiguous()) for k, v in f.items()}
dspec = to_dev(rng.normal(size=(NB, L)) * (rng.uniform(size=(NB, L)) < .6), dev)
bwd = lambda: ops.brdf_spec_bwd(g['xyz'], g['cam'], g['normal'], g['z'], g['lxyz'], tblob, dspec)
res['brdf_spec_bwd brdf_bwd_rows 0 (brdf_spec_bwd_kernel<false>)'] = with_options(bwd, brdf_bwd_rows=0)
res['brdf_spec_bwd default (brdf_spec_bwd_kernel<true>)'] = timed(bwd)

NR = 1 << 20                              # the prior on explicit rows: 2^20 rows + their reciprocal halves
rf = bp.brdf_rows_fill(NR)
zr, rus = to_dev(rf['z'], dev), to_dev(rf['rusink'], dev)
kr, br = bp.net128(bp.BRDF_ROWS_SEED, bp.BRDF_ROWS_ZDIM + 15, 1)
rblob = ops.pack_brdf_train_weights(kr, br, bp.BRDF_ROWS_ZDIM).to(dev)
res['brdf_rows_fwd (brdf_rows_kernel<false>)'] = timed(lambda: ops.brdf_rows_fwd(zr, rus, rblob, reci=True))
flat, dks, dbs = buffers(kr, br, dev)
dout = to_dev(rng.normal(size=2 * NR), dev)
res['brdf_rows_bwd (brdf_rows_kernel<true> + weight-gradient GEMMs)'] = timed(lambda: ops.brdf_rows_bwd(zr, rus, rblob, dout, dks, dbs, reci=True))
print(json.dumps({'lib': os.environ['NFX_LIB_PATH'], 'ms': res}), flush=True)
