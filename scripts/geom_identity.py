"""Outputs of the density / density-gradient kernels (nerf_geom.hip, nerf_geom_x3.hip, nerf_sigma_x3_pipe.hip) and the bytes
of the fp32-class packers, saved (first call) or compared bit for bit (later calls): the check for a change of these sources
that must not change a single bit.  One process per library:
    NFX_LIB_PATH=old.so python scripts/geom_identity.py save;  python scripts/geom_identity.py check
    ... save --pack-only / check --pack-only: the packers alone (no GPU)
The 840-point sets of tests/nerf_point_cases.py ('glorot', 'fitted'), as [8, 105] and [120, 7]."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfactor_amd import build  # noqa: E402

if not os.environ.get('NFX_LIB_PATH'):
    build.build()
import torch  # noqa: E402
from nerfactor_amd import _capi, ops  # noqa: E402
from tests import common, nerf_point_cases as pc  # noqa: E402

mode = sys.argv[1]
pack_only = '--pack-only' in sys.argv
path = os.path.join(ROOT, 'build', 'geom_identity_pack.pt' if pack_only else 'geom_identity.pt')     # build/ is not tracked
out = {}


def option(key, value, fn):
    _capi.set_option(key, value)
    try:
        return fn()
    finally:
        _capi.unset_option(key)


# ------------------------------------------------------------------------------------------ the packers' bytes, prec = 'fp32'
for name in pc.SETS:
    ks, bs = common.nerf_layers(pc.point_set(name).net)
    out['pack_nerf_weights/' + name] = ops.pack_nerf_weights(ks, bs, 'fp32')
    out['pack_nerf_geom_weights/' + name] = ops.pack_nerf_geom_weights(ks, bs, 'fp32')
rng = np.random.default_rng(128)
for in_kind, z_dim, out_dim in ((_capi.IN_XYZ, 0, 3), (_capi.IN_XYZ_LDIR, 0, 1), (_capi.IN_Z_RUSINK, 3, 1)):
    in_dims = {_capi.IN_XYZ: 63, _capi.IN_XYZ_LDIR: 90, _capi.IN_Z_RUSINK: z_dim + 15}[in_kind]
    shapes = [(in_dims, 128), (128, 128), (128, 128), (128 + in_dims, 128), (128, out_dim)]
    ks = [rng.normal(size=s).astype(np.float32) / np.sqrt(s[0]) for s in shapes]
    bs = [rng.normal(size=s[1]).astype(np.float32) * .1 for s in shapes]
    out['pack_mlp128_weights/%d_%d_%d' % (in_kind, z_dim, out_dim)] = ops.pack_mlp128_weights(ks, bs, in_kind, out_dim, z_dim, 'fp32')

# ------------------------------------------------------------------------------------------------------------- the kernels
if not pack_only:
    dev = torch.device('cuda:0')
    for name in pc.SETS:
        ps = pc.point_set(name)
        blob = {p: ops.pack_nerf_geom_weights(*common.nerf_layers(ps.net), prec=p).to(dev) for p in ('bf16', 'fp32')}
        picked = np.random.default_rng(840).permutation(pc.N)[:333].astype(np.int32)
        lst = torch.full((pc.N,), -1, dtype=torch.int32, device=dev)
        lst[:333] = torch.from_numpy(picked).to(dev)
        cnt = torch.tensor([333], dtype=torch.int32, device=dev)
        for s in (105, 7):
            o, d, z = (torch.from_numpy(np.array(a)).to(dev) for a in ps.layout(s))
            n = pc.N // s
            key = '%s/S%d/' % (name, s)
            for v in (0, 1):
                out[key + 'sigma_fwd bf16 sigma_variant %d' % v] = option('sigma_variant', v, lambda: ops.nerf_sigma_fwd(o, d, z, blob['bf16'], 'bf16'))
                out[key + 'sigma_fwd fp32 sigma_x3_variant %d' % v] = option('sigma_x3_variant', v, lambda: ops.nerf_sigma_fwd(o, d, z, blob['fp32'], 'fp32'))
                for p in ('bf16', 'fp32'):
                    nrm, sig = option('sigma_grad_rows', v, lambda: ops.nerf_sigma_grad(o, d, z, blob[p], p))
                    out[key + 'sigma_grad %s sigma_grad_rows %d' % (p, v)] = torch.cat([nrm, sig[..., None]], -1)

                def stride4():
                    rgbs = torch.full((n, s, 4), -12345., device=dev)
                    _capi.check(_capi.lib.nfx_nerf_sigma_refine(ops._ptr(o), ops._ptr(d), ops._ptr(z), n, s, ops._ptr(blob['fp32']), ops._ptr(lst),
                                                                ops._ptr(cnt), ops._ptr(rgbs), ops._stream()), 'nfx_nerf_sigma_refine')
                    return rgbs
                out[key + 'list stride 4 sigma_x3_variant %d' % v] = option('sigma_x3_variant', v, stride4)
                out[key + 'list stride 1 sigma_x3_variant %d' % v] = option('sigma_x3_variant', v, lambda: ops.nerf_sigma_fwd_list(
                    o, d, z, blob['fp32'], lst, cnt, torch.full((n, s), -12345., device=dev), 'fp32'))
                out[key + 'last sample sigma_x3_variant %d' % v] = option('sigma_x3_variant', v, lambda: ops.nerf_refine_last_sample(
                    o, d, z, torch.full((n, s, 4), -12345., device=dev), blob['fp32']))
            # the bf16 list kernel of the occupancy march, for completeness of nfx_nerf_sigma_fwd_list
            out[key + 'list stride 1 bf16'] = ops.nerf_sigma_fwd_list(o, d, z, blob['bf16'], lst, cnt, torch.full((n, s), -12345., device=dev), 'bf16')
    torch.cuda.synchronize()

out = {k: v.detach().cpu().contiguous() for k, v in out.items()}
lib = os.environ.get('NFX_LIB_PATH', 'the tree\'s libnfx.so')
if mode == 'save':
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print('saved %d cases from %s' % (len(out), lib))
    for k, v in out.items():
        print('  %-60s %8d elements  sha1 %s' % (k, v.numel(), hashlib.sha1(v.numpy().tobytes()).hexdigest()[:12]))
else:
    ref = torch.load(path)
    assert sorted(ref) == sorted(out), 'other cases than the saved ones'
    bad = 0
    print('compared %d cases of %s with the saved ones' % (len(out), lib))
    for k, v in out.items():
        a, b = v.numpy().view(np.uint8), ref[k].numpy().view(np.uint8)
        differing = int((v.reshape(-1).view(torch.int32) != ref[k].reshape(-1).view(torch.int32)).sum()) if v.dtype == torch.float32 \
            else (int((a != b).sum()) if a.shape == b.shape else -1)
        bad += differing != 0
        print('  %-60s %8d elements  %d differing' % (k, v.numel(), differing))
    print('ALL BIT-IDENTICAL' if not bad else '%d CASES DIFFER' % bad)
    sys.exit(1 if bad else 0)
