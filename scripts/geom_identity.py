"""Outputs of kernels, saved (first call) or compared bit for bit (later calls): the check for a change of their sources
that must not change a single bit.  One process per library:
    NFX_LIB_PATH=old.so python scripts/geom_identity.py save;  python scripts/geom_identity.py check
    ... save --pack-only / check --pack-only: the packers alone (no GPU)
    ... save --group rows / check --group rows, save --group bwd / check --group bwd: the other groups of cases
--group geom (the default): the density / density-gradient kernels (nerf_geom.hip, nerf_geom_x3.hip, nerf_sigma_x3_pipe.hip)
  and the bytes of the fp32-class packers, on the 840-point sets of tests/nerf_point_cases.py ('glorot', 'fitted'), as
  [8, 105] and [120, 7].
--group rows: the width-128 row kernels behind brdf_row.hpp and mlp128_resident.hpp (lvis_v2.hip, mlp128.hip, mlp128_x3.hip,
  brdf_sphere.hip, brdf_bwd.hip) on the seeded cases of tests/row_mlp_cases.py, tests/test_gpu_brdf_sphere.py and
  tests/bwd_probes.py.
--group bwd: the training backward kernels behind bwd_tile.hpp and mlp128_bwd_ring.hpp (mlp128_bwd.hip, mlp128_bwd_fused.hip,
  nerf_bwd.hip) on the launch shapes of tests/bwd_probes.py, with dense seeded upstream gradients of which about 40 % of the
  rows are exact zeros, under every path and option that selects another kernel.
--group generic (also with --pack-only): the runtime-shaped MLP (mlp_generic.hip, capi_generic.cpp) in its three operand modes:
  the packers' bytes for every shape of tests/generic_exact_cases.py, and forward, dW, db, dx of four of them at 97 and 161 rows."""
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
group = sys.argv[sys.argv.index('--group') + 1] if '--group' in sys.argv else 'geom'
assert group in ('geom', 'rows', 'bwd', 'generic') and not (pack_only and group not in ('geom', 'generic'))
path = os.path.join(ROOT, 'build', 'geom_identity%s%s.pt' % ('' if group == 'geom' else '_' + group, '_pack' if pack_only else ''))     # build/ is not tracked
out = {}


def option(key, value, fn):
    _capi.set_option(key, value)
    try:
        return fn()
    finally:
        _capi.unset_option(key)


def geom_cases():
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


def options(fn, **kw):
    for k, v in kw.items():
        if v is not None:
            _capi.set_option(k, v)
    try:
        return fn()
    finally:
        for k, v in kw.items():
            if v is not None:
                _capi.unset_option(k)


def rows_cases():
    """The width-128 row kernels: learned BRDF in every shipped form (+ brdf_ct 8, + prec fp32), light visibility in every
    variant and the ROWS form, the sphere preview, the BRDF backward (dense and list) and the prior on explicit rows."""
    from tests import bwd_probes as bp, row_mlp_cases as rc, test_gpu_brdf_sphere as ts, test_gpu_row_mlp_fwd as tf
    from tests.test_gpu_bwd_row_probes import buffers
    to_dev = tf.dev
    dev = torch.device('cuda:0')
    for name in rc.SMALL + ['l512']:
        c = rc.case(name)
        d = tf.Dev(c, dev)
        blob = {p: tf.pack(*rc.brdf_net(c.zd), _capi.IN_Z_RUSINK, 1, dev, z_dim=c.zd, prec=p) for p in ('bf16', 'fp32')}
        for variant, ct in tf.brdf_forms() + [(6, 8)]:
            out['brdf/%s variant %d brdf_ct %s' % (name, variant, ct)] = options(lambda: tf.run_brdf(d, blob['bf16']), brdf_variant=variant, brdf_ct=ct)
        out['brdf/%s fp32' % name] = tf.run_brdf(d, blob['fp32'], prec='fp32')
    lblob = tf.pack(*rc.lvis_net(), _capi.IN_XYZ_LDIR, 1, dev)
    for name in rc.LVIS_CASES:
        c = rc.case(name)
        d = tf.Dev(c, dev)
        for variant in tf.LVIS_VARIANTS:
            out['lvis/%s variant %d' % (name, variant)] = options(lambda: tf.run_lvis(d, lblob), lvis_variant=variant)
        rows = torch.from_numpy(np.random.default_rng(5).permutation(2 * c.n + 3)[:c.n].astype(np.int32)).to(dev)
        for variant in (8, 4):
            full = torch.full((2 * c.n + 3, c.L), -7., device=dev)
            options(lambda: ops.lvis_fwd(d.xyz, d.lxyz, lblob, out=full, out_row=rows), lvis_variant=variant, lvis_rows=1)
            out['lvis/%s ROWS variant %d' % (name, variant)] = full
    for spec in ts.CASES[:2]:
        out['sphere/%s' % (spec,)] = ts.Case(_capi, dev, *spec).run()
    for zd in bp.BRDF_SPEC_ZDIMS:
        nl, n = bp.BRDF_SWEEP
        ks, bs = bp.net128(700 + zd, zd + 15, 1)
        tblob = ops.pack_brdf_train_weights(ks, bs, zd).to(dev)
        f = {k: to_dev(v, dev) for k, v in bp.brdf_spec_fill(n, nl, zd).items()}
        rng = np.random.default_rng(710 + zd)
        dspec = to_dev(rng.normal(size=(n, nl)) * (rng.uniform(size=(n, nl)) < .6), dev)      # 40 % of the rows carry no gradient
        for rows_opt in (0, 1):
            dz, dn = options(lambda: ops.brdf_spec_bwd(f['xyz'], f['cam'], f['normal'], f['z'], f['lxyz'], tblob, dspec), brdf_bwd_rows=rows_opt)
            out['brdf_spec_bwd/z_dim %d brdf_bwd_rows %d' % (zd, rows_opt)] = torch.cat([dz, dn], 1)
    ks, bs = bp.net128(bp.BRDF_ROWS_SEED, bp.BRDF_ROWS_ZDIM + 15, 1)
    tblob = ops.pack_brdf_train_weights(ks, bs, bp.BRDF_ROWS_ZDIM).to(dev)
    f = {k: to_dev(v, dev) for k, v in bp.brdf_rows_fill(bp.BRDF_ROWS_N).items()}
    for reci in (False, True):
        out['brdf_rows_fwd/reci %d' % reci] = ops.brdf_rows_fwd(f['z'], f['rusink'], tblob, reci=reci)
        flat, dks, dbs = buffers(ks, bs, dev)
        dout = to_dev(np.random.default_rng(720 + reci).normal(size=(1 + reci) * bp.BRDF_ROWS_N), dev)
        out['brdf_rows_bwd/reci %d d_z' % reci] = ops.brdf_rows_bwd(f['z'], f['rusink'], tblob, dout, dks, dbs, reci=reci)
        out['brdf_rows_bwd/reci %d dW db' % reci] = flat
    torch.cuda.synchronize()


def bwd_cases():
    """The gradient buffer (every dW and db, flat) of the width-128 backward (IN_XYZ: 260 rows, one net per output activation;
    IN_XYZ_LDIR: 32 lights x 9 points; the three-head launch: 260 rows) under fused / fused1 / fused3 / gemm0 / gemm1, the gemm
    paths with the register-staged and the ring kernel, and of the NeRF backward (3 x 87 and 9 x 128 points) with the
    register-staged kernel and the ring kernel at 4 and 8 waves, with and without the row list, behind both GEMM forms."""
    from tests import bwd_probes as bp
    from tests.test_gpu_bwd_row_probes import Ldir, Nerf, Xyz, dev as to_dev
    dev = torch.device('cuda:0')

    def sparse_rows(seed, rows, width):      # dense values; about 40 % of the rows are exact zeros
        rng = np.random.default_rng(seed)
        return to_dev(rng.normal(size=(rows, width)) * (rng.uniform(size=(rows, 1)) < .6), dev)

    paths = [('fused', dict(wgrad_fused=1)), ('fused1', dict(wgrad_fused=1, m128_blocks=1)), ('fused3', dict(wgrad_fused=1, m128_blocks=3))]
    paths += [('gemm%d m128_bwd %d' % (lds, ring), dict(wgrad_fused=0, wgrad_lds=lds, m128_bwd=ring)) for lds in (0, 1) for ring in (0, 1)]
    n = bp.N_SWEEP
    x = to_dev(bp.xyz_fill(n)['xyz'], dev)
    xyz = {name: Xyz(_capi, dev, name) for name in bp.HEAD_NETS}
    douts = {name: sparse_rows(800 + i, n, t.p.out_dim) for i, (name, t) in enumerate(xyz.items())}
    ld = Ldir(_capi, dev)
    nl, npt = bp.LDIR_SWEEP
    lf = {k: to_dev(v, dev) for k, v in bp.ldir_fill(npt, nl).items()}
    ldout = sparse_rows(810, npt * nl, 1).reshape(npt, nl).contiguous()
    for pname, kw in paths:
        for name in bp.SWEEP_NETS:
            out['mlp128_bwd xyz/%s %s' % (name, pname)] = options(lambda: xyz[name].run(x, douts[name]).clone(), **kw)
        out['mlp128_bwd xyz+ldir/%s' % pname] = options(lambda: ld.run(lf['xyz'], lf['xyz_dir'], lf['lxyz'], ldout).clone(), **kw)

        def heads():
            for t in xyz.values():
                t.flat.zero_()
            ops.mlp128_bwd_heads(_capi.IN_XYZ, x, [(douts[name], t.blob, t.dks, t.dbs, t.p.act, t.p.post) for name, t in xyz.items()],
                                 xyz_scale=bp.XYZ_SCALE)
            return torch.cat([t.flat for t in xyz.values()])
        out['mlp128_bwd_heads/%s' % pname] = options(heads, **kw)
    nerf = Nerf(dev)
    forms = [('nerf_bwd 0', dict(nerf_bwd=0))]
    forms += [('nerf_bwd 1 nerf_bwd_nw %d nerf_bwd_rows %d' % (nw, rows), dict(nerf_bwd=1, nerf_bwd_nw=nw, nerf_bwd_rows=rows)) for nw in (4, 8) for rows in (0, 1)]
    for rays, s in (bp.NERF_SWEEP, bp.NERF_PAIR):
        f, _ = nerf.batch(rays, s)
        d = sparse_rows(820 + s, rays * s, 4).reshape(rays, s, 4).contiguous()
        for fname, kw in forms:
            for lds in (0, 1):
                out['nerf_mlp_bwd/%dx%d %s wgrad_lds %d' % (rays, s, fname, lds)] = options(
                    lambda: nerf.run(f['rayo'], f['rayd'], f['z'], d).clone(), wgrad_lds=lds, **kw)
    torch.cuda.synchronize()


def generic_cases():
    """The runtime-shaped MLP (mlp_generic.hip, capi_generic.cpp) in its three operand modes.  The packers' bytes (forward and
    train blob) for every shape of tests/generic_exact_cases.py; on the GPU forward, dW, db and dx, with and without want_dx, of
    four of them on real-valued seeded data (Glorot weights, non-zero biases: no sum is exact by construction), with a sigmoid
    and a softplus output and a sigmoid hidden layer, at 97 rows (four waves per workgroup: one workgroup whose fourth wave has
    a partial tile) and 161 (a second workgroup, two of whose waves have no tile)."""
    from tests import generic_exact_cases as G

    def glorot(name, acts=None):
        c = G.case(name)
        rng = np.random.default_rng(900 + sorted(G.SHAPES).index(name))
        ks = [rng.uniform(-1, 1, size=k.shape).astype(np.float32) * np.float32(np.sqrt(6. / sum(k.shape))) for k, _ in c.layers]
        bs = [rng.normal(size=b.shape).astype(np.float32) * np.float32(.1) for _, b in c.layers]
        return c, rng, ks, bs, acts or c.acts

    for name in sorted(G.SHAPES):
        c, _, ks, bs, acts = glorot(name)
        for prec in G.PRECS:
            for train in (False, True):
                out['pack%s/%s %s' % ('_train' if train else '', name, prec)] = ops.GenericNet(ks, bs, acts, c.skip_at or None, train=train, prec=prec).blob
    if pack_only:
        return
    dev = torch.device('cuda:0')
    for name, acts in (('w128x3_skip1', ['relu'] * 3 + ['sigmoid']), ('two_skips', ['relu', 'relu', 'softplus']),
                       ('in283', ['sigmoid', None]), ('wide320', None)):
        c, rng, ks, bs, acts = glorot(name, acts)
        x_all = rng.normal(size=(161, c.d_in)).astype(np.float32)
        dy_all = rng.normal(size=(161, c.widths[-1])).astype(np.float32)
        for prec in G.PRECS:
            net = ops.GenericNet(ks, bs, acts, c.skip_at or None, train=True, prec=prec).to(dev)
            for n in (97, 161):
                x, dy = torch.from_numpy(x_all[:n]).to(dev), torch.from_numpy(dy_all[:n]).to(dev)
                key = 'generic/%s %s n %d ' % (name, prec, n)
                out[key + 'y'] = ops.mlp_generic_fwd(x, net)
                for want_dx in (False, True):
                    flat = [torch.full(k.shape, .5, device=dev) for k in ks] + [torch.full(b.shape, -.25, device=dev) for b in bs]      # (the kernels ADD)
                    dx = ops.mlp_generic_bwd(x, net, dy, flat[:len(ks)], flat[len(ks):], want_dx=want_dx)
                    out[key + 'dW db want_dx %d' % want_dx] = torch.cat([t.reshape(-1) for t in flat])
                    if want_dx:
                        out[key + 'dx'] = dx
                out[key + 'dx alone'] = ops.mlp_generic_bwd(x, net, dy, None, None, want_dx=True)
    torch.cuda.synchronize()


{'geom': geom_cases, 'rows': rows_cases, 'bwd': bwd_cases, 'generic': generic_cases}[group]()

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
