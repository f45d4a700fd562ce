"""The MLP backward kernels (csrc/mlp128_bwd.hip, mlp128_bwd_fused.hip, nerf_bwd.hip, brdf_bwd.hip) one row at a time, bit
for bit.  Inputs, constants and float64 oracles: tests/bwd_probes.py (its docstring has the argument).

A.  Position and isolation, no tolerance.  The upstream gradient is non-zero in ONE row r, which holds a probe input; every
    other row holds random finite inputs.  Every gradient tensor (one flat buffer of all dW / db) must EQUAL, value for
    value, the launch G* that holds the probe alone (n = 1), for every r of the batch and every launch shape: all lanes,
    waves, tiles, tails, workgroups and list slots run the same arithmetic, no row reads anything of another row, none is
    dropped or counted twice, and the reductions over waves, workgroups and slabs lose nothing.
B.  G* against float64 autograd of the same-rounding network, per tensor, at the bounds tests/test_gpu_train.py states for the
    whole batch (2.5e-2 width-128, 3e-2 NeRF and the learned BRDF) — now a bound on one row's path.  The worst measured
    distance per op is printed (profiles/bwd_row_probes/errors.txt).
C.  A one-row dW is outer(bf16 input, bf16 dZ) and db the same bf16 dZ (the fused kernel takes db0 / db3 from a 1.0 in the
    encoding's pad slot, the GEMM path sums the very dZ operand, train.hip), so dW[i, j] / db[j] must be the oracle's bf16
    encoding of the probe, element for element: layer 0 and the skip rows, for NeRF the view rows of rgb_out[0] as well.

The entry points build bf16 only (prec = fp32 is refused with NFX_ENOSUP), so there is no fp32 sweep.  nfx_brdf_spec_bwd takes
light counts that are multiples of 32: its reference launch is one point with 32 lights, the probe at light 0.
Out of reach of one-hot probes: a defect that needs two rows with a gradient in one MFMA block (the two-probe NeRF case and
the batch tests of tests/test_gpu_train.py stand there) and summation over many rows (tests/test_gpu_wgrad_exact.py)."""
import numpy as np
import pytest
import torch

from tests import bwd_probes as bp

pytestmark = pytest.mark.gpu

P = bp.N_PROBES
TOL_128, TOL_NERF, TOL_BRDF = 2.5e-2, 3e-2, bp.TOL_BRDF


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def buffers(ks, bs, cuda):
    """one flat fp32 buffer and the dW / db views into it"""
    sizes = [int(np.prod(a.shape)) for a in list(ks) + list(bs)]
    flat = torch.zeros(sum(sizes), device=cuda)
    views, at = [], 0
    for a, s in zip(list(ks) + list(bs), sizes):
        views.append(flat[at:at + s].view(a.shape))
        at += s
    return flat, views[:len(ks)], views[len(ks):]


def split(flat, ks, bs):
    out, at = [], 0
    for a in list(ks) + list(bs):
        s = int(np.prod(a.shape))
        out.append(flat[at:at + s].view(a.shape).double().cpu())
        at += s
    return out


def report(op, errs, tol):
    """errs: per probe, the per-tensor relative Frobenius distances of the one-row launch from float64.  Prints the worst
    tensor of every probe, then asserts every tensor of every probe."""
    worst = [max(e) for e in errs]
    print("bwd_row_probes: %-34s bound %.1e  worst tensor per probe: %s  worst %.3e  median %.3e"
          % (op, tol, ' '.join('%.2e' % w for w in worst), max(worst), float(np.median(worst))))
    assert all(w < tol for w in worst), (op, errs)


def check_gstar(gstar):
    for k, g in enumerate(gstar):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, 'probe %d: the reference launch is empty' % k


def set_path(nfx_opt, path):
    """the names of test_lvis_backward_vs_autograd: fused[N] = on-chip weight gradients (N persistent workgroups), gemm0 / gemm1 =
    stored activations and the direct / LDS weight-gradient GEMMs"""
    if path.startswith('fused'):
        nfx_opt.set('wgrad_fused', 1)
        if path[5:]:
            nfx_opt.set('m128_blocks', int(path[5:]))
        else:
            nfx_opt.unset('m128_blocks')
    else:
        nfx_opt.set('wgrad_fused', 0)
        nfx_opt.set('wgrad_lds', path[-1])
        nfx_opt.unset('m128_blocks')


def distances(got, want):
    return [bp.rel_frobenius(g, w) for g, w in zip(got, want)]


def recovered(dw_rows, db, enc, what):
    bad, cols = bp.input_recovery(dw_rows, db, bp.bf16(enc))
    assert cols > 0 and bad == 0, '%s: dW / db differs from the bf16 encoding in %d places (%d columns)' % (what, bad, cols)


# ------------------------------------------------------------------------------------------------ width-128, IN_XYZ
class Xyz:
    def __init__(self, nfx_lib, cuda, name):
        from nerfactor_amd import ops
        self.ops, self.kind, self.cuda, self.p = ops, nfx_lib.IN_XYZ, cuda, bp.xyz_probes(name)
        p = self.p
        self.blob = ops.pack_mlp128_train_weights(p.ks, p.bs, self.kind, p.out_dim).to(cuda)
        self.flat, self.dks, self.dbs = buffers(p.ks, p.bs, cuda)
        self.x, self.g = dev(p.inputs['xyz'], cuda), dev(p.g, cuda)

    def run(self, xyz, dout):
        self.flat.zero_()
        self.ops.mlp128_bwd(self.kind, xyz, dout, self.blob, self.dks, self.dbs, out_act=self.p.act, xyz_scale=bp.XYZ_SCALE,
                            post_scale=self.p.post)
        return self.flat

    def gstar(self):
        g = [self.run(self.x[k:k + 1].contiguous(), self.g[k:k + 1].contiguous()).clone() for k in range(P)]
        check_gstar(g)
        return g

    def sweep(self, n, rows, gstar):
        """-> the rows at which the gradients are not G*"""
        x = dev(bp.xyz_fill(n)['xyz'], self.cuda)
        dout = torch.zeros(n, self.p.out_dim, device=self.cuda)
        bad = []
        for r in rows:
            k = r % P
            keep = x[r].clone()
            x[r], dout[r] = self.x[k], self.g[k]
            if not torch.equal(self.run(x, dout), gstar[k]):
                bad.append(r)
            x[r], dout[r] = keep, 0.
        return bad


@pytest.mark.parametrize('path', ['fused', 'fused1', 'fused3', 'gemm0', 'gemm1'])
@pytest.mark.parametrize('net', bp.SWEEP_NETS)
def test_xyz_every_row_of_two_tiles_and_a_tail(nfx_lib, cuda, nfx_opt, net, path):
    """n = 260: two full 128-row tiles and a 4-row tail, EVERY row position.  fused: one workgroup per tile; fused1: one workgroup
    walks all three tiles and the weight ring wraps; fused3; gemm0 / gemm1: activations stored, both GEMM forms."""
    set_path(nfx_opt, path)
    t = Xyz(nfx_lib, cuda, net)
    bad = t.sweep(bp.N_SWEEP, bp.sweep_rows(bp.N_SWEEP), t.gstar())
    assert not bad, '%s %s: gradients differ from the one-row launch with the probe at rows %s' % (net, path, bad)


@pytest.mark.parametrize('net', bp.SWEEP_NETS)
def test_xyz_first_and_last_row_around_one_tile(nfx_lib, cuda, nfx_opt, net):
    set_path(nfx_opt, 'fused')
    t = Xyz(nfx_lib, cuda, net)
    gstar = t.gstar()
    for n in bp.N_EDGES:
        bad = t.sweep(n, bp.edge_rows(n), gstar)
        assert not bad, (net, n, bad)


@pytest.mark.parametrize('path', ['fused', 'gemm0', 'gemm1'])
@pytest.mark.parametrize('net', bp.SWEEP_NETS)
def test_xyz_one_row_vs_float64(nfx_lib, cuda, nfx_opt, net, path):
    set_path(nfx_opt, path)
    t = Xyz(nfx_lib, cuda, net)
    p, errs = t.p, []
    for k, g in enumerate(t.gstar()):
        got = split(g, p.ks, p.bs)
        errs.append(distances(got, bp.mlp128_oracle(p, k)))
        recovered(got[0], got[5], p.enc[k], '%s %s probe %d layer 0' % (net, path, k))
        recovered(got[3][128:], got[8], p.enc[k], '%s %s probe %d skip rows' % (net, path, k))
    report('mlp128_bwd xyz %s %s' % (net, path), errs, TOL_128)


def test_heads_of_one_launch_each_equal_their_own_row(nfx_lib, cuda, nfx_opt):
    """ops.mlp128_bwd_heads: three networks over the same rows in one launch pair, each head's probe at a row of its own (its
    gradient is zero at the other heads' rows).  Each head must equal its own one-row nfx_mlp128_bwd launch."""
    from nerfactor_amd import ops
    set_path(nfx_opt, 'fused')
    heads = [Xyz(nfx_lib, cuda, name) for name in bp.HEAD_NETS]
    gstars = [t.gstar() for t in heads]
    n = bp.N_SWEEP
    x = dev(bp.xyz_fill(n, seed=7)['xyz'], cuda)
    douts = [torch.zeros(n, t.p.out_dim, device=cuda) for t in heads]
    args = [(d, t.blob, t.dks, t.dbs, t.p.act, t.p.post) for d, t in zip(douts, heads)]
    bad = []
    for r in range(n):
        rows = [(r + 87 * h) % n for h in range(len(heads))]        # three different rows, in different tiles
        k = r % P
        keep = x[rows].clone()
        for t, d, row in zip(heads, douts, rows):
            x[row], d[row] = t.x[k], t.g[k]
            t.flat.zero_()
        ops.mlp128_bwd_heads(nfx_lib.IN_XYZ, x, args, xyz_scale=bp.XYZ_SCALE)
        bad += [(r, h) for h, t in enumerate(heads) if not torch.equal(t.flat, gstars[h][k])]
        for d, row in zip(douts, rows):
            d[row] = 0.
        x[rows] = keep
    assert not bad, 'heads differ from their one-row launches at (first head row, head) %s' % bad


# ------------------------------------------------------------------------------------------- width-128, IN_XYZ_LDIR
class Ldir:
    def __init__(self, nfx_lib, cuda):
        from nerfactor_amd import ops
        self.ops, self.kind, self.cuda, self.p = ops, nfx_lib.IN_XYZ_LDIR, cuda, bp.ldir_probes()
        p = self.p
        self.blob = ops.pack_mlp128_train_weights(p.ks, p.bs, self.kind, 1).to(cuda)
        self.flat, self.dks, self.dbs = buffers(p.ks, p.bs, cuda)
        self.inp = {k: dev(v, cuda) for k, v in p.inputs.items()}
        self.g = dev(p.g, cuda)

    def run(self, xyz, xyz_dir, lxyz, dout):
        self.flat.zero_()
        self.ops.mlp128_bwd(self.kind, xyz, dout, self.blob, self.dks, self.dbs, out_act='sigmoid', lxyz=lxyz, xyz_dir=xyz_dir)
        return self.flat

    def gstar(self):
        i = self.inp
        g = [self.run(*(i[name][k:k + 1].contiguous() for name in ('xyz', 'xyz_dir', 'lxyz')), self.g[k:k + 1].contiguous()).clone()
             for k in range(P)]
        check_gstar(g)
        return g

    def sweep(self, nl, n, pairs, gstar):
        """pairs: (point, light) of the probe row"""
        f = {k: dev(v, self.cuda) for k, v in bp.ldir_fill(n, nl).items()}
        dout = torch.zeros(n, nl, device=self.cuda)
        bad = []
        for j, (pt, l) in enumerate(pairs):
            k = j % P
            keep = [f['xyz'][pt].clone(), f['xyz_dir'][pt].clone(), f['lxyz'][l].clone()]
            f['xyz'][pt], f['xyz_dir'][pt], f['lxyz'][l] = self.inp['xyz'][k], self.inp['xyz_dir'][k], self.inp['lxyz'][k]
            dout[pt, l] = self.g[k, 0]
            if not torch.equal(self.run(f['xyz'], f['xyz_dir'], f['lxyz'], dout), gstar[k]):
                bad.append((pt, l))
            f['xyz'][pt], f['xyz_dir'][pt], f['lxyz'][l] = keep
            dout[pt, l] = 0.
        return bad


@pytest.mark.parametrize('path', ['fused', 'fused3', 'gemm0', 'gemm1'])
def test_ldir_every_point_light_row(nfx_lib, cuda, nfx_opt, path):
    """32 lights x 9 points = 288 rows: a 128-row tile spans four points, the last point's lights are a 32-row tail."""
    set_path(nfx_opt, path)
    t = Ldir(nfx_lib, cuda)
    nl, n = bp.LDIR_SWEEP
    bad = t.sweep(nl, n, [(r // nl, r % nl) for r in range(n * nl)], t.gstar())
    assert not bad, '%s: gradients differ from the one-row launch with the probe at (point, light) %s' % (path, bad)


@pytest.mark.parametrize('path', ['fused', 'fused3', 'gemm0', 'gemm1'])
def test_ldir_lights_of_a_point_straddle_tiles(nfx_lib, cuda, nfx_opt, path):
    """512 lights x 2 points: lights 0, 127, 128 and 511 of the first point, 0 and 511 of the second."""
    set_path(nfx_opt, path)
    t = Ldir(nfx_lib, cuda)
    nl, n = bp.LDIR_WIDE
    bad = t.sweep(nl, n, bp.ldir_wide_rows(nl), t.gstar())
    assert not bad, (path, bad)


@pytest.mark.parametrize('path', ['fused', 'gemm0', 'gemm1'])
def test_ldir_one_row_vs_float64(nfx_lib, cuda, nfx_opt, path):
    set_path(nfx_opt, path)
    t = Ldir(nfx_lib, cuda)
    p, errs = t.p, []
    for k, g in enumerate(t.gstar()):
        got = split(g, p.ks, p.bs)
        errs.append(distances(got, bp.mlp128_oracle(p, k)))
        recovered(got[0], got[5], p.enc[k], '%s probe %d layer 0' % (path, k))
        recovered(got[3][128:], got[8], p.enc[k], '%s probe %d skip rows' % (path, k))
    report('mlp128_bwd xyz+ldir %s' % path, errs, TOL_128)


# ------------------------------------------------------------------------------------------------------------- NeRF
class Nerf:
    def __init__(self, cuda):
        from nerfactor_amd import ops
        self.ops, self.cuda, self.p = ops, cuda, bp.nerf_probes()
        p = self.p
        self.blob = ops.pack_nerf_train_weights(p.ks, p.bs).to(cuda)
        self.flat, self.dks, self.dbs = buffers(p.ks, p.bs, cuda)
        self.inp = {k: dev(v, cuda) for k, v in p.inputs.items()}
        self.g = {kind: dev(g, cuda) for kind, g in p.g_kinds.items()}

    def run(self, rayo, rayd, z, d):
        self.flat.zero_()
        self.ws, self.shape = self.ops.nerf_mlp_bwd(rayo, rayd, z, d, self.blob, self.dks, self.dbs), tuple(z.shape)
        return self.flat

    def listed_count(self, nfx_lib):
        """the length of the device-built list of the last launch (the first word of the list, at the end of the workspace)"""
        rays, s = self.shape
        total = nfx_lib.lib.nfx_nerf_bwd_workspace_bytes(rays, s) // 4
        return int(self.ws.view(torch.int32)[total - self.ops.nerf_bwd_list_words(rays * s)[3]])

    def gstar(self, kind='full'):
        i = self.inp
        g = [self.run(i['rayo'][k:k + 1].contiguous(), i['rayd'][k:k + 1].contiguous(), i['z'][k:k + 1].reshape(1, 1).contiguous(),
                      self.g[kind][k].reshape(1, 1, 4).contiguous()).clone() for k in range(P)]
        check_gstar(g)
        return g

    def batch(self, rays, s):
        f = {k: dev(v, self.cuda) for k, v in bp.nerf_fill(rays, s).items()}
        return f, torch.zeros(rays, s, 4, device=self.cuda)

    def place(self, f, d, m, k, kind='full'):
        """probe k at point m; -> what to hand to restore()"""
        ray, s = divmod(m, d.shape[1])
        keep = (ray, s, f['rayo'][ray].clone(), f['rayd'][ray].clone(), f['z'][ray, s].clone())
        f['rayo'][ray], f['rayd'][ray], f['z'][ray, s] = self.inp['rayo'][k], self.inp['rayd'][k], self.inp['z'][k]
        d[ray, s] = self.g[kind][k]
        return keep

    @staticmethod
    def restore(f, d, keep):
        ray, s, o, dd, zz = keep
        f['rayo'][ray], f['rayd'][ray], f['z'][ray, s] = o, dd, zz
        d[ray, s] = 0.

    def sweep(self, rays, s, points, gstar, kind='full'):
        f, d = self.batch(rays, s)
        bad = []
        for m in points:
            keep = self.place(f, d, m, m % P, kind)
            if not torch.equal(self.run(f['rayo'], f['rayd'], f['z'], d), gstar[m % P]):
                bad.append(m)
            self.restore(f, d, keep)
        return bad


def set_nerf(nfx_opt, listed, variant):
    """lds0 / lds1: the direct / LDS weight-gradient GEMMs behind the default 8-wave kernel; nw4: the 4-wave kernel (LDS GEMMs).
    The direct GEMM form reads no device-side row count, so under lds0 the library differentiates every point whatever
    nerf_bwd_rows says (capi_train.cpp: nfx_wgrad_counted_ok); under lds1 and nw4 the list is built and used."""
    nfx_opt.set('nerf_bwd_rows', listed)
    if variant == 'nw4':
        nfx_opt.set('nerf_bwd_nw', 4)
    nfx_opt.set('wgrad_lds', 0 if variant == 'lds0' else 1)


@pytest.mark.parametrize('variant', ['lds0', 'lds1', 'nw4'])
@pytest.mark.parametrize('listed', [0, 1])
def test_nerf_every_point(nfx_lib, cuda, nfx_opt, listed, variant):
    """3 rays x 87 samples = 261 points: a 256-point tile and a tail (nw4: two 128-point tiles and a tail), tile edges inside a
    ray.  listed = 0: every point is differentiated; 1: the device builds a one-entry list."""
    set_nerf(nfx_opt, listed, variant)
    t = Nerf(cuda)
    rays, s = bp.NERF_SWEEP
    bad = t.sweep(rays, s, bp.sweep_rows(rays * s), t.gstar())
    assert not bad, 'listed=%d %s: gradients differ from the one-point launch with the probe at points %s' % (listed, variant, bad)
    if listed and variant != 'lds0':
        assert t.listed_count(nfx_lib) == 1       # the sweep did run on a one-entry list


def _tensor_views(flat, p):
    out, at = [], 0
    for a in list(p.ks) + list(p.bs):
        s = int(np.prod(a.shape))
        out.append(flat[at:at + s].view(a.shape))
        at += s
    return out


@pytest.mark.parametrize('listed', [0, 1])
@pytest.mark.parametrize('kind', ['density', 'colour'])
def test_nerf_partial_gradients_leave_exact_zeros(nfx_lib, cuda, nfx_opt, kind, listed):
    """A gradient in the density alone leaves the bottleneck's, both colour layers' and their biases' gradients exactly zero; one
    in the three colours alone leaves sigma_out's exactly zero; in both, a unit the oracle masks has an exactly zero db entry
    and an exactly zero dW column.  And the one-row launch is met at both sides of every tile edge."""
    set_nerf(nfx_opt, listed, 'lds1')
    t = Nerf(cuda)
    p = t.p
    gstar = t.gstar(kind)
    for k, g in enumerate(gstar):
        v = _tensor_views(g, p)
        dk, db = v[:12], v[12:]
        for layer in ((9, 10, 11) if kind == 'density' else (8,)):
            assert not bool(dk[layer].any()) and not bool(db[layer].any()), (kind, k, layer)
        for pre, layer in zip(p.pre, bp.NERF_RELU_LAYERS):
            if kind == 'density' and layer == 10:
                continue
            masked = (pre[k] <= 0).to(cuda)
            assert bool(masked.any()) and not bool(db[layer][masked].any()) and not bool(dk[layer][:, masked].any()), (kind, k, layer)
            assert bool(db[layer][~masked].any()), (kind, k, layer)
    rays, s = bp.NERF_SWEEP
    rows = sorted(set(bp.tile_edge_rows(rays * s, bp.TILE_ROWS)) | set(bp.tile_edge_rows(rays * s, bp.NERF_TILE_ROWS)))
    bad = t.sweep(rays, s, rows, gstar, kind)
    assert not bad, (kind, listed, bad)


def test_nerf_two_probes_on_either_side_of_a_list_block_edge(nfx_lib, cuda, nfx_opt):
    """9 rays x 128 samples, gradients at points 1023 and 1024 (the device counts the list per 1024 points): the gradients are
    the sum of the two one-probe launches to fp32 summation — 2e-5 of the largest entry, the figure
    test_nerf_mlp_backward_over_the_points_with_a_gradient uses — and each one-probe launch is its one-point launch."""
    set_nerf(nfx_opt, 1, 'lds1')
    t = Nerf(cuda)
    gstar = t.gstar()
    rays, s = bp.NERF_PAIR
    f, d = t.batch(rays, s)
    edge = bp.LIST_BLOCK
    singles = []
    for m, k in ((edge - 1, 0), (edge, 1)):
        keep = t.place(f, d, m, k)
        singles.append(t.run(f['rayo'], f['rayd'], f['z'], d).clone())
        assert torch.equal(singles[-1], gstar[k]), m
        t.restore(f, d, keep)
    t.place(f, d, edge - 1, 0)
    t.place(f, d, edge, 1)
    both = t.run(f['rayo'], f['rayd'], f['z'], d)
    want = singles[0] + singles[1]
    scale = float(want.abs().max())
    assert t.listed_count(nfx_lib) == 2
    assert scale > 0 and float((both - want).abs().max()) <= 2e-5 * scale, float((both - want).abs().max()) / scale


@pytest.mark.parametrize('wgrad_lds', [0, 1])
def test_nerf_one_point_vs_float64(nfx_lib, cuda, nfx_opt, wgrad_lds):
    nfx_opt.set('wgrad_lds', wgrad_lds)
    t = Nerf(cuda)
    p, errs = t.p, []
    for k, g in enumerate(t.gstar()):
        got = split(g, p.ks, p.bs)
        errs.append(distances(got, bp.nerf_oracle(p, k)))
        recovered(got[0], got[12], p.pe_x[k], 'probe %d layer 0' % k)
        recovered(got[5][256:], got[12 + 5], p.pe_x[k], 'probe %d skip rows' % k)
        recovered(got[10][256:], got[12 + 10], p.pe_v[k], 'probe %d view rows' % k)
    report('nerf_mlp_bwd wgrad_lds=%d' % wgrad_lds, errs, TOL_NERF)


# ---------------------------------------------------------------------------------- learned BRDF inside the shading path
class Spec:
    def __init__(self, cuda, zd):
        from nerfactor_amd import ops
        self.ops, self.cuda, self.p, self.zd = ops, cuda, bp.brdf_spec_probes(zd), zd
        self.blob = ops.pack_brdf_train_weights(self.p.ks, self.p.bs, zd).to(cuda)
        self.inp = {k: dev(v, cuda) for k, v in self.p.inputs.items()}
        self.g = dev(self.p.g, cuda)

    def run(self, f, dspec):
        return self.ops.brdf_spec_bwd(f['xyz'], f['cam'], f['normal'], f['z'], f['lxyz'], self.blob, dspec)

    def fill(self, n, nl):
        return {k: dev(v, self.cuda) for k, v in bp.brdf_spec_fill(n, nl, self.zd).items()}

    def place(self, f, pt, l, k):
        for name in ('xyz', 'cam', 'normal', 'z'):
            f[name][pt] = self.inp[name][k]
        f['lxyz'][l] = self.inp['lxyz'][k]

    def gstar(self):
        """one point, 32 lights (the smallest count the entry point takes), the probe at light 0"""
        out = []
        for k in range(P):
            f = self.fill(1, bp.BRDF_LIGHT_MULTIPLE)
            self.place(f, 0, 0, k)
            dspec = torch.zeros(1, bp.BRDF_LIGHT_MULTIPLE, device=self.cuda)
            dspec[0, 0] = self.g[k, 0]
            dz, dn = self.run(f, dspec)
            out.append(torch.cat((dz[0], dn[0])).clone())
        check_gstar(out)
        return out


@pytest.mark.parametrize('listed', [0, 1])
@pytest.mark.parametrize('zd', bp.BRDF_SPEC_ZDIMS)
def test_brdf_spec_every_front_lit_row(nfx_lib, cuda, nfx_opt, zd, listed):
    """32 lights x 9 points, the probe (a front-lit pair with n . l > 1e-2) at every (point, light): d_z and d_normal of the
    probe's point are the reference launch's, every other point's exactly zero — the kernel sums in fixed point from the first
    addition on, so neither the lane, the wave nor the list slot of the row may show."""
    nfx_opt.set('brdf_bwd_rows', listed)
    t = Spec(cuda, zd)
    gstar = t.gstar()
    nl, n = bp.BRDF_SWEEP
    base = t.fill(n, nl)
    dspec = torch.zeros(n, nl, device=cuda)
    bad = []
    for r in range(n * nl):
        pt, l = divmod(r, nl)
        k = r % P
        f = {name: v.clone() for name, v in base.items()}
        t.place(f, pt, l, k)
        dspec[pt, l] = t.g[k, 0]
        dz, dn = t.run(f, dspec)
        want = torch.zeros(n, zd + 3, device=cuda)
        want[pt] = gstar[k]
        if not torch.equal(torch.cat((dz, dn), 1), want):
            bad.append((pt, l))
        dspec[pt, l] = 0.
    assert not bad, 'z_dim %d listed=%d: d_z / d_normal differ with the probe at (point, light) %s' % (zd, listed, bad)


@pytest.mark.parametrize('zd', bp.BRDF_SPEC_ZDIMS)
def test_brdf_spec_one_row_vs_float64(nfx_lib, cuda, nfx_opt, zd):
    """d_z and d_normal are projections of the input gradient, not outer products: the probes of this op also keep the
    oracle's own floor (dZ rounded per layer or not) under a 3.5th of the bound — bwd_probes.brdf_spec_probes has the rows the
    first draw gave, on which the kernel reproduced the oracle pair's 3e-2 .. 5e-2 to three digits."""
    t = Spec(cuda, zd)
    errs = []
    for k, g in enumerate(t.gstar()):
        dz, dn = bp.brdf_spec_oracle(t.p, k)
        g = g.double().cpu()
        errs.append(distances([g[:zd], g[zd:]], [dz, dn]))
    report('brdf_spec_bwd z_dim=%d' % zd, errs, TOL_BRDF)


# ------------------------------------------------------------------------------------------- the prior on explicit rows
class Rows:
    def __init__(self, cuda):
        from nerfactor_amd import ops
        self.ops, self.cuda, self.p = ops, cuda, bp.brdf_rows_probes()
        p = self.p
        self.blob = ops.pack_brdf_train_weights(p.ks, p.bs, bp.BRDF_ROWS_ZDIM).to(cuda)
        self.flat, self.dks, self.dbs = buffers(p.ks, p.bs, cuda)
        self.z, self.rus, self.g = dev(p.inputs['z'], cuda), dev(p.inputs['rusink'], cuda), dev(p.g, cuda)
        self.rus_reci = dev(bp.reciprocal(p.inputs['rusink']), cuda)

    def run(self, z, rus, dout, reci):
        self.flat.zero_()
        d_z = self.ops.brdf_rows_bwd(z, rus, self.blob, dout, self.dks, self.dbs, reci=reci)
        return self.flat, d_z

    def gstar(self, reci_half):
        """probe k alone, without a reciprocal half: as it is, or (reci_half) with phi_d + pi already added in fp32"""
        rus = self.rus_reci if reci_half else self.rus
        out = []
        for k in range(P):
            flat, d_z = self.run(self.z[k:k + 1].contiguous(), rus[k:k + 1].contiguous(), self.g[k].contiguous(), False)
            out.append((flat.clone(), d_z[0].clone()))
        check_gstar([g for g, _ in out])
        return out


@pytest.mark.parametrize('reci', [True, False])
def test_brdf_rows_every_row(nfx_lib, cuda, nfx_opt, reci):
    """ops.brdf_rows_bwd (the prior's training op), z_dim 3, n = 130: 130 rows, or 260 with the reciprocal half (row n + i =
    the inputs of row i at phi_d + pi).  Weight gradients as above; the per-row d_z is the reference launch's in the probe row
    and exactly zero elsewhere."""
    t = Rows(cuda)
    n = bp.BRDF_ROWS_N
    rows = 2 * n if reci else n
    gstar = [t.gstar(False), t.gstar(True)]
    f = bp.brdf_rows_fill(n)
    z, rus = dev(f['z'], cuda), dev(f['rusink'], cuda)
    dout = torch.zeros(rows, device=cuda)
    bad = []
    for r in range(rows):
        i, half, k = r % n, r // n, r % P
        keep = z[i].clone(), rus[i].clone()
        z[i], rus[i] = t.z[k], t.rus[k]
        dout[r] = t.g[k, 0]
        flat, d_z = t.run(z, rus, dout, reci)
        want_dz = torch.zeros(rows, bp.BRDF_ROWS_ZDIM, device=cuda)
        want_dz[r] = gstar[half][k][1]
        if not (torch.equal(flat, gstar[half][k][0]) and torch.equal(d_z, want_dz)):
            bad.append(r)
        z[i], rus[i] = keep
        dout[r] = 0.
    assert not bad, 'reci=%s: gradients differ from the one-row launch with the probe at rows %s' % (reci, bad)


def test_brdf_rows_one_row_vs_float64(nfx_lib, cuda, nfx_opt):
    t = Rows(cuda)
    p, errs = t.p, []
    for half in (False, True):
        for k, (g, d_z) in enumerate(t.gstar(half)):
            got = split(g, p.ks, p.bs)
            want, want_dz = bp.brdf_rows_oracle(p, k, half)
            errs.append(distances(got + [d_z.double().cpu()], want + [want_dz]))
            enc = (p.enc_reci if half else p.enc)[k]
            recovered(got[0], got[5], enc, 'half %d probe %d layer 0' % (half, k))
            recovered(got[3][128:], got[8], enc, 'half %d probe %d skip rows' % (half, k))
    report('brdf_rows_bwd z_dim=%d' % bp.BRDF_ROWS_ZDIM, errs, TOL_BRDF)
