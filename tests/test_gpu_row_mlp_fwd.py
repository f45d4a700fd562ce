"""The forward width-128 row kernels, pinned to their rows bit for bit.

Kernels: mlp128_xyz_kernel, lvis_pre_kernel, lvis_kernel, brdf_spec_kernel (mlp128.hip); resident128_kernel with 2 / 3 / 4
column tiles x 4 waves and 2 x 8, light visibility, learned BRDF and the ROWS instantiation, brdf_compact_kernel (lvis_v2.hip);
mlp128_x3_kernel in its three input kinds (mlp128_x3.hip).  Inputs: tests/row_mlp_cases.py, whose conditions
tests/test_cpu_row_mlp_cases.py holds without a GPU.

(A) A row's value is a function of its own point and light: a column of an MFMA block does not depend on its neighbours and
every shipped form runs the same arithmetic in the same order.  So the output of a batch must equal, bit for bit, the launch
of each point alone (chunks that cut inside a tile for the larger cases), of its prefixes (n * L around every tile size, n
around the number of waves of the grid), of the points and of the lights in another order, on 1 and 3 workgroups, and in
every other form; back-lit rows are exact zeros whatever the output buffer held before.
(B) The batch against the oracle at the bounds the suite already has (tests/test_gpu_nerfactor.py), on every row: the designed
front-lit counts need no `stable` mask.  (A) cannot see a defect that is the same at every position; (B) holds those.

Lines that start with ROWERR carry the measured worst errors (profiles/row_mlp_fwd/errors.txt)."""
import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import common, row_mlp_cases as rc
from tests.test_gpu_nerfactor import dev, pack
from tests.test_gpu_poisoned_buffers import fresh_memory_holds

pytestmark = pytest.mark.gpu

GRIDS = (None, 1, 3)                      # m128_blocks: the default (256), one workgroup, three
LVIS_VARIANTS = (0, 2, 3, 4, 8)
FP32_TOL = 5e-5                           # test_width128_fp32_class_paths_vs_fp64_oracle
_FIELDS = ('xyz', 'xyz_dir', 'cam', 'normal', 'z')


class Dev:
    """a case's tensors on the device"""

    def __init__(self, c, cuda):
        self.c, self.n = c, c.n
        for k in _FIELDS:
            setattr(self, k, dev(getattr(c, k), cuda))
        self.lxyz = dev(c.lxyz, cuda)

    def sub(self, idx):
        d = object.__new__(Dev)
        d.c, d.lxyz = self.c, self.lxyz
        for k in _FIELDS:
            setattr(d, k, getattr(self, k)[idx].contiguous())
        d.n = d.xyz.shape[0]
        return d


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def on_dev(c, cuda):
    return cached(('dev', c.name), lambda: Dev(c, cuda))


def brdf_blob(nfx_lib, cuda, zd, prec='bf16'):
    return cached(('brdf', zd, prec), lambda: pack(*rc.brdf_net(zd), nfx_lib.IN_Z_RUSINK, 1, cuda, z_dim=zd, prec=prec))


def lvis_blob(nfx_lib, cuda, prec='bf16'):
    return cached(('lvis', prec), lambda: pack(*rc.lvis_net(), nfx_lib.IN_XYZ_LDIR, 1, cuda, prec=prec))


def xyz_blob(nfx_lib, cuda, out_dim, prec='bf16'):
    return cached(('xyz', out_dim, prec), lambda: pack(*rc.xyz_net(out_dim), nfx_lib.IN_XYZ, out_dim, cuda, prec=prec))


def oracle(key, make):
    """computed once, shared by the tests that need it, never written to"""
    v = cached(('oracle',) + key, make)
    v.setflags(write=False)
    return v


def options(nfx_opt, **kw):
    for k, v in kw.items():
        if v is None:
            nfx_opt.unset(k)
        else:
            nfx_opt.set(k, v)


def run_brdf(d, blob, lxyz=None, prec='bf16'):
    from nerfactor_amd import ops
    return ops.brdf_spec_fwd(d.xyz, d.cam, d.normal, d.z, d.lxyz if lxyz is None else lxyz, blob, prec=prec)


def run_lvis(d, blob, lxyz=None, prec='bf16', other_dir=False):
    from nerfactor_amd import ops
    return ops.lvis_fwd(d.xyz, d.lxyz if lxyz is None else lxyz, blob, xyz_scale=1., xyz_dir=d.xyz_dir if other_dir else None, prec=prec)


def perms(n, seed):
    """an order-reversing and a random permutation"""
    return [np.arange(n)[::-1].copy(), np.random.default_rng(seed).permutation(n)]


def parts_of(c):
    return [(i, i + 1) for i in range(c.n)] if c.n <= 40 else rc.chunks(c)


def check_parts_and_orders(run, d, base, what):
    """one point alone (chunks for the larger cases), the points in another order, the lights in another order"""
    c, cuda = d.c, base.device
    for a, b in parts_of(c):
        common.assert_same_bits(base[a:b], run(d.sub(slice(a, b)), None), '%s: points [%d, %d) alone against the batch' % (what, a, b))
    for i, perm in enumerate(perms(c.n, 3)):
        if c.n > 1:
            idx = torch.from_numpy(perm).to(cuda)
            common.assert_same_bits(base[idx], run(d.sub(idx), None), '%s: points in order %d against the batch' % (what, i))
    for i, perm in enumerate(perms(c.L, 4)):
        idx = torch.from_numpy(perm).to(cuda)
        common.assert_same_bits(base[:, idx], run(d, d.lxyz[idx].contiguous()), '%s: lights in order %d against the batch' % (what, i))


def check_prefixes(run, d, base, what, ks=None):
    for k in rc.prefixes(d.c) if ks is None else ks:
        common.assert_same_bits(base[:k], run(d.sub(slice(0, k)), None), '%s: the first %d points against the batch' % (what, k))


def brdf_forms():
    """(brdf_variant, brdf_ct) of every shipped form; brdf_ct 8 stays out (opt-in)"""
    return [(v, None) for v in (0, 2, 3, 4)] + [(5, ct) for ct in rc.COMPACT_CTS] + [(6, ct) for ct in rc.COMPACT_CTS]


# ======================================================================================================= learned BRDF
@pytest.mark.parametrize('name', rc.CASE_NAMES)
def test_brdf_rows_against_the_oracle_and_exact_zeros(nfx_lib, cuda, nfx_opt, name):
    """(B) the default form (6), the same-arithmetic compaction (5), the dense (3) and the streamed (0) kernel against the
    oracle at the bounds of test_brdf_spec_vs_oracle, on EVERY row; back-lit rows exactly 0.0 and front-lit rows > 0 with the
    output buffer pre-filled with 0xFF (NaN) and with 0x00: a point without a front-lit light is a row of written zeros."""
    c = rc.case(name)
    d, blob = on_dev(c, cuda), brdf_blob(nfx_lib, cuda, c.zd)
    want = oracle(('brdf', name), c.brdf)
    want_q = oracle(('brdf_q', name), lambda: c.brdf(quant=nerf_ref.bf16_round))
    front = c.local_lz() > 0
    assert np.array_equal((front).sum(1), c.front_count)
    scale = max(1., want.max())
    for variant in (6, 5, 3, 0):
        options(nfx_opt, brdf_variant=variant)
        outs = []
        for byte in (0xFF, 0x00):
            with fresh_memory_holds(byte) as px:
                outs.append(run_brdf(d, blob))
                torch.cuda.synchronize()
            assert px.filled >= 1
        common.assert_same_bits(outs[0], outs[1], 'brdf %s variant %d: fresh memory 0xFF against 0x00' % (name, variant))
        got = outs[0].cpu().numpy()
        assert got.shape == want.shape and np.isfinite(got).all()
        eq, e = np.abs(got - want_q).max(), np.abs(got - want).max()
        print('ROWERR brdf %-10s variant %d  vs same-rounding oracle %.3e (bound %.3e)  vs fp32 oracle %.3e (bound %.3e)' % (
            name, variant, eq, 6e-3 * scale, e, 3e-2 * scale))
        assert np.all(got[~front] == 0) and np.all(got[front] > 0), (name, variant)
        assert not np.signbit(got[~front]).any()
        assert eq < 6e-3 * scale, (name, variant, eq)
        assert e < 3e-2 * scale, (name, variant, e)


@pytest.mark.parametrize('name', rc.CASE_NAMES)
def test_brdf_forms_and_grids_are_bit_identical(nfx_lib, cuda, nfx_opt, name):
    """(A) forms and grids: streamed, resident 2 / 3 / 4 and compaction 5 with 2 / 3 / 4 column tiles against each other; 6 with
    2 / 3 / 4 against each other; each on the default grid, one workgroup and three; 6 against 5 as
    test_row_mlp_kernel_variants_are_bit_identical does (same zero pattern, 2e-2 max(1, max))."""
    c = rc.case(name)
    d, blob = on_dev(c, cuda), brdf_blob(nfx_lib, cuda, c.zd)
    base = {}
    for variant, ct in brdf_forms():
        for blocks in GRIDS:
            options(nfx_opt, brdf_variant=variant, brdf_ct=ct, m128_blocks=blocks)
            got = run_brdf(d, blob)
            ref = base.setdefault(variant == 6, got)
            common.assert_same_bits(ref, got, 'brdf %s: variant %d, brdf_ct %s, m128_blocks %s against the first form' % (name, variant, ct, blocks))
    same, closed = base[False], base[True]
    assert torch.equal(same > 0, closed > 0)
    assert (same - closed).abs().max().item() < 2e-2 * max(1., same.max().item())


@pytest.mark.parametrize('name', rc.CASE_NAMES)
def test_brdf_rows_do_not_depend_on_their_neighbours(nfx_lib, cuda, nfx_opt, name):
    """(A) one point alone, prefixes, point and light permutations: the default compaction form, the same-arithmetic one with
    three column tiles, two column tiles, the dense and the streamed kernel; prefixes on every grid."""
    c = rc.case(name)
    d, blob = on_dev(c, cuda), brdf_blob(nfx_lib, cuda, c.zd)
    run = lambda dd, lx: run_brdf(dd, blob, lx)
    for variant, ct in [(6, 4), (5, 3), (6, 2), (3, None), (0, None)]:
        options(nfx_opt, brdf_variant=variant, brdf_ct=ct, m128_blocks=None)
        base = run(d, None)
        what = 'brdf %s variant %d ct %s' % (name, variant, ct)
        check_parts_and_orders(run, d, base, what)
        for blocks in GRIDS:
            options(nfx_opt, m128_blocks=blocks)
            check_prefixes(run, d, base, '%s m128_blocks %s' % (what, blocks))


# =================================================================================================== light visibility
@pytest.mark.parametrize('other_dir', [False, True])
@pytest.mark.parametrize('name', rc.LVIS_CASES)
def test_lvis_rows_against_the_oracle(nfx_lib, cuda, nfx_opt, name, other_dir):
    """(B) the default form (8) and the streamed kernel (0) at the bounds of test_lvis_vs_oracle; with the light directions
    taken from other points than the ones the MLP sees (xyz_dir)."""
    c = rc.case(name)
    d, blob = on_dev(c, cuda), lvis_blob(nfx_lib, cuda)
    want = oracle(('lvis', name, other_dir), lambda: c.lvis(other_dir=other_dir))
    want_q = oracle(('lvis_q', name, other_dir), lambda: c.lvis(quant=nerf_ref.bf16_round, other_dir=other_dir))
    for variant in (8, 0):
        options(nfx_opt, lvis_variant=variant)
        got = run_lvis(d, blob, other_dir=other_dir).cpu().numpy()
        assert got.shape == (c.n, c.L) and np.all((got >= 0) & (got <= 1))
        eq, e = np.abs(got - want_q).max(), np.abs(got - want).max()
        print('ROWERR lvis %-10s variant %d xyz_dir %d  vs same-rounding oracle %.3e (bound 1e-2)  vs fp32 oracle %.3e (bound 3e-2)' % (
            name, variant, other_dir, eq, e))
        assert e < 3e-2 and eq < 1e-2, (name, variant, e, eq)


@pytest.mark.parametrize('name', rc.LVIS_CASES)
def test_lvis_forms_grids_and_rows_do_not_depend_on_their_neighbours(nfx_lib, cuda, nfx_opt, name):
    """(A) variants 0, 2, 3, 4, 8 on the default grid, one workgroup and three against each other (with 1 and 3 one workgroup
    walks many tiles and the prefetch runs ahead across points); for each variant one point alone, the point and light
    orders; prefixes on every grid for the default, the streamed and the three-column-tile form."""
    c = rc.case(name)
    d, blob = on_dev(c, cuda), lvis_blob(nfx_lib, cuda)
    base = None
    for other_dir in (False, True):
        run = lambda dd, lx: run_lvis(dd, blob, lx, other_dir=other_dir)
        base = None
        for variant in LVIS_VARIANTS if not other_dir else (8, 0):
            for blocks in GRIDS:
                options(nfx_opt, lvis_variant=variant, m128_blocks=blocks)
                got = run(d, None)
                base = got if base is None else base
                common.assert_same_bits(base, got, 'lvis %s: variant %d, m128_blocks %s, xyz_dir %d against the first form' % (name, variant, blocks, other_dir))
                if variant in (8, 0, 3):
                    check_prefixes(run, d, base, 'lvis %s variant %d m128_blocks %s' % (name, variant, blocks))
            options(nfx_opt, m128_blocks=None)
            check_parts_and_orders(run, d, base, 'lvis %s variant %d xyz_dir %d' % (name, variant, other_dir))


@pytest.mark.parametrize('variant', [8, 4])
@pytest.mark.parametrize('name', rc.LVIS_CASES)
def test_lvis_rows_mode_on_the_new_shapes_and_grids(nfx_lib, cuda, nfx_opt, name, variant):
    """lvis_fwd(out=, out_row=) under lvis_rows 1 (resident128_kernel<., 0, ., true>): the named rows equal the compact launch,
    every other row of a -7-filled buffer is untouched, on every grid and for prefixes that end inside a tile."""
    from nerfactor_amd import ops
    c = rc.case(name)
    d, blob = on_dev(c, cuda), lvis_blob(nfx_lib, cuda)
    options(nfx_opt, lvis_variant=variant, lvis_rows=1)
    assert ops.lvis_rows_supported()
    compact = run_lvis(d, blob)
    n_all = 2 * c.n + 3
    rows = np.random.default_rng(5).permutation(n_all)[:c.n].astype(np.int32)     # not sorted: any row order
    for blocks in GRIDS:
        options(nfx_opt, m128_blocks=blocks)
        for k in sorted(set([c.n] + rc.prefixes(c)[-3:])):
            dd = d.sub(slice(0, k))
            out_row = torch.from_numpy(rows[:k].copy()).to(cuda)
            full = torch.full((n_all, c.L), -7., device=cuda)
            flag = torch.zeros(1, dtype=torch.int32, device=cuda)
            got = ops.lvis_fwd(dd.xyz, dd.lxyz, blob, out=full, out_row=out_row, nan_flag=flag)
            assert got is full and int(flag.item()) == 0
            common.assert_same_bits(compact[:k], full[out_row.long()], 'lvis rows mode %s variant %d m128_blocks %s, %d points' % (name, variant, blocks, k))
            others = torch.ones(n_all, dtype=torch.bool, device=cuda)
            others[out_row.long()] = False
            assert bool((full[others] == -7.).all())


@pytest.mark.parametrize('variant', [8, 0])
def test_lvis_pre_at_every_point_count(nfx_lib, cuda, nfx_opt, variant):
    """lvis_pre_kernel at n = 1, 255, 256, 257, 1031 (5 tiles through one weight ring on one workgroup): 1031 points x 32 lights
    against the oracle, every prefix and every grid bit-equal to the batch."""
    c = rc.pre_case()
    d, blob = on_dev(c, cuda), lvis_blob(nfx_lib, cuda)
    options(nfx_opt, lvis_variant=variant)
    base = run_lvis(d, blob)
    got = base.cpu().numpy()
    want = oracle(('lvis', 'pre'), c.lvis)
    want_q = oracle(('lvis_q', 'pre'), lambda: c.lvis(quant=nerf_ref.bf16_round))
    eq, e = np.abs(got - want_q).max(), np.abs(got - want).max()
    print('ROWERR lvis %-10s variant %d xyz_dir 0  vs same-rounding oracle %.3e (bound 1e-2)  vs fp32 oracle %.3e (bound 3e-2)' % ('pre', variant, eq, e))
    assert e < 3e-2 and eq < 1e-2
    run = lambda dd, lx: run_lvis(dd, blob, lx)
    for blocks in GRIDS:
        options(nfx_opt, m128_blocks=blocks)
        check_prefixes(run, d, base, 'lvis pre variant %d m128_blocks %s' % (variant, blocks), ks=rc.XYZ_N)


# ====================================================================================================== xyz head kernel
def _xyz_sample():
    return sorted(set(range(0, 1031, 97)) | {1, 31, 32, 254, 255, 256, 257, 511, 512, 1023, 1024, 1030})


@pytest.mark.parametrize('head', rc.XYZ_HEADS, ids=lambda h: 'o%d_%s_%g_%g' % h)
def test_mlp128_xyz_rows(nfx_lib, cuda, nfx_opt, head):
    """mlp128_xyz_kernel with out_dim 1, 3, 4, 5, 8 (the upper lane half stores rows 4 .. 7), with and without activation, scale
    and bias: (B) 1031 points against the oracle at the bounds of test_mlp128_xyz_vs_oracle; (A) n = 1, 255, 256, 257 as prefixes,
    one workgroup (5 tiles through one weight ring) and three, single points, the points in another order; every element
    written, whatever the output buffer held."""
    from nerfactor_amd import ops
    out_dim, act, scale, bias = head
    blob = xyz_blob(nfx_lib, cuda, out_dim)
    x = cached('xyz_points', lambda: dev(rc.xyz_points(), cuda))
    run = lambda xx: ops.mlp128_xyz_fwd(xx, blob, out_dim, out_act=act, xyz_scale=rc.XYZ_SCALE, post_scale=scale, post_bias=bias)
    outs = []
    for byte in (0xFF, 0x00):
        with fresh_memory_holds(byte) as px:
            outs.append(run(x))
            torch.cuda.synchronize()
        assert px.filled >= 1
    base = outs[0]
    common.assert_same_bits(base, outs[1], 'mlp128_xyz %s: fresh memory 0xFF against 0x00' % (head,))
    got = base.cpu().numpy()
    want = oracle(('xyz', head), lambda: rc.xyz_head(head))
    want_q = oracle(('xyz_q', head), lambda: rc.xyz_head(head, quant=nerf_ref.bf16_round))
    assert got.shape == (1031, out_dim) and np.isfinite(got).all()
    eq, e = np.abs(got - want_q).max(), np.abs(got - want).max()
    print('ROWERR xyz  %-24s vs same-rounding oracle %.3e (bound 4e-3)  vs fp32 oracle %.3e (bound 3e-2)' % (head, eq, e))
    assert eq < 4e-3 and e < 3e-2, (head, eq, e)
    for blocks in GRIDS:
        options(nfx_opt, m128_blocks=blocks)
        for n in rc.XYZ_N:
            common.assert_same_bits(base[:n], run(x[:n].contiguous()), 'mlp128_xyz %s m128_blocks %s: the first %d points against the batch' % (head, blocks, n))
    options(nfx_opt, m128_blocks=None)
    for i in _xyz_sample():
        common.assert_same_bits(base[i:i + 1], run(x[i:i + 1].contiguous()), 'mlp128_xyz %s: point %d alone against the batch' % (head, i))
    for k, perm in enumerate(perms(1031, 6)):
        idx = torch.from_numpy(perm).to(cuda)
        common.assert_same_bits(base[idx], run(x[idx].contiguous()), 'mlp128_xyz %s: points in order %d against the batch' % (head, k))


# ===================================================================================================== fp32-class path
@pytest.mark.parametrize('name', rc.FP32_CASES)
def test_fp32_class_row_kernels(nfx_lib, cuda, nfx_opt, name):
    """mlp128_x3_kernel, (point, light) kinds, prec = 'fp32': the same one-point, permutation, prefix and grid identities, and the
    float64 oracle at the bounds of test_width128_fp32_class_paths_vs_fp64_oracle (FP32_TOL; learned BRDF: 0.99 quantile at FP32_TOL,
    every row at 4 FP32_TOL, times max(1, max))."""
    c = rc.case(name)
    d = on_dev(c, cuda)
    front = c.local_lz(np.float64) > 0
    for kind in ('lvis', 'lvis_dir', 'brdf'):
        if kind == 'brdf':
            blob = brdf_blob(nfx_lib, cuda, c.zd, 'fp32')
            run = lambda dd, lx: run_brdf(dd, blob, lx, prec='fp32')
            want = oracle(('brdf64', name), lambda: c.brdf(dtype=np.float64))
        else:
            blob = lvis_blob(nfx_lib, cuda, 'fp32')
            other = kind == 'lvis_dir'
            run = lambda dd, lx: run_lvis(dd, blob, lx, prec='fp32', other_dir=other)
            want = oracle(('lvis64', name, other), lambda: c.lvis(dtype=np.float64, other_dir=other))
        options(nfx_opt, m128_blocks=None)
        base = run(d, None)
        got = base.cpu().numpy()
        err = np.abs(got - want)
        print('ROWERR fp32 %-8s %-10s max %.3e  0.99 quantile %.3e (FP32_TOL %.0e)' % (kind, name, err.max(), np.quantile(err, .99), FP32_TOL))
        assert got.shape == want.shape and np.isfinite(got).all()
        if kind == 'brdf':
            scale = max(1., want.max())
            assert np.all(got[~front] == 0) and np.all(got[front] > 0)
            assert np.quantile(err, .99) < FP32_TOL * scale and err.max() < 4 * FP32_TOL * scale, (kind, name, err.max())
        else:
            assert err.max() < FP32_TOL, (kind, name, err.max())
        what = 'fp32-class %s %s' % (kind, name)
        check_parts_and_orders(run, d, base, what)
        for blocks in GRIDS:
            options(nfx_opt, m128_blocks=blocks)
            common.assert_same_bits(base, run(d, None), '%s: m128_blocks %s against the default grid' % (what, blocks))
            check_prefixes(run, d, base, '%s m128_blocks %s' % (what, blocks))


@pytest.mark.parametrize('head', [rc.XYZ_HEADS[3], rc.XYZ_HEADS[4]], ids=lambda h: 'o%d_%s_%g_%g' % h)
def test_fp32_class_xyz_rows(nfx_lib, cuda, nfx_opt, head):
    """mlp128_x3_kernel, xyz kind, out_dim 5 and 8: float64 oracle at FP32_TOL max(1, max |want|) and at least 50 x closer than the bf16
    kernel (as test_width128_fp32_class_paths_vs_fp64_oracle at n >= 300); prefixes, grids, single points, point order."""
    from nerfactor_amd import ops
    out_dim, act, scale, bias = head
    blob, blob16 = xyz_blob(nfx_lib, cuda, out_dim, 'fp32'), xyz_blob(nfx_lib, cuda, out_dim)
    x = cached('xyz_points', lambda: dev(rc.xyz_points(), cuda))
    run = lambda xx, prec='fp32': ops.mlp128_xyz_fwd(xx, blob if prec == 'fp32' else blob16, out_dim, out_act=act, xyz_scale=rc.XYZ_SCALE,
                                                    post_scale=scale, post_bias=bias, prec=prec)
    base = run(x)
    want = oracle(('xyz64', head), lambda: rc.xyz_head(head, dtype=np.float64))
    err, err16 = np.abs(base.cpu().numpy() - want).max(), np.abs(run(x, 'bf16').cpu().numpy() - want).max()
    print('ROWERR fp32 xyz %-24s max %.3e (bound %.3e), bf16 kernel %.3e' % (head, err, FP32_TOL * max(1., np.abs(want).max()), err16))
    assert err < FP32_TOL * max(1., np.abs(want).max()) and err < 0.02 * err16, (err, err16)
    for blocks in GRIDS:
        options(nfx_opt, m128_blocks=blocks)
        for n in rc.XYZ_N:
            common.assert_same_bits(base[:n], run(x[:n].contiguous()), 'fp32-class xyz %s m128_blocks %s: the first %d points against the batch' % (head, blocks, n))
    options(nfx_opt, m128_blocks=None)
    for i in _xyz_sample():
        common.assert_same_bits(base[i:i + 1], run(x[i:i + 1].contiguous()), 'fp32-class xyz %s: point %d alone against the batch' % (head, i))
    for k, perm in enumerate(perms(1031, 6)):
        idx = torch.from_numpy(perm).to(cuda)
        common.assert_same_bits(base[idx], run(x[idx].contiguous()), 'fp32-class xyz %s: points in order %d against the batch' % (head, k))
