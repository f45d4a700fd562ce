"""The batched weight-gradient GEMMs of csrc/train.hip (wgrad_kernel, wgrad_lds_narrow_kernel, wgrad_lds_kernel with its
device-side row count, wgrad_reduce_kernel) on their own, EXACTLY.

Operands are small integers: exact in bf16, their products and every partial sum exact in fp32 in any order
(|sum| <= 64 * 1040 + 100 < 2^24), so each dW / db must equal an int64 matmul bit for bit — no tolerance.  dW and db start
from random integers (the kernels accumulate), every allocation carries 64 sentinel floats behind it, and everything the
kernels must not read as a number holds bf16 NaN (0xFFFF): the rows at or past `rows` (counted mode: at or past
round16(count)) up to ld, and the odd half of the last feature pair of an odd feature count.  The partial-sum workspace
starts as NaN too.  The call tables are the shipped ones plus an adversarial one; the kernel form and the slab plan are chosen
through the library's options and checked with the plan query.

What the NaN in the odd half of a last pair can and cannot show: as feature F of an F-feature operand it only ever reaches
accumulator row (column) F, which no kernel stores, so a kernel that fails to zero it still passes; a kernel that SELECTS the
wrong half, or reads a pair too many, does not (profiles/wgrad_exact/mutations.txt)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_ROWS = 1040
# every row count any case contracts over: the references are prefix sums of one product per table
BREAKS = (0, 1, 15, 16, 17, 64, 80, 112, 128, 144, 255, 256, 257, 272, 400, 528, 1024, 1025, 1040)
SENTINELS = 64
NAN16 = 0xFFFF


class Table:
    """xs / zs: operand name -> feature count.  dws: dW name -> (rows of the whole dW, n_out).  calls: (x, z, dW, first
    dW row the call writes, with a bias) in launch order."""

    def __init__(self, name, seed, xs, zs, dws, calls):
        self.name, self.seed, self.xs, self.zs, self.dws, self.calls = name, seed, xs, zs, dws, calls
        for dw, (k_total, n_out) in dws.items():      # the calls of one dW tile its rows and share the gradient operand
            mine = sorted((c for c in calls if c[2] == dw), key=lambda c: c[3])
            row = 0
            for x, z, _, row0, _ in mine:
                assert row0 == row and zs[z] == n_out and z == mine[0][1], (name, dw)
                row += xs[x]
            assert row == k_total, (name, dw)

    @property
    def dims(self):
        return [(self.xs[x], self.zs[z]) for x, z, _, _, _ in self.calls]

    def __repr__(self):
        return self.name


def nerf_table():
    """The 14 calls of nfx_nerf_mlp_bwd: kNerfWgradDims and the table that function builds (capi_train.cpp).
    {256,256} and {63,256} of layer 5 share zt and write rows 0..255 / 256..318 of one [319, 256] dW, {27,128} writes behind
    {256,128}; both skip-row calls pass db = null."""
    xs = {'pe': 63, 'pv': 27, 'bott': 256, 'r0': 128}
    xs.update({'a%d' % l: 256 for l in range(8)})
    zs = {'dz%d' % l: 256 for l in range(8)}
    zs.update({'dsig': 1, 'dbott': 256, 'dr0': 128, 'drgb': 3})
    dws = {'k%d' % l: (256, 256) for l in range(1, 8)}
    dws.update({'k0': (63, 256), 'k5': (319, 256), 'k8': (256, 1), 'k9': (256, 256), 'k10': (283, 128), 'k11': (128, 3)})
    calls = [('pe', 'dz0', 'k0', 0, True)]
    calls += [('a%d' % (l - 1), 'dz%d' % l, 'k%d' % l, 0, True) for l in range(1, 8)]
    calls += [('pe', 'dz5', 'k5', 256, False), ('a7', 'dsig', 'k8', 0, True), ('a7', 'dbott', 'k9', 0, True),
              ('bott', 'dr0', 'k10', 0, True), ('pv', 'dr0', 'k10', 256, False), ('r0', 'drgb', 'k11', 0, True)]
    t = Table('nerf14', 11, xs, zs, dws, calls)
    assert t.dims == [(63, 256)] + [(256, 256)] * 7 + [(63, 256), (256, 1), (256, 256), (256, 128), (27, 128), (128, 3)]
    return t


def width128_table(name, seed, ind, out_dim):
    """The six calls of a width-128 backward: mlp128_wgrad_calls and the table nfx_mlp128_bwd builds
    (capi_train.cpp) — ind = 63 | 90, out_dim = 1 .. 8 — and, with ind = z_dim + 15 and out_dim = 1, brdf_rows_wgrad_calls and
    the table nfx_brdf_rows_bwd builds.  The skip rows go behind layer 3's, without a bias."""
    xs = {'x': ind, 'h0': 128, 'h1': 128, 'h2': 128, 'h3': 128}
    zs = {'dz0': 128, 'dz1': 128, 'dz2': 128, 'dz3': 128, 'dzo': out_dim}
    dws = {'k0': (ind, 128), 'k1': (128, 128), 'k2': (128, 128), 'k3': (128 + ind, 128), 'k4': (128, out_dim)}
    calls = [('x', 'dz0', 'k0', 0, True), ('h0', 'dz1', 'k1', 0, True), ('h1', 'dz2', 'k2', 0, True),
             ('h2', 'dz3', 'k3', 0, True), ('x', 'dz3', 'k3', 128, False), ('h3', 'dzo', 'k4', 0, True)]
    t = Table(name, seed, xs, zs, dws, calls)
    assert t.dims == [(ind, 128), (128, 128), (128, 128), (128, 128), (ind, 128), (128, out_dim)]
    return t


def adversarial_table():
    """Exactly kWgMaxCalls = 16 calls at the sizes where a blocked GEMM breaks: one feature, one feature in a second block
    (129 = 128 + 1, 257 = 256 + 1), an odd count in a later block, db = null between two calls with a bias, a shared zt
    writing neighbouring row ranges of one dW, a last call without a bias."""
    shapes = [(1, 1, True), (2, 1, False), (127, 255, True), (129, 257, False), (257, 129, True), (512, 3, True),
              (3, 512, False), (130, 257, True), (33, 257, False), (16, 16, True), (128, 128, False), (255, 1, True),
              (1, 255, False), (64, 130, True), (256, 256, True), (5, 7, False)]
    xs, zs, dws, calls = {}, {}, {}, []
    for i, (k, n, bias) in enumerate(shapes):
        xs['x%d' % i] = k
        if i == 8:      # shares call 7's gradient operand, writes rows 130..162 of call 7's dW
            calls.append(('x8', 'z7', 'w7', 130, bias))
            continue
        zs['z%d' % i] = n
        dws['w%d' % i] = (k + 33 if i == 7 else k, n)
        calls.append(('x%d' % i, 'z%d' % i, 'w%d' % i, 0, bias))
    t = Table('adversarial16', 13, xs, zs, dws, calls)
    assert len(t.calls) == 16 and t.dims == [(k, n) for k, n, _ in shapes]
    return t


NERF = nerf_table()
ADV = adversarial_table()
W128 = [width128_table('w128_in%d_out%d' % (ind, od), 20 + i, ind, od)
        for i, (ind, od) in enumerate([(63, 1), (63, 3), (63, 8), (90, 1), (90, 3), (90, 8)])]
BRDF = width128_table('brdf_rows_z3', 31, 3 + 15, 1)      # z_dim = 3, the shape of tests/test_gpu_brdf_rows.py
NARROW_TABLES = W128 + [BRDF]
WIDE_TABLES = [NERF, ADV]


@functools.lru_cache(maxsize=None)
def operands(table):
    """name -> [MAX_ROWS, F] int64 in [-8, 8], not symmetric in any sense: a transposed or permuted operand cannot pass"""
    rng = np.random.default_rng(table.seed)
    return ({x: rng.integers(-8, 9, size=(MAX_ROWS, f)) for x, f in table.xs.items()},
            {z: rng.integers(-8, 9, size=(MAX_ROWS, f)) for z, f in table.zs.items()})


@functools.lru_cache(maxsize=None)
def reference(table):
    """dW name -> {n: (X_cat[:n].T @ Z[:n], Z[:n].sum(0))} in int64 for every n of BREAKS, X_cat = the inputs of the dW's
    calls side by side (the GEMM over the concatenated inputs).  Computed once per table, as prefix sums."""
    X, Z = operands(table)
    out = {}
    for dw in table.dws:
        mine = sorted((c for c in table.calls if c[2] == dw), key=lambda c: c[3])
        xcat = np.concatenate([X[c[0]] for c in mine], axis=1)
        z = Z[mine[0][1]]
        w, b, at = np.zeros((xcat.shape[1], z.shape[1]), np.int64), np.zeros(z.shape[1], np.int64), {}
        for lo, hi in zip((0,) + BREAKS, BREAKS):
            if hi > lo:
                w = w + np.ascontiguousarray(xcat[lo:hi].T) @ z[lo:hi]
                b = b + z[lo:hi].sum(0)
            at[hi] = (w.astype(np.int32), b)      # (|sum| < 2^17: half the memory; added to int64 below)
        out[dw] = at
    return out


def pair_major(vals, ld, n_data, n_zero_to=None):
    """[rows, F] integers -> the feature-pair-major layout of csrc/feat_store.hpp, [ceil(F / 2)][ld][2] bf16, as int16 bits.
    Rows [0, n_data) hold vals; rows [n_data, n_zero_to) zeros (n_zero_to given); every other row up to ld, and the odd half
    of the last pair of an odd F, bf16 NaN."""
    f = vals.shape[1]
    pairs = (f + 1) // 2
    a = np.full((ld, 2 * pairs), NAN16, np.uint16)
    # a small integer's bf16 is the upper half of its fp32 (at most 4 significant bits)
    a[:n_data, :f] = (vals[:n_data].astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    if n_zero_to is not None:
        a[n_data:n_zero_to, :f] = 0
    return np.ascontiguousarray(a.reshape(ld, pairs, 2).transpose(1, 0, 2)).view(np.int16)


def ld_of(rows):
    """ld = rows for 64, 128 and 256 rows; otherwise past the next multiple of 128 by 4 (ld % 4 is all the loads need)"""
    return rows if rows in (64, 128, 256) else (rows + 127) // 128 * 128 + 4


def run_case(ops, cuda, table, rows, ld, count=None, seed=0, expect_form=None):
    """One batch launch on poisoned operands; asserts every dW / db against the int64 reference, the sentinels, and that the
    plan took the form the case is about.  Returns the plan."""
    X, Z = operands(table)
    plan = ops.selftest_wgrad_plan(table.dims, rows)
    if expect_form is not None:
        assert (plan['use_lds'], plan['wide']) == expect_form, plan
    n = rows if count is None else count
    n16 = (n + 15) // 16 * 16
    if count is None:
        xt = {k: pair_major(v, ld, rows) for k, v in X.items()}
        zt = {k: pair_major(v, ld, rows) for k, v in Z.items()}
    else:   # the producers' contract: [count, round16(count)) holds zeros in zt, finite values in xt
        xt = {k: pair_major(v, ld, n16) for k, v in X.items()}
        zt = {k: pair_major(v, ld, n, n16) for k, v in Z.items()}
    xt = {k: torch.from_numpy(v).to(cuda).view(torch.bfloat16) for k, v in xt.items()}
    zt = {k: torch.from_numpy(v).to(cuda).view(torch.bfloat16) for k, v in zt.items()}
    rng = np.random.default_rng(1000 + seed)
    guard = np.arange(SENTINELS, dtype=np.float32) * 3 + 12345
    dw0, db0, dw, db = {}, {}, {}, {}
    for name, (k_total, n_out) in table.dws.items():
        dw0[name] = rng.integers(-100, 101, size=(k_total, n_out))
        dw[name] = torch.from_numpy(np.concatenate((dw0[name].ravel().astype(np.float32), guard))).to(cuda)
        if any(c[2] == name and c[4] for c in table.calls):
            db0[name] = rng.integers(-100, 101, size=n_out)
            db[name] = torch.from_numpy(np.concatenate((db0[name].astype(np.float32), guard))).to(cuda)
    need = ops.selftest_wgrad_partial_bytes(table.dims, rows)
    partial = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=cuda)       # fp32 NaN throughout
    calls = [(xt[x], zt[z], table.xs[x], table.zs[z], dw[w][row0 * table.dws[w][1]:], db[w] if bias else None)
             for x, z, w, row0, bias in table.calls]
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=cuda)
    ops.selftest_wgrad_batch(calls, ld, rows, partial, count=cnt, partial_bytes=need)
    torch.cuda.synchronize()
    ref = reference(table)
    nonzero = False
    for name, (k_total, n_out) in table.dws.items():
        got = dw[name].cpu().numpy()
        prod, bsum = ref[name][n]
        np.testing.assert_array_equal(got[-SENTINELS:], guard, err_msg='%s: sentinels behind dW %s' % (table, name))
        np.testing.assert_array_equal(got[:-SENTINELS].reshape(k_total, n_out).astype(np.float64),
                                      (prod + dw0[name]).astype(np.float64), err_msg='%s: dW %s' % (table, name))
        nonzero = nonzero or bool(got[:-SENTINELS].any())
        if n > 0 and k_total * n_out >= 64:
            assert (got[:-SENTINELS].reshape(k_total, n_out) != dw0[name]).any(), '%s: dW %s was not written' % (table, name)
        if name in db:
            gotb = db[name].cpu().numpy()
            np.testing.assert_array_equal(gotb[-SENTINELS:], guard, err_msg='%s: sentinels behind db %s' % (table, name))
            np.testing.assert_array_equal(gotb[:-SENTINELS].astype(np.float64), (bsum + db0[name]).astype(np.float64),
                                          err_msg='%s: db %s' % (table, name))
    assert nonzero, '%s: every dW came back all zero' % table
    assert (partial[need:] == 0xFF).all(), 'the partial-sum workspace was written past the size the bytes query gives'
    return plan


def set_options(nfx_opt, **kw):
    for key in ('wgrad_lds', 'wgrad_slabs', 'wgrad_rounds', 'wgrad_narrow'):
        if kw.get(key) is None:
            nfx_opt.unset(key)
        else:
            nfx_opt.set(key, kw[key])


# ------------------------------------------------------------------------------------------------------------ the forms
@pytest.mark.parametrize('table', [NERF, ADV, BRDF] + W128, ids=repr)
@pytest.mark.parametrize('rows,slabs', [(16, None), (128, None), (144, None), (400, None), (400, 3)])
def test_direct_form(nfx_lib, cuda, nfx_opt, table, rows, slabs):
    """wgrad_kernel: one wave per 128 x 128 block and slab.  Default slabs of 128 rows (144 and 400 rows end in a 16-row
    slab); wgrad_slabs = 3 at 400 rows: slabs of 144, 144 and 112 rows."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=0, wgrad_slabs=slabs)
    plan = run_case(ops, cuda, table, rows, ld_of(rows), seed=rows, expect_form=(False, False))
    assert (plan['slab'], plan['n_slabs']) == ((144, 3) if slabs else (128, (rows + 127) // 128))


@pytest.mark.parametrize('table', NARROW_TABLES, ids=repr)
@pytest.mark.parametrize('rows', [16, 112, 128, 144, 256, 272, 528])
def test_narrow_lds_form(nfx_lib, cuda, nfx_opt, table, rows):
    """wgrad_lds_narrow_kernel (every dim <= 128): 128-row chunks split over four waves.  528 rows: three slabs of 256 rows,
    the last of 16 rows; 272: a second slab of 16; 144: a second chunk of 16; 112: a chunk that is not full."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=1)
    plan = run_case(ops, cuda, table, rows, ld_of(rows), seed=rows, expect_form=(True, False))
    assert (plan['slab'], plan['n_slabs']) == (256, (rows + 255) // 256)


@pytest.mark.parametrize('table', WIDE_TABLES, ids=repr)
@pytest.mark.parametrize('variant', ['default', 'slabs4', 'rounds2'])
@pytest.mark.parametrize('rows', [16, 64, 80, 256, 272, 1040])
def test_wide_lds_form(nfx_lib, cuda, nfx_opt, table, rows, variant):
    """wgrad_lds_kernel (a dim > 128): 256 x 256 blocks, 64-row chunks, four waves one quadrant each."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=1, wgrad_slabs=4 if variant == 'slabs4' else None,
                wgrad_rounds=2 if variant == 'rounds2' else None)
    plan = run_case(ops, cuda, table, rows, ld_of(rows), seed=rows, expect_form=(True, True))
    if variant == 'slabs4' and rows == 1040:
        assert (plan['slab'], plan['n_slabs']) == (320, 4)


@pytest.mark.parametrize('table', NARROW_TABLES, ids=repr)
@pytest.mark.parametrize('rows', [144, 528])
def test_wide_lds_form_on_narrow_dims(nfx_lib, cuda, nfx_opt, table, rows):
    """wgrad_narrow = 0: the width-128 tables through the wide kernel (three of its four quadrants hold no feature)."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=1, wgrad_narrow=0)
    run_case(ops, cuda, table, rows, ld_of(rows), seed=rows, expect_form=(True, True))


# ------------------------------------------------------------------------------------------------------ counted mode
@pytest.mark.parametrize('table', WIDE_TABLES, ids=repr)
@pytest.mark.parametrize('slabs', [None, 4])
@pytest.mark.parametrize('count', [0, 1, 15, 16, 17, 255, 256, 257, 1024, 1025, 1040])
def test_wide_lds_form_counted(nfx_lib, cuda, nfx_opt, table, count, slabs):
    """The row count read from device memory: capacity 1040 rows (ld 1280), the rows that count are [0, count).  The slabs
    are re-cut on the device; slabs wholly past the counted rows write zeros.  count = 0: dW and db come back as they went
    in (the reference's prefix sum at 0 is zero: the same assertion)."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=1, wgrad_slabs=slabs)
    run_case(ops, cuda, table, MAX_ROWS, 1280, count=count, seed=count, expect_form=(True, True))


# ------------------------------------------------------------------------------------------------------------ refusals
def _small_batch(cuda, table, rows, ld):
    X, Z = operands(table)
    xt = {k: torch.from_numpy(pair_major(v, ld, rows)).to(cuda).view(torch.bfloat16) for k, v in X.items()}
    zt = {k: torch.from_numpy(pair_major(v, ld, rows)).to(cuda).view(torch.bfloat16) for k, v in Z.items()}
    dw = {w: torch.full((k * n + SENTINELS,), 7., device=cuda) for w, (k, n) in table.dws.items()}
    db = {w: torch.full((n + SENTINELS,), 7., device=cuda) for w, (k, n) in table.dws.items()}
    calls = [(xt[x], zt[z], table.xs[x], table.zs[z], dw[w][row0 * table.dws[w][1]:], db[w] if bias else None)
             for x, z, w, row0, bias in table.calls]
    return calls, dw, db


def _untouched(dw, db):
    torch.cuda.synchronize()
    return all(bool((t == 7.).all()) for t in list(dw.values()) + list(db.values()))


def test_refusals(nfx_lib, cuda, nfx_opt):
    """Every bad argument is an error of the library's own (NFX_EINVAL = -1, NFX_EALIGN = -2) before anything is launched:
    dW and db keep their bits."""
    from nerfactor_amd import ops
    set_options(nfx_opt, wgrad_lds=1)
    rows, ld = 32, 64
    calls, dw, db = _small_batch(cuda, ADV, rows, ld)
    need = ops.selftest_wgrad_partial_bytes(ADV.dims, rows)
    partial = torch.zeros((need + 32,), dtype=torch.uint8, device=cuda)
    count = torch.tensor([16, 16], dtype=torch.int32, device=cuda)
    einval, ealign = r'\(-1\)', r'\(-2\)'

    def refused(match, calls=calls, ld=ld, rows=rows, partial=partial, count=None, partial_bytes=need):
        with pytest.raises(nfx_lib.NfxError, match=match):
            ops.selftest_wgrad_batch(calls, ld, rows, partial, count=count, partial_bytes=partial_bytes)
        assert _untouched(dw, db)

    refused(einval, calls=calls + calls[:1])                  # 17 calls
    refused(einval, rows=24)                                  # not a multiple of 16
    refused(einval, ld=16)                                    # ld < rows
    refused(einval, ld=34)                                    # ld % 4 != 0
    refused(einval, partial_bytes=need - 4)                   # workspace too small
    refused(ealign, partial=partial[8:])                      # partial not 16-byte aligned
    bad = list(calls)
    bad[2] = (calls[2][0].view(-1)[1:],) + calls[2][1:]       # xt 2 bytes off
    refused(ealign, calls=bad)
    bad = list(calls)
    bad[3] = calls[3][:1] + (calls[3][1].view(-1)[4:],) + calls[3][2:]      # zt 8 bytes off
    refused(ealign, calls=bad)
    raw = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    bad = list(calls)
    bad[0] = calls[0][:4] + (raw[2:], calls[0][5])            # dw 2 bytes off (call 0 is 1 x 1)
    refused(ealign, calls=bad)
    bad[0] = calls[0][:5] + (raw[1:],)                        # db 1 byte off
    refused(ealign, calls=bad)
    refused(ealign, count=raw[2:])                            # count 2 bytes off
    assert not bool(raw.any())
    assert ops.selftest_wgrad_partial_bytes(ADV.dims + ADV.dims[:1], rows) == 0
    with pytest.raises(nfx_lib.NfxError, match=einval):
        ops.selftest_wgrad_plan(ADV.dims + ADV.dims[:1], rows)
    # a device-side count is read by the wide LDS form only
    nfx_opt.set('wgrad_lds', 0)
    need0 = ops.selftest_wgrad_partial_bytes(ADV.dims, rows)
    refused(einval, count=count, partial=torch.zeros((need0,), dtype=torch.uint8, device=cuda), partial_bytes=need0)
    nfx_opt.set('wgrad_lds', 1)
    ncalls, ndw, ndb = _small_batch(cuda, BRDF, rows, ld)
    nneed = ops.selftest_wgrad_partial_bytes(BRDF.dims, rows)
    with pytest.raises(nfx_lib.NfxError, match=einval):
        ops.selftest_wgrad_batch(ncalls, ld, rows, torch.zeros((nneed,), dtype=torch.uint8, device=cuda), count=count)
    assert _untouched(ndw, ndb)
    # and the same batch without the count goes through (the refusals above are about the argument, not the batch)
    ops.selftest_wgrad_batch(calls, ld, rows, partial, partial_bytes=need)
    assert not _untouched(dw, db)
