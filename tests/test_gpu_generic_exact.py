"""The runtime-shaped MLP kernels (csrc/mlp_generic.hip: forward, backward, weight gradients and their reduction) with NO
tolerance, in all three operand modes.

Part 1 (integer networks, tests/generic_exact_cases.py): forward, dW, db and dx equal an int64 reference bit for bit at every
row count, under both fill bytes of freshly allocated memory, through the strided / column-offset forms of every argument,
under every launch option (nerf_blocks, wgrad_splits, wgrad_map), and the train / re-packed blobs equal the forward / host
ones.  The conditions that make equality the right demand are proved on the CPU (tests/test_cpu_generic_exact_cases.py).
Part 2 (real-valued data, sigmoid and softplus included): what must hold without a reference — a row's y and dx are functions
of that row alone, and a dy that is non-zero in one row gives the dW / db of that row launched alone under every split and
map (every other row contributes exact zeros, so no reduction order can show)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import generic_exact_cases as G
from tests.test_gpu_poisoned_buffers import fresh_memory_holds

pytestmark = pytest.mark.gpu

NAMES = sorted(G.SHAPES)
FILLS = (0x00, 0xFF)
_NETS = {}


def f32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def int_net(name, prec, cuda, train):
    from nerfactor_amd import ops
    key = (name, prec, train)
    if key not in _NETS:
        c = G.case(name)
        _NETS[key] = ops.GenericNet([k.astype(np.float32) for k, _ in c.layers], [b.astype(np.float32) for _, b in c.layers],
                                    c.acts, c.skip_at or None, train=train, prec=prec).to(cuda)
    return _NETS[key]


def same(got, want, what):
    """bit for bit: `want` is an integer array, `got` the fp32 tensor the kernel left"""
    got = got.detach().cpu().numpy()
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    first = [(tuple(int(v) for v in i), float(want[tuple(i)]), float(got[tuple(i)])) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ from the integer reference; rows %s; first (index, want, got) %s" % (
        what, len(bad), got.size, sorted({int(i[0]) for i in bad})[:10], first))


def keeps_fill(t, byte, what):
    assert bool((t.contiguous().view(torch.uint8) == byte).all()), '%s was written' % what


def bwd_strided(net, x, dy_wide, col0_dy, dks, dbs, dx_buf):
    """nfx_mlp_generic_bwd with every leading dimension of the C-ABI in use: dy read from columns [col0_dy, ...) of a wider
    matrix, dx written into the first d_in columns of a wider one.  The workspace is allocated as ops.mlp_generic_bwd
    allocates it (through ops.torch, i.e. through the fill of fresh_memory_holds)."""
    from nerfactor_amd import ops
    lib, n = ops.lib, x.shape[0]
    nbytes = lib.nfx_mlp_generic_bwd_workspace_bytes(n, net.d_in, net.n_layers, net._w, net._s, net.prec)
    ws = ops.torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    karr = (ctypes.c_void_p * net.n_layers)(*[t.data_ptr() for t in dks]) if dks else None
    barr = (ctypes.c_void_p * net.n_layers)(*[t.data_ptr() for t in dbs]) if dbs else None
    ops.check(lib.nfx_mlp_generic_bwd(ops._ptr(x), n, x.stride(0), net.d_in, net.n_layers, net._w, net._a, net._s,
                                      ops._ptr(net.blob), net.prec, ops._ptr(dy_wide), dy_wide.stride(0), col0_dy,
                                      ops._ptr(dx_buf) if dx_buf is not None else None, dx_buf.stride(0) if dx_buf is not None else net.d_in,
                                      karr, barr, ops._ptr(ws), ws.numel(), ops._stream()), 'nfx_mlp_generic_bwd')


def start_buffers(c, cuda):
    return [f32(a, cuda) for a in c.dw0], [f32(a, cuda) for a in c.db0]


def check_forward(name, prec, cuda, n, fill, what):
    from nerfactor_amd import ops
    c, r = G.case(name), G.reference(name, prec)
    net = int_net(name, prec, cuda, False)
    x = f32(c.x[:n], cuda)
    with fresh_memory_holds(fill) as px:
        y = ops.mlp_generic_fwd(x, net)
        assert px.filled == 1
        same(y, r.y[:n], '%s y' % what)
        # into columns [4, 4 + d_out) of a wider matrix, from a strided x whose other columns are NaN
        wide = ops.torch.empty((n, c.widths[-1] + 7), dtype=torch.float32, device=cuda)
        xs = torch.full((n, c.d_in + 3), float('nan'), device=cuda)
        xs[:, :c.d_in] = x
        ops.mlp_generic_fwd(xs[:, :c.d_in], net, out=wide, col0=4)
        same(wide[:, 4:4 + c.widths[-1]], r.y[:n], '%s y through out= / col0=' % what)
        keeps_fill(wide[:, :4], fill, '%s: columns in front of col0' % what)
        keeps_fill(wide[:, 4 + c.widths[-1]:], fill, '%s: columns behind the output' % what)


def check_backward(name, prec, cuda, n, fill, what, modes=True):
    from nerfactor_amd import ops
    c, r = G.case(name), G.reference(name, prec)
    net = int_net(name, prec, cuda, True)
    want_dw, want_db = G.weight_grads(name, prec, n)
    x = f32(c.x[:n], cuda)
    dyw = torch.full((n, c.widths[-1] + 5), float('nan'), device=cuda)
    dyw[:, 3:3 + c.widths[-1]] = f32(c.dy[:n], cuda)
    with fresh_memory_holds(fill):
        dks, dbs = start_buffers(c, cuda)
        dxb = ops.torch.empty((n, c.d_in + 6), dtype=torch.float32, device=cuda)
        bwd_strided(net, x, dyw, 3, dks, dbs, dxb)
        for i in range(len(dks)):
            same(dks[i], want_dw[i], '%s dW[%d]' % (what, i))
            same(dbs[i], want_db[i], '%s db[%d]' % (what, i))
        same(dxb[:, :c.d_in], r.dx[:n], '%s dx' % what)
        keeps_fill(dxb[:, c.d_in:], fill, '%s: the padding of dx' % what)
        if not modes:
            return
        dy = f32(c.dy[:n], cuda)
        dks2, dbs2 = start_buffers(c, cuda)
        assert ops.mlp_generic_bwd(x, net, dy, dks2, dbs2) is None                 # no input gradient wanted
        for i in range(len(dks)):
            same(dks2[i], want_dw[i], '%s dW[%d], want_dx = False' % (what, i))
            same(dbs2[i], want_db[i], '%s db[%d], want_dx = False' % (what, i))
        same(ops.mlp_generic_bwd(x, net, dy, None, None, want_dx=True), r.dx[:n], '%s dx, input gradient only' % what)


# ------------------------------------------------------------------------------------------- part 1: integer networks
@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_forward_is_the_integer_reference(nfx_lib, cuda, name, prec):
    for n in G.ROWS:
        for fill in FILLS:
            check_forward(name, prec, cuda, n, fill, '%s %s n=%d fill=%#x NW,WIDE=%s' % (name, prec, n, fill, G.instantiation(name, prec, n)))


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_backward_is_the_integer_reference(nfx_lib, cuda, name, prec):
    for n in G.ROWS:
        for fill in FILLS:
            check_backward(name, prec, cuda, n, fill, '%s %s n=%d fill=%#x NW,WIDE=%s' % (name, prec, n, fill, G.instantiation(name, prec, n)),
                           modes=fill == 0xFF)


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_launch_options_change_nothing(nfx_lib, nfx_opt, cuda, name, prec):
    """nerf_blocks 1 / 3: 8 / 24 waves in all, so the workgroups of a 289- / 1299-row launch walk a second row tile and the
    weight ring wraps onto it.  wgrad_splits 1 / 3 / default (10 uneven splits of 41 row tiles) x wgrad_map 0 / 1."""
    for blocks in (1, 3):
        nfx_opt.set('nerf_blocks', blocks)
        for n in (289, G.N_MAX):
            what = '%s %s n=%d nerf_blocks=%d' % (name, prec, n, blocks)
            check_forward(name, prec, cuda, n, 0xFF, what)
            check_backward(name, prec, cuda, n, 0xFF, what, modes=False)
    nfx_opt.unset('nerf_blocks')
    for splits in (1, 3, None):
        nfx_opt.unset('wgrad_splits') if splits is None else nfx_opt.set('wgrad_splits', splits)
        for wmap in (0, 1):
            nfx_opt.set('wgrad_map', wmap)
            for n in (129, G.N_MAX):
                check_backward(name, prec, cuda, n, 0xFF, '%s %s n=%d wgrad_splits=%s wgrad_map=%d' % (name, prec, n, splits, wmap), modes=False)


def test_every_instantiation_ran():
    """which <M, NW, WIDE> each launch above runs is a function of the case (generic_exact_cases.instantiation, pinned to the
    source on the CPU): all of them occur"""
    ran = {(prec,) + G.instantiation(name, prec, n) for name in NAMES for prec in G.PRECS for n in G.ROWS}
    assert ran == {('bf16', 1, False), ('bf16', 1, True), ('fp32', 1, False), ('fp32', 2, False), ('fp32', 4, False), ('fp32', 1, True),
                   ('fp32_native', 1, False), ('fp32_native', 2, False), ('fp32_native', 4, False), ('fp32_native', 1, True)}


def real_net(name, rng):
    """the shapes with the activations of tests/test_gpu_generic.py (sigmoid and softplus back in), glorot weights"""
    c = G.case(name)
    acts = {'w256x8_skip4': ['relu'] * 8 + ['sigmoid'], 'two_skips': ['relu', 'softplus', None], 'in539': ['relu', 'sigmoid'],
            'w128x3_skip1': ['relu'] * 3 + ['sigmoid']}.get(name, c.acts)
    ks = [nerf_ref.glorot_uniform(rng, k.shape[0], k.shape[1]) for k, _ in c.layers]
    bs = [rng.uniform(-.2, .2, size=w).astype(np.float32) for w in c.widths]
    return c, ks, bs, acts


@pytest.mark.parametrize('name', NAMES)
def test_train_blob_and_device_repack(nfx_lib, cuda, name):
    """The train blob's forward is the forward blob's; the device re-pack route of an fp32-class blob — the native blob
    followed by nfx_mlp_generic_split_hilo — gives the host-packed blob byte for byte, on the integer weights and on real ones."""
    from nerfactor_amd import ops
    c = G.case(name)
    x = f32(c.x[:129], cuda)
    for prec in G.PRECS:
        same(ops.mlp_generic_fwd(x, int_net(name, prec, cuda, True)), G.reference(name, prec).y[:129], '%s %s train blob' % (name, prec))
        a, b = int_net(name, prec, cuda, True).blob, int_net(name, prec, cuda, False).blob
        assert torch.equal(a[:b.numel()], b)
    _, ks, bs, acts = real_net(name, np.random.default_rng(7))
    for kk, bb, aa in (([k.astype(np.float32) for k, _ in c.layers], [b.astype(np.float32) for _, b in c.layers], c.acts), (ks, bs, acts)):
        for train in (False, True):
            host = ops.GenericNet(kk, bb, aa, c.skip_at or None, train=train, prec='fp32').to(cuda)
            native = ops.GenericNet(kk, bb, aa, c.skip_at or None, train=train, prec='fp32_native').to(cuda)
            assert not torch.equal(native.blob, host.blob)
            ops.generic_split_hilo(native.blob, native)
            assert torch.equal(native.blob, host.blob), (name, train)


# ------------------------------------------------------------------------------------------ part 2: real-valued data
N_REAL = 289
PROBE_ROWS = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 287, 288)


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_a_row_is_a_function_of_that_row(nfx_lib, nfx_opt, cuda, name, prec):
    """y and dx of a 289-row batch, row by row: equal to the row launched alone (the first, last and tile-boundary rows and a
    random sample), to every prefix, to the batch in reversed and in random order, under every nerf_blocks setting."""
    from nerfactor_amd import ops
    rng = np.random.default_rng(NAMES.index(name))
    c, ks, bs, acts = real_net(name, rng)
    net = ops.GenericNet(ks, bs, acts, c.skip_at or None, train=True, prec=prec).to(cuda)
    x = f32(rng.normal(size=(N_REAL, c.d_in)), cuda)
    dy = f32(rng.normal(size=(N_REAL, c.widths[-1])), cuda)

    def run(x, dy):
        return ops.mlp_generic_fwd(x, net), ops.mlp_generic_bwd(x, net, dy, None, None, want_dx=True)
    y, dx = run(x, dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and bool((dx != 0).any())
    rows = sorted(set(PROBE_ROWS) | set(int(v) for v in rng.choice(N_REAL, size=8, replace=False)))
    for r in rows:
        y1, dx1 = run(x[r:r + 1].contiguous(), dy[r:r + 1].contiguous())
        assert torch.equal(y1[0], y[r]) and torch.equal(dx1[0], dx[r]), (name, prec, 'row alone', r)
    for n in G.ROWS[1:-1]:
        yp, dxp = run(x[:n].contiguous(), dy[:n].contiguous())
        assert torch.equal(yp, y[:n]) and torch.equal(dxp, dx[:n]), (name, prec, 'prefix', n)
    perm = torch.from_numpy(rng.permutation(N_REAL)).to(cuda)
    for order in (torch.arange(N_REAL - 1, -1, -1, device=cuda), perm):
        yo, dxo = run(x[order].contiguous(), dy[order].contiguous())
        assert torch.equal(yo, y[order]) and torch.equal(dxo, dx[order]), (name, prec, 'another order')
    for blocks in (1, 3):
        nfx_opt.set('nerf_blocks', blocks)
        yb, dxb = run(x, dy)
        assert torch.equal(yb, y) and torch.equal(dxb, dx), (name, prec, 'nerf_blocks', blocks)


@pytest.mark.parametrize('prec', G.PRECS)
@pytest.mark.parametrize('name', NAMES)
def test_one_hot_dy_gives_that_rows_weight_gradients(nfx_lib, nfx_opt, cuda, name, prec):
    """dy non-zero in ONE row of 1299: dW and db equal, value for value, those of that row launched alone — under every
    wgrad_splits / wgrad_map setting: every other row contributes exact zeros."""
    from nerfactor_amd import ops
    rng = np.random.default_rng(100 + NAMES.index(name))
    c, ks, bs, acts = real_net(name, rng)
    net = ops.GenericNet(ks, bs, acts, c.skip_at or None, train=True, prec=prec).to(cuda)
    n = G.N_MAX
    x = f32(rng.normal(size=(n, c.d_in)), cuda)
    dy_row = f32(rng.normal(size=(1, c.widths[-1])) + 2., cuda)

    def grads(x, dy):
        dks, dbs = [torch.zeros(k.shape, device=cuda) for k in ks], [torch.zeros(b.shape, device=cuda) for b in bs]
        ops.mlp_generic_bwd(x, net, dy, dks, dbs)
        return dks + dbs
    for r in (0, 31, 32, int(rng.integers(33, n - 40)), n - 20, n - 19, n - 1):
        alone = grads(x[r:r + 1].contiguous(), dy_row)
        assert all(bool((t != 0).any()) for t in alone[len(ks):]), (name, prec, r)
        dy = torch.zeros((n, c.widths[-1]), device=cuda)
        dy[r] = dy_row[0]
        for splits in (1, 3, None):
            nfx_opt.unset('wgrad_splits') if splits is None else nfx_opt.set('wgrad_splits', splits)
            for wmap in (0, 1):
                nfx_opt.set('wgrad_map', wmap)
                for i, (a, b) in enumerate(zip(alone, grads(x, dy))):
                    assert torch.equal(a, b), (name, prec, 'row', r, 'splits', splits, 'map', wmap, 'tensor', i,
                                               float((a - b).abs().max()))
        nfx_opt.unset('wgrad_splits')
        nfx_opt.unset('wgrad_map')
