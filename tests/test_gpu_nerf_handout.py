"""The hand-out of point tiles from a device counter (option `nerf_handout`, nfx_nerf_mlp_fwd_render): bit for bit the static
walk of the same kernel over the same fold (`nerf_handout` = 0, nfx_nerf_mlp_fwd_folded), on outputs pre-filled with NaN so that
a row nobody wrote shows, at every relation of tiles to workgroups; the counter is cleared by every call (a workspace is reused,
a captured call is replayed) and ends where the protocol model of test_cpu_nerf_handout.py says.

Shapes: a tile is 256 points.  The point counts 256, 3 tiles, 41 tiles and their neighbours come from the sample counts 64, 192
and 7; the counts 1, 255, 257 and 3 tiles + 17 have no factor among those three and run at 1 or 5 samples per ray."""
import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import common

pytestmark = pytest.mark.gpu

TILE = 256
BLOCKS = (1, 2, 3, 256)     # one workgroup walks every tile (41 of them at most) ... more workgroups than tiles
# (rays, samples) -> points
SHAPES = [(4, 64), (164, 64),               # 256 = one tile exactly; 41 tiles exactly
          (4, 192), (55, 192),              # 3 tiles exactly; 41 tiles + 64 points
          (1, 7), (37, 7), (112, 7), (1500, 7),   # 7; one tile + 3; 3 tiles + 16; 41 tiles + 4
          (1, 1), (51, 5), (257, 1), (157, 5)]    # 1; 255; 257; 3 tiles + 17


def _inputs(n_rays, n_samples, cuda):
    rng = np.random.default_rng(1000 * n_samples + n_rays)
    rayo = rng.uniform(-1, 1, size=(n_rays, 3)).astype(np.float32) * 3
    rayd = nerf_ref.l2_normalize(rng.normal(size=(n_rays, 3)).astype(np.float32), 1, 1e-12)
    z = np.sort(rng.uniform(2, 6, size=(n_rays, n_samples)).astype(np.float32), -1)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (rayo, rayd, z))


@pytest.fixture(scope='module')
def blob(nfx_lib, cuda):
    from nerfactor_amd import ops
    return ops.pack_nerf_weights(*common.nerf_layers(common.nerf_nets(seed=7)[1])).to(cuda)


def _workspace(nfx_lib, cuda):
    """A render workspace of bytes 0x7f: a counter nobody clears starts at 0x7f7f7f7f, past every tile."""
    return torch.full((nfx_lib.lib.nfx_nerf_render_workspace_bytes(),), 0x7f, dtype=torch.uint8, device=cuda)


def _render(nfx_lib, rayo, rayd, z, blob, ws, out):
    from nerfactor_amd import ops
    out.fill_(float('nan'))
    nfx_lib.check(nfx_lib.lib.nfx_nerf_mlp_fwd_render(rayo.data_ptr(), rayd.data_ptr(), z.data_ptr(), z.shape[0], z.shape[1],
                                                      blob.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), ops._stream()),
                  'nfx_nerf_mlp_fwd_render')
    return out


def _control_word(ws):
    return int(ws[-16:].view(torch.int32)[0].item())


def _check_counter(ws, n_pts, blocks, what):
    tiles = -(-n_pts // TILE)
    grid = min(tiles, blocks)
    lo, got = max(tiles - grid, 0), _control_word(ws)
    print('%s: %d tiles, %d workgroups, control word %d (allowed %d .. %d)' % (what, tiles, grid, got, lo, lo + 3 * grid))
    assert lo <= got <= lo + 3 * grid, (what, got, lo, grid)
    # the kernel's own count, as in the model: every workgroup claims once in front of its loop and once per pass
    assert got == tiles + grid, (what, got, tiles, grid)


@pytest.mark.parametrize("n_rays,n_samples", SHAPES)
def test_handed_out_tiles_are_the_static_walk_bit_for_bit(nfx_lib, cuda, nfx_opt, blob, n_rays, n_samples):
    from nerfactor_amd import ops
    rayo, rayd, z = _inputs(n_rays, n_samples, cuda)
    nfx_opt.set("nerf_variant", "7")
    nfx_opt.set("nerf_handout", "0")
    nfx_opt.set("nerf_blocks", "256")
    want = ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True)
    assert not torch.isnan(want).any()
    out = torch.empty_like(want)
    for blocks in BLOCKS:
        what = '%d x %d, nerf_blocks %d' % (n_rays, n_samples, blocks)
        nfx_opt.set("nerf_blocks", str(blocks))
        ws = _workspace(nfx_lib, cuda)
        common.assert_same_bits(want, _render(nfx_lib, rayo, rayd, z, blob, ws, out), what + ', first call', row_len=4)
        _check_counter(ws, n_rays * n_samples, blocks, what)
        # the same workspace again: the counter of the first call is cleared
        common.assert_same_bits(want, _render(nfx_lib, rayo, rayd, z, blob, ws, out), what + ', second call', row_len=4)
        _check_counter(ws, n_rays * n_samples, blocks, what + ', second call')
        # and the front end takes this path when the option is on, and by default
        for setting in ("1", None):
            nfx_opt.set("nerf_handout", setting) if setting else nfx_opt.unset("nerf_handout")
            common.assert_same_bits(want, ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True), what + ', ops', row_len=4)
        nfx_opt.set("nerf_handout", "0")
        common.assert_same_bits(want, ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True), what + ', static', row_len=4)


@pytest.mark.parametrize("blocks", [2, 256])
def test_captured_once_replayed_twice(nfx_lib, cuda, nfx_opt, blob, blocks):
    from nerfactor_amd import ops
    rayo, rayd, z = _inputs(164, 64, cuda)
    nfx_opt.set("nerf_variant", "7")
    nfx_opt.set("nerf_blocks", str(blocks))
    nfx_opt.set("nerf_handout", "0")
    want = ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True)
    ws, out = _workspace(nfx_lib, cuda), torch.empty_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _render(nfx_lib, rayo, rayd, z, blob, ws, out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _render(nfx_lib, rayo, rayd, z, blob, ws, out)      # the NaN fill is part of the graph
    for replay in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        common.assert_same_bits(want, out, 'replay %d, nerf_blocks %d' % (replay, blocks), row_len=4)
        _check_counter(ws, 164 * 64, blocks, 'replay %d' % replay)


@pytest.mark.parametrize("variant", [6, 8, 1, 0])
def test_other_variants_walk_statically_through_the_new_entry_point(nfx_lib, cuda, nfx_opt, blob, variant):
    from nerfactor_amd import ops
    rayo, rayd, z = _inputs(157, 5, cuda)
    nfx_opt.set("nerf_variant", str(variant))
    nfx_opt.set("nerf_blocks", "2")
    nfx_opt.set("nerf_handout", "0")
    want = ops.nerf_mlp_fwd(rayo, rayd, z, blob, fold=True)
    ws, out = _workspace(nfx_lib, cuda), torch.empty_like(want)
    common.assert_same_bits(want, _render(nfx_lib, rayo, rayd, z, blob, ws, out), 'variant %d' % variant, row_len=4)
    assert _control_word(ws) == 0, "cleared by the fold, and no claim made"


def test_the_new_entry_point_validates(nfx_lib, cuda, blob):
    lib = nfx_lib.lib
    rayo, rayd, z = _inputs(4, 64, cuda)
    ws, out = _workspace(nfx_lib, cuda), torch.empty((4, 64, 4), device=cuda)
    args = (rayo.data_ptr(), rayd.data_ptr(), z.data_ptr(), 4, 64, blob.data_ptr())
    assert lib.nfx_nerf_mlp_fwd_render(*args, ws.data_ptr(), lib.nfx_nerf_fold_workspace_bytes(), out.data_ptr(), None) == -1
    assert 'too small' in nfx_lib.last_error()
    assert lib.nfx_nerf_mlp_fwd_render(*args, blob.data_ptr() + 1024, ws.numel(), out.data_ptr(), None) == -1
    assert 'overlaps' in nfx_lib.last_error()
    assert lib.nfx_nerf_mlp_fwd_render(*args, None, ws.numel(), out.data_ptr(), None) == -1
    assert lib.nfx_nerf_mlp_fwd_render(*args[:3], 0, 64, blob.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), None) == 0
