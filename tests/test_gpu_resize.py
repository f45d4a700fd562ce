"""csrc/resize.hip on the GPU: nfx_resize_antialias equals the NumPy restatement of its documented
arithmetic (tests/resize_cases.resize) bit for bit, as float32 and as the writer's uint8, at the smallest shapes that reach
every path — one tile and several, a footprint clipped at the image's edges, identity and magnifying axes, 13 taps, channel
counts around the 16-byte vector and around a chunk of channels, all three input types — into buffers poisoned with NaN
bytes, for a batch and for its images one at a time, on another stream, and through the raw C-ABI."""
import ctypes

import numpy as np
import pytest
import torch

from tests import resize_cases as rc

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _poisoned(shape, dtype, cuda):
    """Every byte 0xFF: NaN as float32, 255 as uint8."""
    return torch.full(shape, -1, dtype=torch.int8, device=cuda).view(torch.uint8) if dtype == torch.uint8 else \
        torch.full(shape, -1, dtype=torch.int32, device=cuda).view(torch.float32)


def _dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)          # a copy: the cases are read-only


@pytest.mark.parametrize('size,new,c,dtype', rc.gpu_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_kernel_equals_the_restatement(size, new, c, dtype, nfx_lib, cuda):
    from nerfactor_amd import ops
    x = rc.image(size, c, dtype)
    want, want8 = rc.expected(size, new, c, dtype)
    xd = _dev(x, cuda)
    for out_uint8, ref in ((False, want), (True, want8)):
        out = _poisoned((3,) + new + (c,), torch.uint8 if out_uint8 else torch.float32, cuda)
        got = ops.resize_antialias(xd, new[0], new[1], out_uint8=out_uint8, out=out)
        assert got is out
        g = got.cpu().numpy()
        assert g.shape == ref.shape and g.dtype == ref.dtype
        assert np.array_equal(_bits(g), _bits(ref)), (out_uint8, int((_bits(g) != _bits(ref)).sum()), g.size)
        # batch 1, and a batch of 3 equals its three single calls
        for i in range(3):
            one = ops.resize_antialias(xd[i:i + 1].contiguous(), new[0], new[1], out_uint8=out_uint8)
            assert torch.equal(one[0].view(torch.uint8), got[i].view(torch.uint8)), (out_uint8, i)


def test_one_size_given_truncates_the_other_and_rank_3(nfx_lib, cuda):
    from nerfactor_amd import ops
    from nerfactor_amd.nerfactor.util.light import resize_antialias as host
    x = rc.image((33, 65), 3, 'float32')[0]
    xd = _dev(x, cuda)
    for kw in ({'new_h': 16}, {'new_w': 21}, {'new_h': 40}):
        got = ops.resize_antialias(xd, **kw).cpu().numpy()
        want_shape = host(x, **kw).shape
        assert got.shape == want_shape
        assert np.array_equal(_bits(got), _bits(rc.resize(x, want_shape[0], want_shape[1])))


def test_non_default_stream(nfx_lib, cuda):
    from nerfactor_amd import ops
    size, new, c, dtype = (67, 131), (33, 65), 3, 'uint8'
    want, _ = rc.expected(size, new, c, dtype)
    xd = _dev(rc.image(size, c, dtype), cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        got = ops.resize_antialias(xd, new[0], new[1])
    s.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


def test_raw_c_abi_with_tables_of_the_host_function(nfx_lib, cuda):
    """A C caller's sequence: nfx_resize_axis_table on the host, the tables copied to the device, one call; tables wider than
    the largest tap count (zero-padded) give the same bits."""
    from nerfactor_amd import ops
    size, new, c, dtype = (97, 130), (16, 21), 3, 'uint16'
    want, want8 = rc.expected(size, new, c, dtype)
    xd = _dev(rc.image(size, c, dtype).view(np.int16), cuda)           # the bytes of the uint16 image
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    tabs = []
    for n_in, n_out in ((size[0], new[0]), (size[1], new[1])):
        taps = rc.taps_bound(n_in, n_out)
        first, count, weights = np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.empty((n_out, taps), np.float32)
        h = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert nfx_lib.lib.nfx_resize_axis_table(n_in, n_out, h(first), h(count), h(weights), taps) == rc.axis_table(n_in, n_out)[1].max()
        tabs.append(tuple(torch.from_numpy(a).to(cuda) for a in (first, count, weights)) + (taps,))
    (fy, cy, wy, ty), (fx, cx, wx, tx) = tabs
    for out_uint8, ref in ((0, want), (1, want8)):
        out = _poisoned((3,) + new + (c,), torch.uint8 if out_uint8 else torch.float32, cuda)
        nfx_lib.check(nfx_lib.lib.nfx_resize_antialias(p(xd), 1, 3, size[0], size[1], c, 1. / 65535., p(fy), p(cy), p(wy), ty, p(fx), p(cx),
                                                       p(wx), tx, p(out), out_uint8, new[0], new[1],
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'nfx_resize_antialias')
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref))
    assert np.array_equal(_bits(ops.resize_antialias(xd.view(torch.uint16), new[0], new[1]).cpu().numpy()), _bits(want))


def test_wrapper_refusals(nfx_lib, cuda):
    from nerfactor_amd import ops
    E = nfx_lib.NfxError
    ok = torch.zeros(1, 8, 8, 3, device=cuda)
    with pytest.raises(E, match='CUDA'):
        ops.resize_antialias(ok.cpu(), 4, 4)
    with pytest.raises(E, match='float64'):
        ops.resize_antialias(ok.double(), 4, 4)
    with pytest.raises(E, match='contiguous'):
        ops.resize_antialias(ok.permute(0, 2, 1, 3)[:, :, ::2], 4, 4)
    with pytest.raises(E, match='at least one'):
        ops.resize_antialias(ok, None, None)
    with pytest.raises(E, match=r'\[B, H, W, C\]'):
        ops.resize_antialias(ok[0, 0], 4, 4)
    with pytest.raises(E, match='8 x 8 -> 4 x 0'):
        ops.resize_antialias(ok, 4, 0)
    with pytest.raises(E, match='shrinks an axis by more than 16'):
        ops.resize_antialias(torch.zeros(1, 17, 8, 1, device=cuda), 1, 8)
    with pytest.raises(E, match='`out`'):
        ops.resize_antialias(ok, 4, 4, out=torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=cuda))
    assert ops.resize_antialias(ok, 4, 4).abs().max().item() == 0.
