"""The host side of the antialiased resize, no GPU: nfx_resize_axis_table equals the NumPy restatement
bit for bit, every row of a table is a normalised run of positive weights inside the image, the restatement agrees with the
host filter the existing tests hold to the reference's probes, and the C-ABI refuses out-of-limit arguments with their numbers
before it touches a device."""
import ctypes
import math

import numpy as np
import pytest

from tests import resize_cases as rc


def _table(nfx_lib, n_in, n_out):
    from nerfactor_amd import ops
    return ops.resize_axis_table(n_in, n_out)


@pytest.mark.parametrize('n_in,n_out', rc.TABLE_CASES)
def test_axis_table_equals_the_restatement(n_in, n_out, nfx_lib):
    first, count, weights = _table(nfx_lib, n_in, n_out)
    f2, c2, w2 = rc.axis_table(n_in, n_out)
    assert weights.shape == w2.shape and weights.shape[1] == count.max()
    assert np.array_equal(first, f2) and np.array_equal(count, c2)
    assert np.array_equal(weights.view(np.int32), w2.view(np.int32))
    # the query form returns the same tap count and writes nothing
    assert nfx_lib.lib.nfx_resize_axis_table(n_in, n_out, None, None, None, 0) == count.max()


@pytest.mark.parametrize('n_in,n_out', rc.TABLE_CASES + ((16, 1), (1, 16), (1600, 100)))
def test_rows_are_normalised_runs_inside_the_image(n_in, n_out, nfx_lib):
    first, count, weights = _table(nfx_lib, n_in, n_out)
    support = max(n_in / n_out, 1.)
    assert count.max() <= math.ceil(2 * support) + 1
    for i in range(n_out):
        n = count[i]
        assert n >= 1 and first[i] >= 0 and first[i] + n <= n_in
        assert (weights[i, :n] > 0).all() and (weights[i, n:] == 0).all()
        total = np.float64(0)
        for w in weights[i, :n]:
            total += np.float64(w)
        assert abs(total - 1.) <= (n + 1) * 2. ** -24, (i, total)
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()


def test_a_wider_table_is_zero_padded_and_a_narrow_one_refused(nfx_lib):
    first, count = np.empty(3, np.int32), np.empty(3, np.int32)
    weights = np.full((3, 7), np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert nfx_lib.lib.nfx_resize_axis_table(5, 3, p(first), p(count), p(weights), 7) == 3
    f2, c2, w2 = rc.axis_table(5, 3)
    assert np.array_equal(weights[:, :3].view(np.int32), w2.view(np.int32)) and (weights[:, 3:] == 0).all()
    assert nfx_lib.lib.nfx_resize_axis_table(5, 3, p(first), p(count), p(weights), 2) < 0
    assert '3 taps, max_taps = 2' in nfx_lib.last_error()
    assert nfx_lib.lib.nfx_resize_axis_table(0, 3, None, None, None, 0) < 0
    assert 'n_in = 0, n_out = 3' in nfx_lib.last_error()
    assert nfx_lib.lib.nfx_resize_axis_table(5, 3, p(first), None, None, 3) < 0
    assert 'all given or all null' in nfx_lib.last_error()


@pytest.mark.parametrize('size,new', rc.SIZES + (((48, 64), (12, 16)),))
def test_restatement_agrees_with_the_host_filter(size, new):
    """util.light.resize_antialias is held to the reference's probes by the existing tests.  On float64 images the float32
    restatement stays within (taps_x + taps_y + 4) 2^-23 max|x| of it: each pass adds `taps` products of normalised weights,
    every one of the taps + 1 roundings at most 2^-24 of a partial sum bounded by max|x|, twice (the einsum's float32 passes
    and the restatement's), plus the two roundings of the input and the value between the passes on either side."""
    from nerfactor_amd.nerfactor.util.light import resize_antialias
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    x = rng.uniform(-2., 2., size + (3,))
    want = resize_antialias(x, new[0], new[1])
    got = rc.resize(x.astype(np.float32), new[0], new[1])
    taps_y, taps_x = rc.axis_table(size[0], new[0])[1].max(), rc.axis_table(size[1], new[1])[1].max()
    bound = (taps_x + taps_y + 4) * 2. ** -23 * np.abs(x).max()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(size, new, 'restatement vs host filter', err, 'bound', bound)
    assert got.shape == want.shape == new + (3,) and err <= bound
    # and the float64 form of the restatement is the same filter
    assert np.abs(rc.resize64(x, new[0], new[1]) - want).max() <= bound


def test_quantisation_truncates():
    v = np.array([-1., 0., 0.999 / 255, 1. / 255, 127.5 / 255, 254.999 / 255, 1., 2.], np.float32)
    assert rc.quantize(v).tolist() == [0, 0, 0, 1, 127, 254, 255, 255]


def test_c_abi_refuses_with_numbers_before_any_launch(nfx_lib):
    """Host pointers stand in for device memory: every call is refused by the argument checks, so none is dereferenced."""
    buf = np.zeros(64, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)

    def call(in_type=2, batch=1, h=8, w=8, c=3, oh=4, ow=4, taps_y=3, taps_x=3, src=p, out_uint8=0):
        rc_ = nfx_lib.lib.nfx_resize_antialias(src, in_type, batch, h, w, c, 1., p, p, p, taps_y, p, p, p, taps_x, p, out_uint8, oh, ow, None)
        return rc_, nfx_lib.last_error()

    for kw, text in (({'in_type': 3}, 'in_type = 3'), ({'batch': 0}, 'batch = 0'), ({'batch': 65536}, 'batch = 65536'),
                     ({'h': 0}, '0 x 8 -> 4 x 4'), ({'ow': 65537}, '8 x 8 -> 4 x 65537'), ({'h': 65, 'oh': 4}, '65 x 8 -> 4 x 4 shrinks'),
                     ({'w': 17, 'ow': 1}, '8 x 17 -> 4 x 1 shrinks'), ({'c': 0}, 'c = 0'), ({'c': 4097}, 'c = 4097'),
                     ({'taps_y': 34}, 'taps_y = 34'), ({'taps_x': 0}, 'taps_x = 0'), ({'src': None}, 'null pointer')):
        code, msg = call(**kw)
        assert code == -1 and text in msg, (kw, code, msg)
    code, msg = call(src=ctypes.c_void_p(buf.ctypes.data + 2))
    assert code == -2 and 'aligned' in msg
