"""NumPy restatement of nfx_resize_antialias (include/nfx.h) and the cases of its tests.

axis_table: the table of one axis in fp64 — scale = n_in / n_out, support = max(scale, 1), centre (i + 0.5) scale, weight
max(0, 1 - |(x + 0.5) - centre| / support), the run of positive weights, their sum in ascending order (np.cumsum adds one
element at a time; np.sum does not), each weight divided by it and rounded to float32.  NumPy's float64 operations are single
IEEE operations, so the bits are the library's.

resize: both passes in float32, t = t + w[k] * x[k] in ascending k with the product rounded before the sum (two NumPy
operations), horizontal first; resize64: the same tables applied in float64 (the filter without the float32 roundings)."""
import functools
import math

import numpy as np

# (h, w) -> (oh, ow): both axes shrink; 33 x 65 -> 16 x 32 (one tile at a few channels, many tiles and chunks at 512: the
# tile shrinks until its footprint fits LDS); identity; magnification; 13 or more taps (scale 6.06 / 6.19); one axis an
# identity; one past the largest tile, 32 x 64 outputs, both ways
SIZES = (((5, 7), (3, 4)), ((33, 65), (16, 32)), ((16, 32), (16, 32)), ((9, 4), (20, 9)), ((97, 130), (16, 21)), ((64, 3), (4, 3)),
         ((67, 131), (33, 65)))
CHANNELS = (1, 3, 4, 5, 512, 513)
DTYPES = ('uint8', 'uint16', 'float32')
TABLE_CASES = ((1, 1), (2, 1), (3, 2), (5, 3), (7, 7), (4, 9), (9, 20), (97, 16), (800, 512), (4032, 682))


@functools.lru_cache(maxsize=None)
def axis_table(n_in, n_out):
    """(first int32 [n_out], count int32 [n_out], weights float32 [n_out, taps]), taps = the largest count, zero-padded."""
    scale = np.float64(n_in) / np.float64(n_out)
    support = max(scale, np.float64(1.))
    x = np.arange(n_in, dtype=np.float64) + 0.5
    rows = []
    for i in range(n_out):
        centre = (np.float64(i) + 0.5) * scale
        w = np.maximum(0., 1. - np.abs(x - centre) / support)
        idx = np.nonzero(w > 0.)[0]
        assert len(idx) and (np.diff(idx) == 1).all(), (n_in, n_out, i)
        run = w[idx[0]:idx[-1] + 1]
        rows.append((int(idx[0]), (run / np.cumsum(run)[-1]).astype(np.float32)))
    taps = max(len(r) for _, r in rows)
    first = np.array([f for f, _ in rows], np.int32)
    count = np.array([len(r) for _, r in rows], np.int32)
    weights = np.zeros((n_out, taps), np.float32)
    for i, (_, r) in enumerate(rows):
        weights[i, :len(r)] = r
    for a in (first, count, weights):
        a.setflags(write=False)
    return first, count, weights


def _apply(x, table, axis, dtype):
    """x [..., n_in, ...] along `axis` -> n_out, sums in ascending tap order in `dtype`."""
    first, count, weights = table
    x = np.moveaxis(x, axis, 0)
    out = np.zeros((len(first),) + x.shape[1:], dtype)
    for i in range(len(first)):
        t = np.zeros(x.shape[1:], dtype)
        for k in range(count[i]):
            t = t + dtype(weights[i, k]) * x[first[i] + k]
        out[i] = t
    return np.moveaxis(out, 0, axis)


def to_float32(x):
    """What the kernel takes as an input value: float32(v) * float32(1 / max) for the integer types."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return x
    return x.astype(np.float32) * np.float32(1. / np.iinfo(x.dtype).max)


def resize(x, oh, ow):
    """x [..., h, w, c] uint8 / uint16 / float32 -> float32 [..., oh, ow, c], the kernel's bits."""
    x = to_float32(x)
    h, w = x.shape[-3], x.shape[-2]
    mid = _apply(x, axis_table(w, ow), x.ndim - 2, np.float32)
    return _apply(mid, axis_table(h, oh), x.ndim - 3, np.float32)


def resize64(x, oh, ow):
    """The same filter in float64 on a float64 array (tables still rounded to float32 and widened)."""
    x = np.asarray(x, np.float64)
    h, w = x.shape[-3], x.shape[-2]
    mid = _apply(x, axis_table(w, ow), x.ndim - 2, np.float64)
    return _apply(mid, axis_table(h, oh), x.ndim - 3, np.float64)


def quantize(v):
    """The reference writer's uint8 of a float32 array: clip to [0, 1], times 255 in float32, truncated."""
    v = np.asarray(v, np.float32)
    return (np.minimum(np.maximum(v, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8)


def taps_bound(n_in, n_out):
    return math.ceil(2 * max(n_in / n_out, 1.)) + 1


@functools.lru_cache(maxsize=None)
def image(size, c, dtype, batch=3):
    """A read-only random batch [batch, h, w, c]; float32 values leave [0, 1] on both sides so that the uint8 output clips."""
    rng = np.random.default_rng([size[0], size[1], c, DTYPES.index(dtype)])
    shape = (batch,) + tuple(size) + (c,)
    if dtype == 'float32':
        x = rng.uniform(-0.25, 1.25, shape).astype(np.float32)
    else:
        x = rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=np.int64).astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(size, new, c, dtype):
    """The restatement of image(size, c, dtype) at `new`, computed once: (float32 [3, oh, ow, c], its uint8)."""
    out = resize(image(size, c, dtype), new[0], new[1])
    q = quantize(out)
    out.setflags(write=False)
    q.setflags(write=False)
    return out, q


def gpu_cases():
    """(size, new, c, dtype): every size with c = 3 and every input type; every c at the tile-edge size and at the smallest
    one (float32 and uint8: the 16-byte vector is 4 and 16 elements); the 13-tap and magnifying sizes with c = 5 and 4."""
    cases = [(s, n, 3, d) for s, n in SIZES for d in DTYPES]
    cases += [(s, n, c, d) for s, n in (SIZES[1], SIZES[0]) for c in CHANNELS if c != 3 for d in ('float32', 'uint8')]
    cases += [(SIZES[4][0], SIZES[4][1], 5, 'uint16'), (SIZES[3][0], SIZES[3][1], 4, 'float32'), (SIZES[3][0], SIZES[3][1], 513, 'uint16'),
              (SIZES[5][0], SIZES[5][1], 1, 'uint8'), (SIZES[2][0], SIZES[2][1], 512, 'float32')]
    return cases
