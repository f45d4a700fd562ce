"""Cases and CPU restatements for csrc/image_metrics.hip.  A helper, not a test.

oracle64   NumPy float64 from the definition: every window position is one direct 2-D sum over its 11 x 11 pixels with the
           121 weights exp(-(di^2 + dj^2) / (2 sigma^2)) normalised JOINTLY, as tf.image.ssim builds its kernel; the mean
           squared error is a plain float64 mean.  It shares neither the kernel's separable order nor its integer sums.
emulate    NumPy float64 in the kernel's documented order (the comment at the top of image_metrics.hip): horizontal then
           vertical pass, each accumulated in ascending tap order from g[0] f[x]; the formula as parenthesised there; every
           addend as rint(v 2^40), summed in Python integers.  NumPy neither fuses nor reorders these element-wise steps, so
           the kernel must give the same bits.
"""
import functools
import math

import numpy as np

TILE = (16, 32)          # ops.IMAGE_METRICS_TILE; tests/test_cpu_image_metrics.py checks that it is
SCALE = 2 ** 40
SIGMA, WIN = 1.5, 11

# The largest distances to oracle64 over imc.all_cases(), measured on an MI355X — they come from
# the separable-versus-joint rounding of the window sums and from the 2^-40 quantum of the integer sums, i.e. from the
# images, not from the code under test, which is pinned bit for bit to `emulate` above.  The tests allow four times these.
MEASURED = {'ssim': 4.1e-13, 'map': 5.2e-13, 'psnr': 2.0e-9}


def weights():
    """The 11 taps of one axis in Python floats, the way ops._ssim_weights writes them (the kernel takes them as given)."""
    e = [math.exp(-0.5 * (((i - 5) / 1.5) * ((i - 5) / 1.5))) for i in range(WIN)]
    s = sum(e)
    return tuple(x / s for x in e)


def weights_2d():
    d = np.arange(WIN, dtype=np.float64) - 5
    w = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2 * SIGMA ** 2))
    return w / w.sum()


def values(im, luma):
    """[H, W, C] -> float64 [H, W, C']: the values that are scored."""
    im = np.asarray(im).astype(np.float64)
    if luma and im.shape[-1] == 3:
        return ((0.2126 * im[..., 0] + 0.7152 * im[..., 1]) + 0.0722 * im[..., 2])[..., None]
    return im


# --------------------------------------------------------------------------------------------- oracle
def oracle_fields(x, y):
    """[H, W] float64 values -> (mx, my, sxy, sq) of [H - 10, W - 10], each a direct 2-D weighted sum."""
    w = weights_2d()
    win = np.lib.stride_tricks.sliding_window_view
    return tuple(np.einsum('ijkl,kl->ij', win(f, (WIN, WIN)), w) for f in (x, y, x * y, x * x + y * y))


def oracle64(a, b, max_val, luma=True, mask=None):
    """One pair [H, W, C] -> {'mse', 'psnr', 'ssim', 'map' [H - 10, W - 10, C']} in float64 from the definition."""
    va, vb = values(a, luma), values(b, luma)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    maps = []
    for ch in range(va.shape[-1]):
        mx, my, sxy, sq = oracle_fields(va[..., ch], vb[..., ch])
        lum = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)
        cs = (2 * sxy - 2 * mx * my + c2) / (sq - (mx ** 2 + my ** 2) + c2)
        maps.append(lum * cs)
    smap = np.stack(maps, -1)
    sel = np.ones(va.shape[:2], bool) if mask is None else np.asarray(mask).astype(bool)
    se = np.square(va[sel] - vb[sel])
    with np.errstate(divide='ignore', invalid='ignore'):
        mse = np.float64(np.sum(se)) / np.float64(se.size)
        psnr = 10 * np.log10(np.float64(max_val) ** 2 / mse)
    return {'mse': float(mse), 'psnr': float(psnr), 'ssim': float(smap.mean()), 'map': smap}


# --------------------------------------------------------------------------------------------- emulation
def _filter_rows(f, g):
    """sum_k g[k] f[:, x + k] in ascending k starting from g[0] f[:, x]"""
    n = f.shape[1] - (WIN - 1)
    acc = g[0] * f[:, 0:n]
    for k in range(1, WIN):
        acc = acc + g[k] * f[:, k:k + n]
    return acc


def _filter(f, g):
    return _filter_rows(_filter_rows(f, g).T, g).T       # horizontal, then the same down the columns


def _fixed(v):
    return int(np.rint(v * float(SCALE)).astype(np.int64).astype(object).sum()) if v.size else 0


def emulate(a, b, max_val, luma=True, mask=None, g=None):
    """One pair [H, W, C] -> {'map', 'totals' (the eight integers of include/nfx.h), 'mse', 'psnr', 'ssim'}."""
    g = weights() if g is None else g
    max_val = float(max_val)
    va, vb = values(a, luma), values(b, luma)
    k1, k2 = 0.01 * max_val, 0.03 * max_val
    c1, c2 = k1 * k1, k2 * k2
    sel = np.ones(va.shape[:2], bool) if mask is None else np.asarray(mask).astype(bool)
    totals, maps = [0] * 8, []
    with np.errstate(all='ignore'):
        for ch in range(va.shape[-1]):
            x, y = va[..., ch], vb[..., ch]
            mx, my, sxy, sq = (_filter(f, g) for f in (x, y, x * y, (x * x) + (y * y)))
            m = (mx * mx) + (my * my)
            p = (2. * mx) * my
            lum = (p + c1) / (m + c1)
            cs = (((2. * sxy) - p) + c2) / ((sq - m) + c2)
            v = lum * cs
            maps.append(v)
            d = (x[sel] - y[sel]) / max_val
            e = d * d
            if not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(v).all() and (e <= 1.).all()):
                totals[7] = 1
                continue
            totals[ch] = _fixed(e)
            totals[3 + ch] = _fixed(v)
            totals[6] += int(e.size)
    out = {'map': np.stack(maps, -1), 'totals': totals}
    out.update(finalize(totals, out['map'].size, max_val))
    return out


def finalize(totals, n_map, max_val):
    se, sm, n_px, flag = sum(totals[0:3]), sum(totals[3:6]), totals[6], totals[7]
    nan = float('nan')
    if flag:
        return {'mse': nan, 'psnr': nan, 'ssim': nan}
    ssim = float(sm) / float(SCALE) / float(n_map)
    if n_px == 0:
        return {'mse': nan, 'psnr': nan, 'ssim': ssim}
    peak = max_val * max_val
    mse = float(se) / float(SCALE) / float(n_px) * peak
    return {'mse': mse, 'psnr': float('inf') if se == 0 else 10. * math.log10(peak / mse), 'ssim': ssim}


# --------------------------------------------------------------------------------------------- cases
def shapes():
    ty, tx = TILE
    return ((11, 11), (11, 12), (12, 11), (ty + 10 - 1, tx + 10 + 1), (ty + 10 + 1, tx + 10 - 1), (2 * ty + 10, 2 * tx + 10 + 3))


DTYPES = ('uint8', 'float32')
BATCHES, CHANNELS, LUMAS, MASKS = (1, 3), (1, 3), (True, False), ('none', 'random', 'zero')


def max_val_of(dtype):
    return 255. if dtype == 'uint8' else 1.


@functools.lru_cache(maxsize=None)
def images(shape, dtype, C, B=3):
    """(a, b, mask) of [B, H, W, C] / [B, H, W]: a smooth ramp plus noise with a FLAT patch (where sxx_yy - (mx^2 + my^2)
    cancels to rounding), b = a disturbed; image 1 of a batch differs from a by one pixel only."""
    H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * W + C + (7 if dtype == 'uint8' else 0))
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.35 * np.sin(0.37 * yy + 0.1)[..., None] * np.cos(0.23 * xx[..., None] + np.arange(C))
    a = np.clip(base[None] + 0.08 * rng.standard_normal((B, H, W, C)), 0, 1)
    a[:, : H // 2, : W // 2] = 0.8                       # flat at a high level
    b = np.clip(a + 0.05 * rng.standard_normal((B, H, W, C)), 0, 1)
    if B > 1:
        b[1] = a[1]
        b[1, H - 1, W - 1, 0] = 1. - a[1, H - 1, W - 1, 0]       # a pixel only the last tile's halo holds
    mask = (rng.random((B, H, W)) < 0.6).astype(np.uint8)
    if dtype == 'uint8':
        a, b = (a * 255).astype(np.uint8), (b * 255).astype(np.uint8)
    else:
        a, b = a.astype(np.float32), b.astype(np.float32)
    for arr in (a, b, mask):
        arr.setflags(write=False)
    return a, b, mask


def mask_of(kind, mask):
    return None if kind == 'none' else mask if kind == 'random' else np.zeros_like(mask)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, C, luma, mask_kind, i):
    """(emulate, oracle64) of image i of the three-image batch of a case; computed once."""
    a, b, mask = images(shape, dtype, C)
    m = mask_of(mask_kind, mask)
    m = None if m is None else m[i]
    return emulate(a[i], b[i], max_val_of(dtype), luma, m), oracle64(a[i], b[i], max_val_of(dtype), luma, m)


def all_cases():
    for shape in shapes():
        for dtype in DTYPES:
            for C in CHANNELS:
                for luma in LUMAS:
                    for mask_kind in MASKS:
                        yield shape, dtype, C, luma, mask_kind
