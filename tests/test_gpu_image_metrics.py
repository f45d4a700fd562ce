"""csrc/image_metrics.hip on the GPU: the SSIM map and the integer totals equal the NumPy emulation
of the kernel's documented operation order bit for bit (tests/image_metric_cases.emulate) at one window, one off a tile seam
either way and across several tiles, for uint8 and float32, grey and RGB, luma on and off, with and without a mask; the
numbers stay inside four times the measured distance to the float64 oracle that is written from the definition (oracle64);
identities, poisoned buffers, a NaN, and every refusal of the wrapper."""
import numpy as np
import pytest
import torch

from tests import image_metric_cases as imc

pytestmark = pytest.mark.gpu

MEASURED = imc.MEASURED


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.int64), np.asarray(y, np.float64).view(np.int64))


def _run(cuda, a, b, max_val, luma, mask=None, **kw):
    from nerfactor_amd import ops
    dev = lambda t: None if t is None else torch.from_numpy(np.array(t)).to(cuda)       # a copy: the cases are read-only
    return ops.image_metrics(dev(a), dev(b), max_val, luma=luma, mask=dev(mask), **kw)


def test_tile_is_the_one_the_cases_aim_at(nfx_lib):
    from nerfactor_amd import ops
    assert tuple(ops.IMAGE_METRICS_TILE) == imc.TILE and ops.IMAGE_METRICS_WEIGHTS == imc.weights()


@pytest.mark.parametrize('dtype', imc.DTYPES)
@pytest.mark.parametrize('shape', imc.shapes(), ids=lambda s: '%dx%d' % s)
def test_map_and_totals_equal_the_emulation(shape, dtype, nfx_lib, cuda):
    """B = 1 and B = 3, C = 1 and 3, luma on and off, mask absent / random / all zero (count 0: PSNR NaN, no crash)."""
    max_val = imc.max_val_of(dtype)
    for C in imc.CHANNELS:
        a, b, mask = imc.images(shape, dtype, C)
        for luma in imc.LUMAS:
            for mask_kind in imc.MASKS:
                m = imc.mask_of(mask_kind, mask)
                for B in imc.BATCHES:
                    got = _run(cuda, a[:B], b[:B], max_val, luma, None if m is None else m[:B], return_map=True)
                    smap = got['ssim_map'].cpu().numpy()
                    where = (shape, dtype, C, luma, mask_kind, B)
                    assert smap.shape == (B, shape[0] - 10, shape[1] - 10, 1 if (luma or C == 1) else C), where
                    for i in range(B):
                        emu, _ = imc.reference(shape, dtype, C, luma, mask_kind, i)
                        assert _same_bits(smap[i], emu['map']), where
                        assert got['totals'][i].tolist() == emu['totals'], where
                        for k in ('mse', 'psnr', 'ssim'):
                            assert _same_bits(got[k][i].item(), emu[k]), (where, k, got[k][i].item(), emu[k])
                        if mask_kind == 'zero':
                            assert int(got['n_px'][i]) == 0 and np.isnan(got['psnr'][i].item()) and np.isfinite(got['ssim'][i].item())


def test_against_the_float64_oracle(nfx_lib, cuda):
    """Largest |ssim - oracle|, |map - oracle| and |psnr - oracle| (dB, pairs with mse > 0) over the whole case list; printed
    before they are asserted."""
    worst = {'ssim': 0., 'map': 0., 'psnr': 0.}
    for shape, dtype, C, luma, mask_kind in imc.all_cases():
        a, b, mask = imc.images(shape, dtype, C)
        m = imc.mask_of(mask_kind, mask)
        got = _run(cuda, a, b, imc.max_val_of(dtype), luma, m, return_map=True)
        smap = got['ssim_map'].cpu().numpy()
        for i in range(a.shape[0]):
            _, ref = imc.reference(shape, dtype, C, luma, mask_kind, i)
            worst['ssim'] = max(worst['ssim'], abs(got['ssim'][i].item() - ref['ssim']))
            worst['map'] = max(worst['map'], float(np.abs(smap[i] - ref['map']).max()))
            if mask_kind != 'zero' and ref['mse'] > 0:
                worst['psnr'] = max(worst['psnr'], abs(got['psnr'][i].item() - ref['psnr']))
    print('image_metrics vs oracle64:', worst)
    for k, v in worst.items():
        assert v <= 4 * MEASURED[k], (k, v, MEASURED[k])


def test_identities(nfx_lib, cuda):
    """ssim(x, x) is exactly 1 and psnr inf: with y = x every step of the two quotients gives bit-equal numerator and
    denominator — (2 mx) mx = 2 fl(mx mx) = fl(mx mx) + fl(mx mx), and G*(x x + x x) = 2 G*(x x) exactly because a factor
    2 passes through every product and sum unrounded — so lum = cs = 1, every addend is 2^40 and the mean is 1."""
    for dtype in imc.DTYPES:
        for C, luma in ((3, True), (3, False), (1, True)):
            a, b, mask = imc.images(imc.shapes()[5], dtype, C)
            mv = imc.max_val_of(dtype)
            same = _run(cuda, a, a, mv, luma)
            assert same['ssim'].tolist() == [1.0] * 3 and (same['psnr'] == float('inf')).all() and same['mse'].tolist() == [0.] * 3
            ab, ba = _run(cuda, a, b, mv, luma, mask, return_map=True), _run(cuda, b, a, mv, luma, mask, return_map=True)
            again = _run(cuda, a, b, mv, luma, mask, return_map=True)
            for other in (ba, again):                       # symmetric in its arguments; two runs
                assert torch.equal(ab['totals'], other['totals']) and torch.equal(ab['ssim_map'], other['ssim_map'])
            for i in range(3):                              # a batch of three = three calls of one
                one = _run(cuda, a[i:i + 1], b[i:i + 1], mv, luma, mask[i:i + 1], return_map=True)
                assert torch.equal(one['totals'][0], ab['totals'][i]) and torch.equal(one['ssim_map'][0], ab['ssim_map'][i])
                for k in ('mse', 'psnr', 'ssim'):
                    assert _same_bits(one[k][0].item(), ab[k][i].item())


def test_poisoned_workspace_and_outputs(nfx_lib, cuda):
    from nerfactor_amd import ops
    shape = imc.shapes()[5]
    for dtype, C, luma in (('uint8', 3, True), ('float32', 3, False)):
        a, b, mask = imc.images(shape, dtype, C)
        want = _run(cuda, a, b, imc.max_val_of(dtype), luma, mask, return_map=True)
        cp = 1 if luma else C
        words = nfx_lib.lib.nfx_image_metrics_workspace_bytes(3, shape[0], shape[1], C, int(luma)) // 8
        assert words > 0
        poison = lambda *s: torch.full(s, -1, dtype=torch.int64, device=cuda)          # every byte 0xFF
        totals, ws = poison(3, 8), poison(words)
        smap = poison(3, shape[0] - 10, shape[1] - 10, cp).view(torch.float64)
        got = _run(cuda, a, b, imc.max_val_of(dtype), luma, mask, totals=totals, ws=ws, ssim_map=smap)
        assert got['ssim_map'] is smap and torch.equal(got['totals'], want['totals'])
        assert torch.equal(smap.view(torch.int64), want['ssim_map'].view(torch.int64))
        assert torch.equal(totals.cpu(), want['totals'])
        with pytest.raises(nfx_lib.NfxError, match='workspace'):
            _run(cuda, a, b, imc.max_val_of(dtype), luma, mask, ws=ws[:-1])


def test_non_finite_image_is_nan_and_the_others_are_not(nfx_lib, cuda):
    shape = imc.shapes()[4]
    a, b, _ = imc.images(shape, 'float32', 3)
    want = _run(cuda, a, b, 1., True)
    for bad in (np.nan, np.inf):
        for luma in (True, False):
            b2 = b.copy()
            b2[1, 3, shape[1] - 1, 2] = bad
            got = _run(cuda, a, b2, 1., luma)
            ref = _run(cuda, a, b, 1., luma)
            for k in ('mse', 'psnr', 'ssim'):
                assert np.isnan(got[k][1].item()), (bad, luma, k)
                assert _same_bits(got[k][[0, 2]].numpy(), ref[k][[0, 2]].numpy())
    assert np.isfinite(want['ssim'].numpy()).all()
    # a pair outside the declared range (|a - b| > max_val) is NaN too, not a wrapped integer
    got = _run(cuda, a * 3, np.zeros_like(a), 1., True)
    assert np.isnan(got['psnr'].numpy()).all()


def test_refusals(nfx_lib, cuda):
    """Each is raised by the wrapper or by the C-ABI's checks, before anything is launched."""
    from nerfactor_amd import ops
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=cuda)
    ok = u8(1, 12, 12, 3)
    E = nfx_lib.NfxError
    with pytest.raises(E, match='10 x 12'):
        ops.image_metrics(u8(1, 10, 12, 3), u8(1, 10, 12, 3), 255)
    with pytest.raises(E, match='12 x 10'):
        ops.image_metrics(u8(1, 12, 10, 1), u8(1, 12, 10, 1), 255)
    with pytest.raises(E, match='C = 2'):
        ops.image_metrics(u8(1, 12, 12, 2), u8(1, 12, 12, 2), 255)
    with pytest.raises(E, match='the same'):
        ops.image_metrics(ok, u8(1, 12, 13, 3), 255)
    with pytest.raises(E, match='the same'):
        ops.image_metrics(ok[0], ok[0], 255)
    with pytest.raises(E, match='float32'):
        ops.image_metrics(ok, ok.float(), 255)
    with pytest.raises(E, match='uint8 or both float32'):
        ops.image_metrics(ok.double(), ok.double(), 255)
    with pytest.raises(E, match='contiguous'):
        ops.image_metrics(u8(1, 12, 3, 12).permute(0, 1, 3, 2), ok, 255)
    with pytest.raises(E, match='CUDA'):
        ops.image_metrics(ok.cpu(), ok, 255)
    for bad in (0, -1., float('nan'), float('inf')):
        with pytest.raises(E, match='max_val'):
            ops.image_metrics(ok, ok, bad)
    big = u8(1, 2048, 2049, 1)
    with pytest.raises(E, match='4196352 pixels'):
        ops.image_metrics(big, big, 255)
    with pytest.raises(E, match='mask'):
        ops.image_metrics(ok, ok, 255, mask=u8(1, 12, 13))
    with pytest.raises(E, match='mask'):
        ops.image_metrics(ok, ok, 255, mask=u8(1, 12, 12).float())
    with pytest.raises(E, match='ssim_map'):
        ops.image_metrics(ok, ok, 255, ssim_map=torch.zeros(1, 2, 2, 3, dtype=torch.float64, device=cuda))
    with pytest.raises(E, match='ssim_map'):
        ops.image_metrics(ok, ok, 255, ssim_map=torch.zeros(1, 2, 2, 1, dtype=torch.float32, device=cuda))
    with pytest.raises(E, match='1 <= B'):
        ops.image_metrics(u8(0, 12, 12, 3), u8(0, 12, 12, 3), 255)
    assert ops.image_metrics(ok, ok, 255)['ssim'].tolist() == [1.0]
