"""Image metrics with xiuminglib's call contract (xm.metric.PSNR / SSIM), scored on the GPU by ops.image_metrics
(csrc/image_metrics.hip).

    psnr = PSNR('uint8')(im1, im2, mask=None)        # dB
    ssim = SSIM('uint8')(im1, im2)

The dynamic range comes from the dtype (1 for floats, the integer range for unsigned integers; the kernel scores uint8 and
float32 images, any other dtype raises NotImplementedError).  Inputs are H x W, H x W x 1 or
H x W x 3, NumPy arrays or device tensors; RGB is reduced to luma first, as xm does.  Both metrics also take a leading
batch axis, [B, H, W, C] (a batch is always 4-D), and then return a float64 array of [B] instead of a float.
SSIM is tf.image.ssim's definition at its defaults (11 x 11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03); MS-SSIM is not
implemented."""
import numpy as np
import torch


def to_uint8(x):
    """The reference's quantisation when it writes an image (xm.io.img.write_arr): (clip(x, 0, 1) * 255) truncated."""
    if isinstance(x, torch.Tensor):
        return (x.clamp(0., 1.) * 255.).to(torch.uint8)
    return (np.clip(x, 0., 1.) * 255.).astype(np.uint8)


def rgb2lum(im):
    """xm.img.rgb2lum: 0.2126 r + 0.7152 g + 0.0722 b over the last axis."""
    assert im.shape[-1] == 3, "Input's last dimension must hold RGB"
    return 0.2126 * im[..., 0] + 0.7152 * im[..., 1] + 0.0722 * im[..., 2]


class Base():
    def __init__(self, dtype, device=None):
        self.dtype = np.dtype(dtype)
        if self.dtype.kind == 'f':
            self.drange = 1.
        elif self.dtype.kind == 'u':
            iinfo = np.iinfo(self.dtype)
            self.drange = float(iinfo.max - iinfo.min)
        else:
            raise NotImplementedError(self.dtype.kind)
        if self.dtype not in (np.dtype('uint8'), np.dtype('float32')):
            raise NotImplementedError("the metric kernel scores uint8 and float32 images, not %s" % self.dtype)
        self.device = device

    def _assert_type(self, im):
        got = np.dtype(str(im.dtype).replace('torch.', '')) if isinstance(im, torch.Tensor) else im.dtype
        assert got == self.dtype, "Input data type (%s) different from what was specified (%s)" % (got, self.dtype)

    def _assert_drange(self, im):
        actual = float(im.max()) - float(im.min())
        assert self.drange >= actual, ("The actual dynamic range (%s) is larger than what was derived from the data type (%s)"
                                       % (actual, self.drange))

    @staticmethod
    def _ensure_4d(im):
        """-> ([B, H, W, C], batched)"""
        if im.ndim == 2:
            return im[None, :, :, None], False
        if im.ndim in (3, 4):
            assert im.shape[-1] in (1, 3), "If 3D, input must have either 1 or 3 channels, but has %d" % im.shape[-1]
            return (im[None], False) if im.ndim == 3 else (im, True)
        raise ValueError("Input must be 2D (H-by-W), 3D (H-by-W-by-C) or a 4D batch, but is %dD" % im.ndim)

    def _prepare(self, im1, im2):
        """-> (a, b: contiguous device tensors [B, H, W, C], batched)"""
        out = []
        for im in (im1, im2):
            self._assert_type(im)
            im, batched = self._ensure_4d(im)
            out.append(im)
        assert out[0].shape == out[1].shape, "The two images are not even of the same shape"
        for im in out:
            self._assert_drange(im)
        device = self.device
        if device is None:
            device = next((im.device for im in out if isinstance(im, torch.Tensor) and im.is_cuda), torch.device('cuda'))
        dev = [(im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))).to(device).contiguous() for im in out]
        return dev[0], dev[1], batched

    def _score(self, key, im1, im2, mask=None):
        from . import ops
        a, b, batched = self._prepare(im1, im2)
        if mask is not None:
            if not isinstance(mask, torch.Tensor):
                mask = torch.from_numpy(np.ascontiguousarray(mask))
            if mask.ndim == (4 if batched else 3) and mask.shape[-1] == 1:      # H x W x 1, as xm allows
                mask = mask[..., 0]
            if not batched:
                mask = mask[None]
            assert tuple(mask.shape) == tuple(a.shape[:3]), ("Mask must be of shape %s, but is of shape %s"
                                                             % (tuple(a.shape[1:3]), tuple(mask.shape[1:])))
            mask = (mask != 0).to(torch.uint8).to(a.device).contiguous()     # in case it's not logical yet
        got = ops.image_metrics(a, b, self.drange, luma=True, mask=mask)[key].numpy()
        return got if batched else float(got[0])

    def __call__(self, im1, im2, **kwargs):
        raise NotImplementedError


class PSNR(Base):
    """Peak signal-to-noise ratio in dB, on the luma of RGB inputs; mask: H x W (or B x H x W), the pixels that count."""
    def __call__(self, im1, im2, mask=None):
        return self._score('psnr', im1, im2, mask=mask)


class SSIM(Base):
    """Structural similarity (tf.image.ssim's defaults), on the luma of RGB inputs."""
    def __call__(self, im1, im2, multiscale=False):
        if multiscale:
            raise NotImplementedError("MS-SSIM (tf.image.ssim_multiscale) is not implemented")
        return self._score('ssim', im1, im2)
