"""Thin torch-tensor front end of the C-ABI (include/nfx.h).  torch is plumbing here: it owns the
device buffers and the stream; every op below is one call into libnfx.so, enqueued on torch's
current stream.  Inputs must be CUDA (ROCm) fp32 contiguous tensors; anything else raises."""
import ctypes
import os

import numpy as np
import torch

from . import _capi
from ._capi import PREC_BF16, PREC_FP32, PREC_FP32_NATIVE, check, lib

# 'fp32' = fp32-class (bf16 hi / lo operand pairs on the bf16 matrix pipe); 'fp32_native' (runtime-shaped kernels only) = fp32
# operands on the native fp32 matrix instruction
_PREC = {'bf16': PREC_BF16, 'fp32': PREC_FP32, 'fp32_native': PREC_FP32_NATIVE, PREC_BF16: PREC_BF16, PREC_FP32: PREC_FP32,
         PREC_FP32_NATIVE: PREC_FP32_NATIVE}
_ACT = {None: 0, 'none': 0, 'relu': 1, 'sigmoid': 2, 'softplus': 3}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name, shape=None):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.NfxError("%s must be a CUDA/ROCm tensor (libnfx has no CPU path)" % name)
    if t.dtype != torch.float32:
        raise _capi.NfxError("%s must be float32, got %s" % (name, t.dtype))
    if not t.is_contiguous():
        t = t.contiguous()
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise _capi.NfxError("%s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    return t


# ------------------------------------------------------------------------------- packing
def _as_host_f32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _pack(fn_bytes, fn_pack, kernels, biases, extra):
    ks = [_as_host_f32(k) for k in kernels]
    bs = [_as_host_f32(b) for b in biases]
    n = len(ks)
    karr = (ctypes.c_void_p * n)(*[k.ctypes.data for k in ks])
    barr = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
    nbytes = fn_bytes(*extra)
    if nbytes == 0:
        raise _capi.NfxError("packing: unsupported configuration %r" % (extra,))
    blob = np.zeros(nbytes, np.uint8)
    check(fn_pack(karr, barr, *extra, blob.ctypes.data, nbytes), fn_pack.__name__)
    return torch.from_numpy(blob)



class NotAGather(_capi.NfxError):
    """The packer's output is not a pure gather of the parameters (no device re-pack map exists for it)."""


class DevicePacker:
    """Re-packs one network's blob ON THE DEVICE (nfx_pack_gather) from an index map derived once from the host
    packer `pack_fn(kernels, biases) -> uint8 blob`: the packer is run on arrays holding the base-256 digits (+1)
    of each parameter's flat index — exactly representable in bf16 — so the blobs it returns ARE the gather map
    (0 = padding).  A probe with every parameter = 1 + 2^-20 tells fp32 words from bf16 pairs, and the LO halves of the
    fp32-class kernels' hi / lo operand pairs from the hi ones (round 5: those blobs are re-packed on the device too)."""

    def __init__(self, pack_fn, shapes_k, shapes_b):
        # a packer whose blob is NOT a gather (the hi / lo fragments of the runtime-shaped kernels' fp32-class mode) may
        # name one that is (`pack_fn.gather_fn`: the same blob with fp32 fragments) plus the device pass that turns the
        # gathered blob into its own (`pack_fn.post(blob)`, in place): the map is derived from gather_fn, the one-time
        # bit-for-bit check still runs against pack_fn itself
        self.pack_fn = pack_fn
        self.post = getattr(pack_fn, 'post', None)
        map_fn = getattr(pack_fn, 'gather_fn', pack_fn)
        self.shapes = [tuple(s) for s in list(shapes_k) + list(shapes_b)]
        self.nk = len(shapes_k)
        sizes = [int(np.prod(s)) for s in self.shapes]
        if sum(sizes) >= 1 << 24:      # (bit 30 of a map entry is the residual flag)
            raise _capi.NfxError("DevicePacker: network too large for the 3-digit index map")
        offs = np.cumsum([0] + sizes)

        def run(arrays):
            return map_fn(arrays[:self.nk], arrays[self.nk:]).numpy()

        # probe: every parameter = 1 + 2^-20 -> an fp32 word reads 0x3f800008, a bf16 half 0x3f80 (or 0 = padding); the LO
        # half of an fp32-class operand pair (mlp_x3.hpp: bf16(v - bf16(v))) reads bf16(2^-20) = 0x3580
        probe = run([np.full(s, 1. + 2. ** -20, np.float32) for s in self.shapes]).view(np.uint32)
        is_bias = probe == np.uint32(0x3f800008)                  # "bias" = any parameter stored as fp32
        kinds = (0, 0x3f80, 0x3580)
        halves_ok = np.isin(probe & np.uint32(0xffff), kinds) & np.isin(probe >> np.uint32(16), kinds)
        if not (is_bias | halves_ok).all() or not is_bias.any():
            raise NotAGather("DevicePacker: cannot separate the fp32 and bf16 regions of the blob")
        res_lo = ~is_bias & ((probe & np.uint32(0xffff)) == 0x3580)       # this half holds a residual (lo) value
        res_hi = ~is_bias & ((probe >> np.uint32(16)) == 0x3580)
        self.n_words = int(is_bias.size)
        self.nbytes = self.n_words * 4
        lo = np.zeros(self.n_words, np.int64)
        hi = np.zeros(self.n_words, np.int64)
        fb = np.zeros(self.n_words, np.int64)
        pad_lo = pad_hi = pad_b = None
        # digit passes: parameter i = (digit_d(i) + 1) (1 + 2^-10).  bf16 of it is digit + 1 exactly (the 2^-10 part is under
        # half an ulp of any 8-bit integer), its residual is (digit + 1) 2^-10 exactly, an fp32 word holds the product
        eps = np.float32(2. ** -10)
        for d in range(3):
            arrays = [((((np.arange(offs[i], offs[i + 1]) >> (8 * d)) & 255) + 1).astype(np.float32) * (np.float32(1.) + eps)).reshape(s)
                      for i, s in enumerate(self.shapes)]
            words = run(arrays).view(np.uint32)
            vlo = (words << 16).view(np.float32).astype(np.float64)              # low bf16 of every word
            vhi = (words & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
            vlo = np.rint(np.where(res_lo, vlo * 1024., vlo)).astype(np.int64)
            vhi = np.rint(np.where(res_hi, vhi * 1024., vhi)).astype(np.int64)
            vb = np.rint(np.where(is_bias, words.view(np.float32).astype(np.float64) / (1. + 2. ** -10), 0.)).astype(np.int64)
            if d == 0:
                pad_lo, pad_hi, pad_b = vlo == 0, vhi == 0, vb == 0
            lo += np.maximum(vlo - 1, 0) << (8 * d)
            hi += np.maximum(vhi - 1, 0) << (8 * d)
            fb += np.maximum(vb - 1, 0) << (8 * d)
        lo = np.where(res_lo, lo | (1 << 30), lo)
        hi = np.where(res_hi, hi | (1 << 30), hi)
        lo[pad_lo], hi[pad_hi], fb[pad_b] = -1, -1, -1
        m = np.empty((self.n_words, 2), np.int32)
        m[:, 0] = np.where(is_bias, fb, lo)
        m[:, 1] = np.where(is_bias, -2, hi)
        self.map_host = m
        self._dev = {}
        self._checked = set()

    def _map_in_place(self, tensors):
        """(base address, device map) when every parameter is a contiguous view of one storage: the map's indices into the
        concatenation, translated to element offsets from the lowest parameter's address.  None otherwise."""
        try:
            store = tensors[0].untyped_storage().data_ptr()
            if any(t.untyped_storage().data_ptr() != store or not t.is_contiguous() or t.dtype != torch.float32 for t in tensors):
                return None
        except Exception:
            return None
        ptrs = tuple(t.data_ptr() for t in tensors)
        key = (tensors[0].device, ptrs)
        hit = self._dev.get(key)
        if hit is None:
            base = min(ptrs)
            sizes = [int(np.prod(s)) for s in self.shapes]
            offs = np.cumsum([0] + sizes)
            where = np.concatenate([np.full(k, (p - base) // 4 - offs[i], np.int64) for i, (k, p) in enumerate(zip(sizes, ptrs))])
            if max((p - base) // 4 + k for k, p in zip(sizes, ptrs)) >= 1 << 30:
                return None
            m = self.map_host.astype(np.int64)
            idx = m & 0x3fffffff
            moved = np.where(m >= 0, (idx + where[np.minimum(idx, where.size - 1)]) | (m & (1 << 30)), m)
            hit = (base, torch.from_numpy(moved.astype(np.int32)).to(tensors[0].device))
            self._dev[key] = hit
        return hit

    def pack(self, tensors):
        """tensors: the network's parameters (CUDA fp32, kernels then biases) -> uint8 CUDA blob."""
        dev = tensors[0].device
        blob = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        in_place = self._map_in_place(tensors)
        if in_place is not None:
            # the parameters are views of ONE buffer (optim.AMSGrad's flat bucket): gather straight out of it — no
            # concatenation (2 launches per blob and step, 16 of the 92 launches of a NeRFactor step)
            base, dmap = in_place
            check(lib.nfx_pack_gather(ctypes.c_void_p(base), _ptr(dmap), self.n_words, _ptr(blob), _stream()), 'nfx_pack_gather')
        else:
            if dev not in self._dev:
                self._dev[dev] = torch.from_numpy(self.map_host).to(dev)
            src = torch.cat([t.detach().reshape(-1) for t in tensors])
            check(lib.nfx_pack_gather(_ptr(src), _ptr(self._dev[dev]), self.n_words, _ptr(blob), _stream()),
                  'nfx_pack_gather')
        if self.post is not None:
            self.post(blob)
        path = 'cat' if in_place is None else ('in_place', in_place[0], tuple(t.data_ptr() for t in tensors))
        if path not in self._checked:   # once per network AND gather path (the concatenation map; every in-place map — translated
            # offsets, the bit-30 residual flag, a raw base pointer — the first time it is used): the device gather must
            # reproduce the host packer bit for bit
            want = self.pack_fn(list(tensors[:self.nk]), list(tensors[self.nk:]))
            if not torch.equal(blob.cpu(), want):
                raise _capi.NfxError("DevicePacker: device re-pack (%s path) differs from the host packer" % (
                    path if path == 'cat' else 'in-place'))
            self._checked.add(path)
        return blob


NERF_LAYER_SHAPES = [(63, 256)] + [(256, 256)] * 4 + [(319, 256)] + [(256, 256)] * 2 + \
    [(256, 1), (256, 256), (283, 128), (128, 3)]


def pack_nerf_weights(kernels, biases, prec='bf16'):
    """kernels/biases: 12 Keras-layout arrays [in,out]/[out]: enc[0..7], sigma_out, bottleneck,
    rgb_out[0], rgb_out[1] (nerfactor/models/nerf.py:53-71).  Returns the uint8 blob (host)."""
    if len(kernels) != 12 or len(biases) != 12:
        raise _capi.NfxError("pack_nerf_weights: need 12 kernels and 12 biases")
    for i, (k, b, shp) in enumerate(zip(kernels, biases, NERF_LAYER_SHAPES)):
        if tuple(k.shape) != shp or tuple(b.shape) != (shp[1],):
            raise _capi.NfxError("pack_nerf_weights: layer %d has shapes %s/%s, expected %s/%s" % (
                i, tuple(k.shape), tuple(b.shape), shp, (shp[1],)))
    return _pack(lib.nfx_nerf_packed_bytes, lib.nfx_nerf_pack_weights, kernels, biases,
                 (_PREC[prec],))


def pack_mlp128_weights(kernels, biases, in_kind, out_dim, z_dim=0, prec='bf16'):
    """kernels/biases: the 4 mlp layers + the out layer of a width-128 surface MLP
    (nerfactor/models/shape.py:79-94, nerfactor.py:128-143, brdf.py:57-66)."""
    if len(kernels) != 5 or len(biases) != 5:
        raise _capi.NfxError("pack_mlp128_weights: need 5 kernels and 5 biases")
    return _pack(lib.nfx_mlp128_packed_bytes, lib.nfx_mlp128_pack_weights, kernels, biases,
                 (in_kind, z_dim, out_dim, _PREC[prec]))


# ------------------------------------------------------------------------------ NeRF ops
def l2_normalize3(x, eps):
    x = _dev(x, 'x', (None, 3))
    out = torch.empty_like(x)
    check(lib.nfx_l2_normalize3(_ptr(x), _ptr(out), x.shape[0], eps, _stream()), 'nfx_l2_normalize3')
    return out


def l2_normalize_rows(x, eps=1e-6):
    """tf.linalg.l2_normalize(x, axis=1, epsilon=eps) of x[n, d], d <= 16 (one launch)."""
    x = _dev(x, 'x', (None, None))
    out = torch.empty_like(x)
    check(lib.nfx_l2_normalize_rows(_ptr(x), _ptr(out), x.shape[0], x.shape[1], eps, _stream()), 'nfx_l2_normalize_rows')
    return out


def l2_normalize_rows_bwd(x, dy, eps=1e-6):
    """dx of l2_normalize_rows(x) given dy = dLoss / d y (one launch)."""
    x = _dev(x, 'x', (None, None))
    dy = _dev(dy, 'dy', tuple(x.shape))
    dx = torch.empty_like(x)
    check(lib.nfx_l2_normalize_rows_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.shape[0], x.shape[1], eps, _stream()),
          'nfx_l2_normalize_rows_bwd')
    return dx


def light_smoothness(light, tv_weight, achro_weight):
    """(loss[1], grad[h, w, 3]) of the light probe's smoothness penalties (nerfactor.py:526-539), one launch."""
    light = _dev(light, 'light', (None, None, 3))
    loss = torch.empty((1,), dtype=torch.float32, device=light.device)
    grad = torch.empty_like(light)
    check(lib.nfx_light_smoothness(_ptr(light), light.shape[0], light.shape[1], float(tv_weight), float(achro_weight),
                                   _ptr(loss), _ptr(grad), _stream()), 'nfx_light_smoothness')
    return loss, grad


def all_finite(x):
    """0-dim bool CUDA tensor: no Inf / NaN in the fp32 tensor `x` (one read of x; tf.debugging.check_numerics)."""
    x = _dev(x, 'x')
    flag = torch.zeros((), dtype=torch.int32, device=x.device)
    check(lib.nfx_any_nonfinite(_ptr(x), x.numel(), _ptr(flag), _stream()), 'nfx_any_nonfinite')
    return flag == 0


def scatter_rows(src, row_of, n_all=None):
    """out[i] = src[row_of[i]] where row_of[i] >= 0, zeros elsewhere (tf.scatter_nd of the foreground rows): ONE pass that
    writes every output element once.  src [m, ...] fp32, row_of [n_all] int32."""
    src = _dev(src, 'src')
    row_of = row_of.contiguous()
    if not row_of.is_cuda or row_of.dtype != torch.int32:
        raise _capi.NfxError("scatter_rows: row_of must be a CUDA int32 tensor")
    n_all = row_of.shape[0] if n_all is None else n_all
    d = 1
    for k in src.shape[1:]:
        d *= int(k)
    out = torch.empty((n_all,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    if n_all == 0 or d == 0:   # e.g. [n, 0, 3]: a render with no light probes
        return out
    if src.shape[0] == 0:      # no foreground row at all
        return out.zero_()
    check(lib.nfx_scatter_rows(_ptr(src), ctypes.c_void_p(row_of.data_ptr()), n_all, d, _ptr(out), _stream()),
          'nfx_scatter_rows')
    return out


def gen_z(near, far, n_samples, n_rays, lin_in_disp=False, u=None, device='cuda'):
    u = _dev(u, 'u', (n_rays, n_samples))
    z = torch.empty((n_rays, n_samples), dtype=torch.float32, device=device)
    check(lib.nfx_gen_z(near, far, n_samples, n_rays, int(lin_in_disp), _ptr(u), _ptr(z), _stream()),
          'nfx_gen_z')
    return z


def nerf_fold_blob(blob):
    """The render blob of a packed bf16 NeRF blob (CUDA uint8): the bottleneck folded into rgb_out[0] on the device
    (csrc/nerf_fold.hip).  nerf_mlp_fwd does this itself on every folded call; exposed for the tests."""
    if not blob.is_cuda or blob.dtype != torch.uint8:
        raise _capi.NfxError("blob must be a CUDA uint8 tensor")
    ws = torch.empty(lib.nfx_nerf_fold_workspace_bytes(), dtype=torch.uint8, device=blob.device)
    check(lib.nfx_nerf_fold_blob(_ptr(blob), _ptr(ws), ws.numel(), _stream()), 'nfx_nerf_fold_blob')
    return ws


def nerf_mlp_fwd(rayo, rayd, z, blob, prec='bf16', fold=None):
    """rgbs[N,S,4] = NeRF MLP at rayo + rayd*z with view direction rayd (already normalised).

    fold (bf16 only; no effect on 'fp32'): render with the network's linear bottleneck folded into rgb_out[0] — 70 tiles
    instead of 78, the same density bits, rgb logits within one bf16 layer's rounding of the unfolded kernel's.  None =
    the option `nerf_fold` (on unless set to 0).  Training passes False: its backward re-computes the unfolded forward."""
    rayo = _dev(rayo, 'rayo', (None, 3))
    n = rayo.shape[0]
    rayd = _dev(rayd, 'rayd', (n, 3))
    z = _dev(z, 'z', (n, None))
    if not blob.is_cuda or blob.dtype != torch.uint8:
        raise _capi.NfxError("blob must be a CUDA uint8 tensor")
    s = z.shape[1]
    out = torch.empty((n, s, 4), dtype=torch.float32, device=z.device)
    if fold is None:
        fold = _capi.get_option('nerf_fold') != 0
    if fold and _PREC[prec] == PREC_BF16:
        # the render blob is re-made on every call (blobs are re-packed in place during training, a cache keyed on the
        # address could go stale); the workspace comes from torch's caching allocator: no host synchronisation, safe
        # under stream capture
        # option nerf_handout (on unless set to 0): the default kernel takes its point tiles from a device counter in the
        # workspace's control block, which the fold clears on every call (csrc/nerf_mlp_v6.hip; same bits)
        if _capi.get_option('nerf_handout') != 0:
            ws = torch.empty(lib.nfx_nerf_render_workspace_bytes(), dtype=torch.uint8, device=z.device)
            check(lib.nfx_nerf_mlp_fwd_render(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(blob), _ptr(ws), ws.numel(),
                                              _ptr(out), _stream()), 'nfx_nerf_mlp_fwd_render')
            return out
        ws = torch.empty(lib.nfx_nerf_fold_workspace_bytes(), dtype=torch.uint8, device=z.device)
        check(lib.nfx_nerf_mlp_fwd_folded(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(blob), _ptr(ws), ws.numel(),
                                          _ptr(out), _stream()), 'nfx_nerf_mlp_fwd_folded')
        return out
    check(lib.nfx_nerf_mlp_fwd(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(blob), _PREC[prec],
                               _ptr(out), _stream()), 'nfx_nerf_mlp_fwd')
    return out


def composite_fwd(rgbs, z, rayd, white_bg=True, noise=None, want_weights=True):
    rgbs = _dev(rgbs, 'rgbs', (None, None, 4))
    n, s = rgbs.shape[:2]
    z = _dev(z, 'z', (n, s))
    rayd = _dev(rayd, 'rayd', (n, 3))
    noise = _dev(noise, 'noise', (n, s))
    dev = rgbs.device
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    occu = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty_like(occu)
    disp = torch.empty_like(occu)
    w = torch.empty((n, s), dtype=torch.float32, device=dev) if want_weights else None
    check(lib.nfx_composite_fwd(_ptr(rgbs), _ptr(z), _ptr(rayd), _ptr(noise), n, s, int(white_bg),
                                _ptr(rgb), _ptr(occu), _ptr(depth), _ptr(disp), _ptr(w), _stream()),
          'nfx_composite_fwd')
    return rgb, occu, depth, disp, w


def nerf_surface(sigma, z, rayo, rayd, occu_thres=0., quantize_alpha=True, want_occu=False):
    """(alpha[N], xyz[N,3], depth[N], occu[N] or None) of the fine densities sigma[N,S] at depths z[N,S] along unit
    rays: compositing, occupancy / expected depth and geometry_from_nerf.process_view's epilogue in one launch
    (nfx_nerf_surface_fwd)."""
    sigma = _dev(sigma, 'sigma', (None, None))
    n, s = sigma.shape
    z = _dev(z, 'z', (n, s))
    rayo = _dev(rayo, 'rayo', (n, 3))
    rayd = _dev(rayd, 'rayd', (n, 3))
    dev = sigma.device
    alpha = torch.empty((n,), dtype=torch.float32, device=dev)
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    depth = torch.empty_like(alpha)
    occu = torch.empty_like(alpha) if want_occu else None
    check(lib.nfx_nerf_surface_fwd(_ptr(sigma), _ptr(z), _ptr(rayo), _ptr(rayd), n, s, float(occu_thres),
                                   int(bool(quantize_alpha)), _ptr(alpha), _ptr(xyz), _ptr(depth), _ptr(occu),
                                   _stream()), 'nfx_nerf_surface_fwd')
    return alpha, xyz, depth, occu


def sample_fine(z, weights, n_fine, u=None):
    z = _dev(z, 'z', (None, None))
    n, nc = z.shape
    weights = _dev(weights, 'weights', (n, nc))
    u = _dev(u, 'u', (n, n_fine))
    out = torch.empty((n, nc + n_fine), dtype=torch.float32, device=z.device)
    check(lib.nfx_sample_fine(_ptr(z), _ptr(weights), n, nc, n_fine, _ptr(u), _ptr(out), _stream()),
          'nfx_sample_fine')
    return out


# --------------------------------------------------------------------------- diagnostics
def selftest_mfma_bf16(a, b):
    a = _dev(a, 'a', (32, 16))
    b = _dev(b, 'b', (16, 32))
    d = torch.empty((32, 32), dtype=torch.float32, device=a.device)
    check(lib.nfx_selftest_mfma_bf16(_ptr(a), _ptr(b), _ptr(d), _stream()), 'nfx_selftest_mfma_bf16')
    return d


# ------------------------------------------------------------------------------ runtime-shaped MLP (mlp_generic.hip)
class GenericNet:
    """A packed mlp.Network of arbitrary shape for mlp_generic_fwd / mlp_generic_bwd: blob (uint8 tensor, move it with
    .to(device)) + the layer description the C-ABI takes.  skip_at: the reference's list (after layer i the input is
    re-concatenated, y first: nerfactor/networks/mlp.py:47-48).  train = True packs the train blob (forward fragments +
    transposed fragments for the backward); the forward accepts either.  prec = 'fp32': fp32-class — fp32 activations and
    gradients, every MFMA operand a bf16 hi / lo pair (fragments pre-split by the packer); prec = 'fp32_native': fp32
    fragments for the native fp32 matrix instruction (nothing rounded to bf16, ~5x the matrix time)."""

    def __init__(self, kernels, biases, acts, skip_at=None, train=False, prec='bf16'):
        ks = [_as_host_f32(k) for k in kernels]
        bs = [_as_host_f32(b) for b in biases]
        n = len(ks)
        if n == 0 or len(bs) != n or len(acts) != n:
            raise _capi.NfxError("GenericNet: kernels, biases and acts must have the same, non-zero length")
        self.widths = [int(k.shape[1]) for k in ks]
        skip_at = set(skip_at or [])
        if any(i < 0 or i >= n - 1 for i in skip_at):
            # (a skip behind the last layer widens the network's OUTPUT to concat(y, x): the kernel has no such mode, and
            # dropping it silently would evaluate another function — the caller appends x itself, models/nerf.py:_enc_out)
            raise _capi.NfxError("GenericNet: skip_at %s — a skip must sit behind one of the layers 0 .. %d" % (sorted(skip_at), n - 2))
        self.skip_input = [1 if (i - 1) in skip_at else 0 for i in range(n)]
        self.d_in = int(ks[0].shape[0])
        for i in range(n):
            want = (self.d_in if i == 0 else self.widths[i - 1] + (self.d_in if self.skip_input[i] else 0))
            if ks[i].shape[0] != want or bs[i].shape != (self.widths[i],):
                raise _capi.NfxError("GenericNet: layer %d has kernel %s / bias %s, expected [%d, %d] / [%d]" % (
                    i, ks[i].shape, bs[i].shape, want, self.widths[i], self.widths[i]))
        self.acts = [_ACT[a] for a in acts]
        self._w = (ctypes.c_int * n)(*self.widths)
        self._s = (ctypes.c_int * n)(*self.skip_input)
        self._a = (ctypes.c_int * n)(*self.acts)
        size_fn, pack_fn = ((lib.nfx_mlp_generic_train_packed_bytes, lib.nfx_mlp_generic_pack_train) if train else
                            (lib.nfx_mlp_generic_packed_bytes, lib.nfx_mlp_generic_pack))
        self.prec = _PREC[prec]
        nbytes = size_fn(self.d_in, n, self._w, self._s, self.prec)
        if nbytes == 0:
            raise _capi.NfxError("GenericNet: shape outside the generic kernel's limits: " + _capi.last_error())
        blob = np.zeros(nbytes, np.uint8)
        karr = (ctypes.c_void_p * n)(*[k.ctypes.data for k in ks])
        barr = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        check(pack_fn(karr, barr, self.d_in, n, self._w, self._s, self.prec, blob.ctypes.data, nbytes), 'nfx_mlp_generic_pack')
        self.blob = torch.from_numpy(blob)
        self.n_layers, self.d_out, self.train = n, self.widths[-1], bool(train)
        self.in_dims = [self.d_in if i == 0 else self.widths[i - 1] + (self.d_in if self.skip_input[i] else 0)
                        for i in range(n)]

    def to(self, device):
        self.blob = self.blob.to(device)
        return self


def generic_split_hilo(blob, net):
    """In place, on the device: the fragments of a prec = 'fp32_native' blob of `net`'s shape -> prec = 'fp32' (hi / lo pairs)."""
    if not blob.is_cuda or blob.dtype != torch.uint8:
        raise _capi.NfxError("generic_split_hilo: blob must be a CUDA uint8 tensor")
    check(lib.nfx_mlp_generic_split_hilo(_ptr(blob), net.d_in, net.n_layers, net._w, net._s, int(net.train), _stream()),
          'nfx_mlp_generic_split_hilo')
    return blob


def generic_pack_fn(acts, skip_at, train, prec, descs, tag):
    """The `pack_fn(kernels, biases) -> host blob` the models hand to their blob cache (models/base.py:_packed) for a
    runtime-shaped network; the first call leaves the GenericNet (layer description) in descs[tag].  fp32-class blobs
    carry what ops.DevicePacker needs to rebuild them on the device: the native-fp32 packer (a pure gather) and the
    in-place hi / lo split."""
    def pack(k, b):
        g = GenericNet(k, b, acts, skip_at, train=train, prec=prec)
        descs.setdefault(tag, g)
        return g.blob
    if _PREC[prec] == PREC_FP32:
        shape = {}       # (the layer description nfx_mlp_generic_split_hilo takes: the same for both fp32 layouts)

        def gather(k, b):
            g = GenericNet(k, b, acts, skip_at, train=train, prec='fp32_native')
            shape.setdefault('net', g)
            return g.blob
        pack.gather_fn = gather
        pack.post = lambda blob: generic_split_hilo(blob, shape['net'])
    return pack


def _check_out(who, out, n, col0, width, device):
    """An `out` / `col0` destination: CUDA fp32 [n, >= col0 + width] with unit column stride on `device`."""
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 \
            or out.shape[0] != n or out.stride(1) != 1 or out.device != device:
        raise _capi.NfxError("%s: out must be a CUDA fp32 [%d, ld] matrix with unit column stride on %s" % (who, n, device))
    if col0 < 0 or col0 + width > out.shape[1]:
        raise _capi.NfxError("%s: columns [%d, %d) do not fit out's %d columns" % (who, col0, col0 + width, out.shape[1]))


def mlp_generic_fwd(x, net, out=None, col0=0):
    """y[n, d_out] = net(x[n, >= d_in]) through the runtime-shaped fused kernel; `out` / `col0`: write into columns
    [col0, col0 + d_out) of an existing [n, ld] matrix (assembling a concatenation without a copy)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _capi.NfxError("mlp_generic_fwd: x must be a CUDA fp32 matrix with unit column stride")
    n = x.shape[0]
    if x.shape[1] < net.d_in:
        raise _capi.NfxError("mlp_generic_fwd: x has %d columns, the network reads %d" % (x.shape[1], net.d_in))
    if out is None:
        out = torch.empty((n, col0 + net.d_out), dtype=torch.float32, device=x.device)
    _check_out('mlp_generic_fwd', out, n, col0, net.d_out, x.device)
    check(lib.nfx_mlp_generic_fwd(_ptr(x), n, x.stride(0) if n else net.d_in, net.d_in, net.n_layers, net._w, net._a,
                                  net._s, _ptr(net.blob), net.prec, _ptr(out), out.stride(0) if n else out.shape[1],
                                  col0, _stream()), 'nfx_mlp_generic_fwd')
    return out


def mlp_generic_bwd(x, net, dy, dkernels, dbiases, want_dx=False):
    """Backward of mlp_generic_fwd(x, net): ADDS dLoss/dW into dkernels[i] ([in_i, widths[i]]) and dLoss/db into
    dbiases[i] given dy[n, d_out] = dLoss/d y; returns dLoss/dx [n, d_in] when want_dx (chained networks), else None.
    `net` must carry a train blob (GenericNet(..., train=True))."""
    if not net.train:
        raise _capi.NfxError("mlp_generic_bwd: the network was packed without the backward fragments (train=True)")
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _capi.NfxError("mlp_generic_bwd: x must be a CUDA fp32 matrix with unit column stride")
    n = x.shape[0]
    if x.shape[1] < net.d_in:
        raise _capi.NfxError("mlp_generic_bwd: x has %d columns, the network reads %d" % (x.shape[1], net.d_in))
    dy = _dev(dy, 'dy', (n, net.d_out))
    if dkernels is None and dbiases is None:          # input gradient of a frozen network
        if not want_dx:
            raise _capi.NfxError("mlp_generic_bwd: nothing to compute (no gradient buffers, want_dx = False)")
        dkernels = dbiases = ()
    elif len(dkernels) != net.n_layers or len(dbiases) != net.n_layers:
        raise _capi.NfxError("mlp_generic_bwd: need %d kernel and bias gradient buffers" % net.n_layers)
    for i in range(len(dkernels)):
        for t, name, shape in ((dkernels[i], 'dkernels', (net.in_dims[i], net.widths[i])), (dbiases[i], 'dbiases', (net.widths[i],))):
            if _dev(t, '%s[%d]' % (name, i), shape) is not t:
                raise _capi.NfxError("mlp_generic_bwd: %s[%d] must be contiguous (it is accumulated into)" % (name, i))
    dx = torch.empty((n, net.d_in), dtype=torch.float32, device=x.device) if want_dx else None
    nbytes = lib.nfx_mlp_generic_bwd_workspace_bytes(n, net.d_in, net.n_layers, net._w, net._s, net.prec)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    karr = (ctypes.c_void_p * net.n_layers)(*[t.data_ptr() for t in dkernels]) if dkernels else None
    barr = (ctypes.c_void_p * net.n_layers)(*[t.data_ptr() for t in dbiases]) if dbiases else None
    check(lib.nfx_mlp_generic_bwd(_ptr(x), n, x.stride(0) if n else net.d_in, net.d_in, net.n_layers, net._w, net._a,
                                  net._s, _ptr(net.blob), net.prec, _ptr(dy), net.d_out, 0, _ptr(dx), net.d_in, karr,
                                  barr, _ptr(ws), ws.numel(), _stream()), 'nfx_mlp_generic_bwd')
    return dx


def embed_bwd(n_freqs, x, d_out, incl_input=True, col0=0):
    """dx[n, 3] = (d embed(x) / d x)^T d_out[:, col0 : col0 + 3 incl_input + 6 n_freqs] for explicit vectors x[n, 3]."""
    x = _dev(x, 'x', (None, 3))
    if not isinstance(d_out, torch.Tensor) or not d_out.is_cuda or d_out.dtype != torch.float32 or d_out.dim() != 2 \
            or d_out.stride(1) != 1 or d_out.shape[0] != x.shape[0]:
        raise _capi.NfxError("embed_bwd: d_out must be a CUDA fp32 matrix with one row per vector")
    dx = torch.empty_like(x)
    check(lib.nfx_embed_bwd(_ptr(x), x.shape[0], n_freqs, int(incl_input), _ptr(d_out), d_out.stride(0) if x.shape[0] else 0,
                            col0, _ptr(dx), _stream()), 'nfx_embed_bwd')
    return dx


def embed(n_freqs, incl_input=True, x=None, rayo=None, rayd=None, z=None, per_ray=1, out=None, col0=0, lights=None):
    """Embedder (embedder.py:23-47) on the device: of x[n, 3] (per_ray rows per vector), of the points rayo + rayd z
    (z[n_rays, S] -> n_rays S rows), of the ray directions (rayd with per_ray rows each), or — lights[L, 3] given — of the
    unit directions from every point x[n] to every light (n L rows, shape.py:128-131).  Returns / fills
    out[:, col0 : col0 + 3 incl_input + 6 n_freqs]."""
    d_out = (3 if incl_input else 0) + 6 * n_freqs
    if lights is not None:
        mode, a, b, c = 3, _dev(x, 'x', (None, 3)), _dev(lights, 'lights', (None, 3)), None
        per_ray = b.shape[0]
        n = a.shape[0] * per_ray
    elif z is not None:
        mode, n, per_ray = 1, z.numel(), z.shape[1]
        a, b, c = _dev(rayo, 'rayo', (None, 3)), _dev(rayd, 'rayd', (None, 3)), _dev(z, 'z')
    elif x is not None:
        mode, a, b, c = 0, _dev(x, 'x', (None, 3)), None, None
        n = a.shape[0] * per_ray
    else:
        mode, a, b, c = 2, None, _dev(rayd, 'rayd', (None, 3)), None
        n = b.shape[0] * per_ray
    dev_ = (a if a is not None else b).device
    if out is None:
        out = torch.empty((n, col0 + d_out), dtype=torch.float32, device=dev_)
    _check_out('embed', out, n, col0, d_out, dev_)
    check(lib.nfx_embed(_ptr(a), _ptr(b), _ptr(c), n, per_ray, mode, n_freqs, 1 if incl_input else 0, _ptr(out),
                        out.stride(0) if n else d_out, col0, _stream()), 'nfx_embed')
    return out


def selftest_tr16(h=None, z=None):
    """h, z: [16, 32] row-major tiles -> D[32, 32] = h^T z through LDS + ds_read_b64_tr_b16 (csrc/tr16.hpp); no arguments:
    the instruction's raw lane map, [64, 4]."""
    if h is None:
        d = torch.empty((64, 4), dtype=torch.float32, device='cuda')
        check(lib.nfx_selftest_tr16(None, None, _ptr(d), 1, _stream()), 'nfx_selftest_tr16')
        return d
    h, z = _dev(h, 'h', (16, 32)), _dev(z, 'z', (16, 32))
    d = torch.empty((32, 32), dtype=torch.float32, device=h.device)
    check(lib.nfx_selftest_tr16(_ptr(h), _ptr(z), _ptr(d), 0, _stream()), 'nfx_selftest_tr16')
    return d


def selftest_sincos(x, which):
    x = _dev(x, 'x')
    out = torch.empty_like(x)
    check(lib.nfx_selftest_sincos(_ptr(x), x.numel(), int(which), _ptr(out), _stream()),
          'nfx_selftest_sincos')
    return out


def _wgrad_dims(dims):
    n = len(dims)
    return n, (ctypes.c_int * n)(*[int(d[0]) for d in dims]), (ctypes.c_int * n)(*[int(d[1]) for d in dims])


def selftest_wgrad_plan(dims, rows):
    """dims: [(k_in, n_out), ...] of a weight-gradient batch -> {'use_lds', 'wide', 'slab', 'n_slabs'} under the current
    options.  Host only."""
    n, k, o = _wgrad_dims(dims)
    use_lds, wide, n_slabs, slab = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    check(lib.nfx_selftest_wgrad_plan(n, k, o, int(rows), ctypes.byref(use_lds), ctypes.byref(wide), ctypes.byref(slab),
                                      ctypes.byref(n_slabs)), 'nfx_selftest_wgrad_plan')
    return {'use_lds': bool(use_lds.value), 'wide': bool(wide.value), 'slab': slab.value, 'n_slabs': n_slabs.value}


def selftest_wgrad_partial_bytes(dims, rows):
    """Bytes of partial-sum workspace selftest_wgrad_batch needs for dims = [(k_in, n_out), ...].  Host only."""
    n, k, o = _wgrad_dims(dims)
    return int(lib.nfx_selftest_wgrad_partial_bytes(n, k, o, int(rows)))


def selftest_wgrad_batch(calls, ld, rows, partial, count=None, partial_bytes=None):
    """calls: [(xt, zt, k_in, n_out, dw, db | None), ...] — xt / zt feature-pair-major bf16 [ceil(F / 2), ld, 2], dw / db fp32,
    accumulated into (include/nfx.h: nfx_selftest_wgrad_batch).  Tensors are taken as they are (views included)."""
    n, k, o = _wgrad_dims([(c[2], c[3]) for c in calls])
    col = lambda j: (ctypes.c_void_p * n)(*[None if c[j] is None else c[j].data_ptr() for c in calls])
    if partial_bytes is None:
        partial_bytes = partial.numel() * partial.element_size()
    check(lib.nfx_selftest_wgrad_batch(n, col(0), col(1), k, o, col(4), col(5), int(ld), int(rows), _ptr(count), _ptr(partial),
                                       int(partial_bytes), _stream()), 'nfx_selftest_wgrad_batch')


# ------------------------------------------------------------------------- NeRFactor ops
def mlp128_xyz_fwd(xyz, blob, out_dim, out_act=None, xyz_scale=1., post_scale=1., post_bias=0.,
                   prec='bf16'):
    """out[n, out_dim] = post_scale * act(out(mlp(posenc10(xyz_scale * xyz)))) + post_bias."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    out = torch.empty((n, out_dim), dtype=torch.float32, device=xyz.device)
    check(lib.nfx_mlp128_xyz_fwd(_ptr(xyz), n, xyz_scale, _ptr(blob), out_dim, _ACT[out_act],
                                 post_scale, post_bias, _PREC[prec], _ptr(out), _stream()),
          'nfx_mlp128_xyz_fwd')
    return out


def lvis_rows_supported(prec='bf16'):
    """Does a render store its visibilities (and OLAT renders) straight into the rows of the full-size buffers
    (nfx_lvis_fwd_rows / nfx_shade_olat_fwd_rows)?  OPT-IN: nfx_set_option("lvis_rows", 1) — measured on one box, 20 steps
    each, A/B/A/B (profiles/r06/render_rows_ab.txt): NeRFactor-microfacet render 21.48 / 21.31 ms with, 22.10 / 21.15 without;
    learned BRDF 31.26 / 30.94 against 30.72 / 30.48; OLAT view 22.57 / 22.41 against 22.79 / 22.81 — the scatter and
    check_numerics passes it removes (~0.8 ms of traffic) are paid back by a 1 % slower kernel and the zero-fill: no gain worth
    a second two-waves-per-SIMD kernel form as the default.  bf16 kernels with the network resident in LDS only."""
    return prec == 'bf16' and _capi.get_option("lvis_variant") in (None, 8, 2, 3, 4) and _capi.get_option("lvis_rows") == 1


def zero_rows(dst, row_of):
    """dst[i, :] = 0 where row_of[i] < 0 (the background rows of a tf.scatter_nd whose foreground rows a kernel writes itself)."""
    dst = _dev(dst, 'dst', (row_of.shape[0], None))
    if not row_of.is_cuda or row_of.dtype != torch.int32 or not row_of.is_contiguous():
        raise _capi.NfxError("zero_rows: row_of must be a contiguous CUDA int32 tensor")
    check(lib.nfx_zero_rows(_ptr(dst), ctypes.c_void_p(row_of.data_ptr()), dst.shape[0], dst.shape[1], _stream()), 'nfx_zero_rows')
    return dst


def lvis_fwd(xyz, lxyz, blob, xyz_scale=1., xyz_dir=None, prec='bf16', out=None, out_row=None, nan_flag=None):
    """lvis[n, L]: the light-visibility MLP for every (surface point, light) pair.  `xyz_dir`
    (default xyz) are the points the light directions are taken from.
    Round 6: with `out` [n_all, L] and `out_row` [n] int32 the visibilities of point i are stored at out[out_row[i]] — the
    zero-filled scatter of shape.py:171-176 without its pass (the caller zeroes the other rows: zero_rows) — and `nan_flag`
    (int32[1], zeroed by the caller) receives a 1 if any of them is NaN (tf.debugging.check_numerics without its pass)."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    xyz_dir = _dev(xyz_dir, 'xyz_dir', (xyz.shape[0], 3))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    n, nl = xyz.shape[0], lxyz.shape[0]
    ws_bytes = 0 if prec == 'fp32' else lib.nfx_lvis_workspace_bytes(n)   # (the fp32-class kernel has no per-point fold)
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.float32, device=xyz.device)
    if out_row is not None:
        if out is None or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != nl:
            raise _capi.NfxError("lvis_fwd: `out` must be a contiguous CUDA float32 [n_all, %d] tensor" % nl)
        if not out_row.is_cuda or out_row.dtype != torch.int32 or not out_row.is_contiguous() or out_row.shape != (n,):
            raise _capi.NfxError("lvis_fwd: `out_row` must be a contiguous CUDA int32 [%d] tensor" % n)
        check(lib.nfx_lvis_fwd_rows(_ptr(xyz), _ptr(xyz_dir), n, xyz_scale, _ptr(lxyz), nl, _ptr(blob), _PREC[prec], _ptr(ws),
                                    ws.numel() * 4, ctypes.c_void_p(out_row.data_ptr()), _ptr(out),
                                    None if nan_flag is None else ctypes.c_void_p(nan_flag.data_ptr()), _stream()), 'nfx_lvis_fwd_rows')
        return out
    out = torch.empty((n, nl), dtype=torch.float32, device=xyz.device)
    check(lib.nfx_lvis_fwd(_ptr(xyz), _ptr(xyz_dir), n, xyz_scale, _ptr(lxyz), nl, _ptr(blob), _PREC[prec], _ptr(ws),
                           ws.numel() * 4, _ptr(out), _stream()), 'nfx_lvis_fwd')
    _lvis_verify(out, xyz, xyz_dir, xyz_scale, lxyz, blob, prec)
    return out


_lvis_launches = [0]


def _lvis_verify(out, xyz, xyz_dir, xyz_scale, lxyz, blob, prec, every=100, max_points=8192):
    """nfx_set_option("lvis_verify", k): every k-th launch of the DEFAULT light-visibility kernel (resident128_kernel<2, 0, 8>:
    two waves per SIMD — the regime in which a sibling kernel, brdf_compact_kernel<2, 0, 8>, returns wrong rows for a reason
    three rounds of probes have not found) is checked against the one-wave-per-SIMD kernel (variant 4)
    on every `every`-th point: the two are the same sums in the same order, so ANY differing bit raises NfxError.  Costs
    ~1 % of the launch plus one host read; skipped while a hipGraph is being captured (nothing may wait there)."""
    k = _capi.get_option("lvis_verify")
    if not k or k <= 0 or prec != 'bf16' or out.shape[0] == 0:
        return
    variant = _capi.get_option("lvis_variant")
    if variant not in (None, 8) or torch.cuda.is_current_stream_capturing():
        return
    _lvis_launches[0] += 1
    if _lvis_launches[0] % k:
        return
    n = out.shape[0]
    step = max(1, min(every, n), -(-n // max_points))
    pick = torch.arange(0, n, step, device=out.device)
    x, xd = xyz[pick].contiguous(), (xyz if xyz_dir is None else xyz_dir)[pick].contiguous()
    nl = lxyz.shape[0]
    ref = torch.empty((x.shape[0], nl), dtype=torch.float32, device=out.device)
    ws = torch.empty((max(lib.nfx_lvis_workspace_bytes(x.shape[0]), 16) // 4,), dtype=torch.float32, device=out.device)
    with _capi.option("lvis_variant", 4):
        check(lib.nfx_lvis_fwd(_ptr(x), _ptr(xd), x.shape[0], xyz_scale, _ptr(lxyz), nl, _ptr(blob), _PREC[prec], _ptr(ws),
                               ws.numel() * 4, _ptr(ref), _stream()), 'nfx_lvis_fwd(verify)')
    got = out[pick]
    if not torch.equal(got, ref):
        bad = (got != ref)
        rows = torch.nonzero(bad.any(1))[:, 0]
        raise _capi.NfxError("lvis_verify: resident128_kernel<2, 0, 8> differs from the one-wave-per-SIMD kernel on %d of %d checked "
                             "points (%d elements, first point %d, max |diff| %.3e) — set lvis_variant = 4" % (
                                 rows.numel(), x.shape[0], int(bad.sum()), int(pick[rows[0]]), float((got - ref).abs().max())))


def brdf_spec_fwd(xyz, cam, normal, z, lxyz, blob, prec='bf16'):
    """spec[n, L]: learned-BRDF specular term (0 for back-lit directions)."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    cam = _dev(cam, 'cam', (n, 3))
    normal = _dev(normal, 'normal', (n, 3))
    z = _dev(z, 'z', (n, None))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    out = torch.empty((n, nl), dtype=torch.float32, device=xyz.device)
    check(lib.nfx_brdf_spec_fwd(_ptr(xyz), _ptr(cam), _ptr(normal), _ptr(z), z.shape[1], _ptr(lxyz), nl,
                                _ptr(blob), _PREC[prec], n, _ptr(out), _stream()), 'nfx_brdf_spec_fwd')
    return out


def brdf_sphere_fwd(xyz, normal, cam, z, lxyz, lweight, blob, out=None):
    """rgb[B, n, 3]: the BRDF prior of B latent codes z[B, z_dim] rendered at n sphere samples (xyz, normal [n, 3]) seen from
    `cam` (three numbers) under the lights lxyz[L, 3] with lweight[L, 3] = light * area: the sum over the lit front-facing
    lights of brdf * lweight * cos, accumulated in the kernel (nfx_brdf_sphere_fwd).  blob: pack_mlp128_weights(IN_Z_RUSINK).
    Every element of the result is written (`out`: a buffer to write into instead of a new one)."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    normal = _dev(normal, 'normal', (n, 3))
    z = _dev(z, 'z', (None, None))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    lweight = _dev(lweight, 'lweight', (nl, 3))
    cam3 = (ctypes.c_float * 3)(*[float(v) for v in (cam.tolist() if hasattr(cam, 'tolist') else cam)])
    if out is None:
        out = torch.empty((z.shape[0], n, 3), dtype=torch.float32, device=xyz.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (z.shape[0], n, 3):
        raise _capi.NfxError("brdf_sphere_fwd: `out` must be a contiguous CUDA float32 [%d, %d, 3] tensor" % (z.shape[0], n))
    check(lib.nfx_brdf_sphere_fwd(_ptr(xyz), _ptr(normal), n, ctypes.cast(cam3, ctypes.c_void_p), _ptr(z), z.shape[1], z.shape[0],
                                  _ptr(lxyz), _ptr(lweight), nl, _ptr(blob), _ptr(out), _stream()), 'nfx_brdf_sphere_fwd')
    return out


MERL_CELLS = 180 * 90 * 90


def _merl_table(table, who):
    table = _dev(table, 'table', (MERL_CELLS, 4))
    if table.data_ptr() % 16:
        raise _capi.NfxError("%s: the table must be 16-byte aligned" % who)
    return table


def merl_query(table, rusink, return_idx=False):
    """rgb[n, 3] (and idx[n] int32): the valid entry of a packed MERL table (float32 [180 * 90 * 90, 4], invalid entries -1:
    brdf.merl.MERL.device_table) nearest to each Rusinkiewicz coordinate rusink[n, 3] = (phi_d, theta_h, theta_d) in radians
    (nfx_merl_query).  A non-finite query gives idx -1 and rgb NaN."""
    table = _merl_table(table, 'merl_query')
    rusink = _dev(rusink, 'rusink', (None, 3))
    n = rusink.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=rusink.device)
    idx = torch.empty((n,), dtype=torch.int32, device=rusink.device) if return_idx else None
    check(lib.nfx_merl_query(_ptr(table), _ptr(rusink), n, _ptr(rgb), _ptr(idx), _stream()), 'nfx_merl_query')
    return (rgb, idx) if return_idx else rgb


def merl_sphere_fwd(xyz, normal, cam, table, lxyz, lweight, return_idx=False):
    """rgb[n, 3] (and idx[n, L] int32): a packed MERL table rendered at n sphere samples (xyz, normal [n, 3]) seen from `cam`
    (three numbers) under the lights lxyz[L, 3] with lweight[L, 3] = light * area: the sum over the lit front-facing lights of
    table[idx] * lweight * cos, accumulated in the kernel (nfx_merl_sphere_fwd).  idx is -1 where a row does not contribute."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    normal = _dev(normal, 'normal', (n, 3))
    table = _merl_table(table, 'merl_sphere_fwd')
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    lweight = _dev(lweight, 'lweight', (nl, 3))
    cam3 = (ctypes.c_float * 3)(*[float(v) for v in (cam.tolist() if hasattr(cam, 'tolist') else cam)])
    rgb = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    idx = torch.empty((n, nl), dtype=torch.int32, device=xyz.device) if return_idx else None
    check(lib.nfx_merl_sphere_fwd(_ptr(xyz), _ptr(normal), n, ctypes.cast(cam3, ctypes.c_void_p), _ptr(table), _ptr(lxyz),
                                  _ptr(lweight), nl, _ptr(rgb), _ptr(idx), _stream()), 'nfx_merl_sphere_fwd')
    return (rgb, idx) if return_idx else rgb


def mesh_bvh_build(vertices, faces, max_leaf=4):
    """uint8 host array: the BVH blob of a triangle mesh (nfx_mesh_bvh_build; layout in include/nfx.h).  Pure host code, no GPU
    needed.  vertices float32 [nv, 3], faces int32 [nf, 3]; a non-finite vertex or a face index out of range raises."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    f = np.ascontiguousarray(faces, dtype=np.int32)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise _capi.NfxError("mesh_bvh_build: vertices [nv, 3] and faces [nf, 3] are expected, got %s and %s" % (v.shape, f.shape))
    size = lib.nfx_mesh_bvh_bytes(f.shape[0], int(max_leaf))
    if size == 0:
        raise _capi.NfxError("mesh_bvh_build: %d triangles with max_leaf %d cannot be built" % (f.shape[0], max_leaf))
    blob = np.zeros(size // 16 + 1, dtype=np.complex128).view(np.uint8)[:size]     # 16-byte aligned
    check(lib.nfx_mesh_bvh_build(v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], int(max_leaf), blob.ctypes.data, size),
          'nfx_mesh_bvh_build')
    return blob


def _mesh_blob(blob, header, who):
    if not isinstance(blob, torch.Tensor) or not blob.is_cuda or blob.dtype != torch.uint8 or not blob.is_contiguous():
        raise _capi.NfxError("%s: the BVH blob must be a contiguous CUDA/ROCm uint8 tensor" % who)
    header = np.ascontiguousarray(header, dtype=np.uint8)
    if header.size != 32:
        raise _capi.NfxError("%s: the host header is the blob's first 32 bytes" % who)
    return blob, header


def mesh_cast(blob, header, rayo, rayd):
    """(t[n], tri[n] int32): the closest hit of every ray with the mesh of a BVH blob on the device (`header`: its first 32
    bytes on the host); t = +inf and tri = -1 for a miss, a zero direction or a non-finite ray (nfx_mesh_cast)."""
    blob, header = _mesh_blob(blob, header, 'mesh_cast')
    rayo = _dev(rayo, 'rayo', (None, 3))
    n = rayo.shape[0]
    rayd = _dev(rayd, 'rayd', (n, 3))
    t = torch.empty((n,), dtype=torch.float32, device=rayo.device)
    tri = torch.empty((n,), dtype=torch.int32, device=rayo.device)
    check(lib.nfx_mesh_cast(_ptr(blob), blob.numel(), header.ctypes.data, _ptr(rayo), _ptr(rayd), n, _ptr(t), _ptr(tri), _stream()),
          'nfx_mesh_cast')
    return t, tri


def mesh_lvis(blob, header, xyz, normal, alpha, lxyz, eps, out=None):
    """lvis[n, L]: alpha where the light is in front of the surface (normal . dir > 0) and the shadow ray from
    xyz + eps dir hits nothing, else 0; the rays are made in the kernel (nfx_mesh_lvis)."""
    blob, header = _mesh_blob(blob, header, 'mesh_lvis')
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    normal = _dev(normal, 'normal', (n, 3))
    alpha = _dev(alpha, 'alpha', (n,))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    if out is None:
        out = torch.empty((n, nl), dtype=torch.float32, device=xyz.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != (n, nl):
        raise _capi.NfxError("mesh_lvis: `out` must be a contiguous CUDA float32 [%d, %d] tensor" % (n, nl))
    check(lib.nfx_mesh_lvis(_ptr(blob), blob.numel(), header.ctypes.data, _ptr(xyz), _ptr(normal), _ptr(alpha), n, _ptr(lxyz), nl,
                            float(eps), _ptr(out), _stream()), 'nfx_mesh_lvis')
    return out


# ------------------------------------------------------------------------------ iso-surface
ISOSURFACE_MAX_POINTS = 1 << 31     # nfx.h: NFX_ISOSURFACE_MAX_POINTS


def isosurface_tables():
    """(tri int8 [6, 16, 2, 3, 2], edge int8 [6, 4, 4, 4]): the marching-tetrahedra tables of the kernels
    (nfx_isosurface_tables; layout in include/nfx.h).  Pure host code, no GPU needed."""
    tri, edge = np.zeros((6, 16, 2, 3, 2), dtype=np.int8), np.zeros((6, 4, 4, 4), dtype=np.int8)
    check(lib.nfx_isosurface_tables(tri.ctypes.data, edge.ctypes.data), 'nfx_isosurface_tables')
    return tri, edge


def _iso_field(field):
    if not isinstance(field, torch.Tensor) or not field.is_cuda:
        raise _capi.NfxError("isosurface: field must be a CUDA/ROCm tensor (libnfx has no CPU path)")
    if field.dtype != torch.float32:
        raise _capi.NfxError("isosurface: field must be float32, got %s" % field.dtype)
    if field.dim() != 3:
        raise _capi.NfxError("isosurface: field has shape %s, expected [nx, ny, nz]" % (tuple(field.shape),))
    if not field.is_contiguous():
        raise _capi.NfxError("isosurface: field must be contiguous (z fastest), strides %s of shape %s"
                             % (tuple(field.stride()), tuple(field.shape)))
    nx, ny, nz = (int(s) for s in field.shape)
    if min(nx, ny, nz) < 2:
        raise _capi.NfxError("isosurface: a %d x %d x %d lattice (at least 2 points per axis)" % (nx, ny, nz))
    if nx * ny * nz >= ISOSURFACE_MAX_POINTS:
        raise _capi.NfxError("isosurface: %d x %d x %d = %d lattice points (fewer than 2^31)" % (nx, ny, nz, nx * ny * nz))
    return nx, ny, nz


def _iso_workspace(ws, shape, device):
    nbytes = lib.nfx_isosurface_workspace_bytes(*shape)
    if ws is None:
        return torch.empty((nbytes // 4,), dtype=torch.int32, device=device)
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous() and ws.numel() * 4 >= nbytes):
        raise _capi.NfxError("isosurface: the workspace must be a contiguous CUDA int32 tensor of at least %d words" % (nbytes // 4))
    return ws


def isosurface_workspace(shape, device):
    """The int32 workspace of isosurface_count / isosurface_emit for a lattice of `shape` = (nx, ny, nz)."""
    return _iso_workspace(None, tuple(int(s) for s in shape), device)


def isosurface_count(field, iso, ws=None):
    """The workspace of a lattice, filled (nfx_isosurface_count; no host sync): ws[0] = vertices, ws[1] = triangles,
    ws[2] != 0 when a count does not fit int32."""
    shape = _iso_field(field)
    ws = _iso_workspace(ws, shape, field.device)
    check(lib.nfx_isosurface_count(_ptr(field), *shape, float(iso), _ptr(ws), ws.numel() * 4, _stream()), 'nfx_isosurface_count')
    return ws


def isosurface_emit(field, iso, origin, spacing, ws, nv, nf, vertices=None, faces=None):
    """(vertices[nv, 3] float32, faces[nf, 3] int32) from a counted workspace and its two totals (nfx_isosurface_emit)."""
    shape = _iso_field(field)
    ws = _iso_workspace(ws, shape, field.device)
    origin, spacing = [float(x) for x in origin], [float(x) for x in spacing]
    if len(origin) != 3 or len(spacing) != 3:
        raise _capi.NfxError("isosurface: origin and spacing are three numbers each")
    if not all(s > 0 and np.isfinite(s) for s in spacing):
        raise _capi.NfxError("isosurface: spacing = %s (finite, > 0 on every axis)" % (spacing,))
    if nv >= 2 ** 31 or 3 * nf >= 2 ** 31:
        raise _capi.NfxError("isosurface: nv = %d vertices, nf = %d triangles (nv < 2^31 and 3 nf = %d < 2^31)" % (nv, nf, 3 * nf))
    if vertices is None:
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=field.device)
    if faces is None:
        faces = torch.empty((nf, 3), dtype=torch.int32, device=field.device)
    for t, name, dt, n in ((vertices, 'vertices', torch.float32, nv), (faces, 'faces', torch.int32, nf)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (n, 3)):
            raise _capi.NfxError("isosurface: `%s` must be a contiguous CUDA %s [%d, 3] tensor" % (name, dt, n))
    check(lib.nfx_isosurface_emit(_ptr(field), *shape, float(iso), (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing),
                                  _ptr(ws), ws.numel() * 4, int(nv), int(nf), _ptr(vertices), _ptr(faces), _stream()),
          'nfx_isosurface_emit')
    return vertices, faces


def isosurface(field, iso, origin=(0., 0., 0.), spacing=(1., 1., 1.)):
    """(vertices[nv, 3] float32, faces[nf, 3] int32) on the device: the surface field = iso of float32 field[nx, ny, nz] by
    marching tetrahedra (include/nfx.h), inside where field > iso, normals pointing out of the inside; lattice point (a, b, c)
    sits at origin + (a, b, c) * spacing.  An empty surface gives shapes (0, 3).  One host read: the two totals, between the
    counting and the writing pass."""
    _iso_field(field)
    spacing = [float(x) for x in spacing]
    if len(spacing) != 3 or not all(s > 0 and np.isfinite(s) for s in spacing):
        raise _capi.NfxError("isosurface: spacing = %s (three numbers, finite, > 0 on every axis)" % (spacing,))
    if not np.isfinite(float(iso)):
        raise _capi.NfxError("isosurface: iso = %r is not finite" % (iso,))
    finite = all_finite(field)
    ws = isosurface_count(field, iso)
    nv, nf, overflow, bad = (int(x) for x in torch.cat((ws[:3], (~finite).to(torch.int32).reshape(1))).tolist())
    if bad:
        raise _capi.NfxError("isosurface: the %s field holds Inf or NaN" % (tuple(field.shape),))
    if overflow:
        raise _capi.NfxError("isosurface: the vertex or triangle count of this %s lattice passes 2^31 - 1 (nv < 2^31, 3 nf < 2^31)"
                             % (tuple(field.shape),))
    return isosurface_emit(field, iso, origin, spacing, ws, nv, nf)


# ------------------------------------------------------------------------------ mesh components
def mesh_components(faces, nv, label=None, ws=None):
    """label int32 [nv] on the device: per vertex the smallest vertex index of its connected component, two vertices being
    connected when a face names both (nfx_mesh_components; a vertex that no face names keeps its own index).  faces: a
    contiguous CUDA int32 [nf, 3] tensor.  A face index outside [0, nv) raises with the numbers BEFORE anything is launched
    (two reductions in torch); the kernel's own count of skipped faces is read back afterwards and raises too.  `label` and
    `ws` (int32, at least 4 words) may be passed in; what they hold does not matter.
    Vertices are NOT welded: a mesh stored as a triangle soup has one component per triangle (ops.isosurface meshes are
    indexed, every vertex once)."""
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda and faces.dtype == torch.int32 and faces.is_contiguous()
            and faces.dim() == 2 and faces.shape[1] == 3):
        raise _capi.NfxError("mesh_components: faces must be a contiguous CUDA/ROCm int32 [nf, 3] tensor (libnfx has no CPU path)")
    nv, nf = int(nv), int(faces.shape[0])
    nbytes = lib.nfx_mesh_components_workspace_bytes(nv, nf)
    if nbytes == 0:
        raise _capi.NfxError("mesh_components: nv = %d vertices, nf = %d triangles (0 <= nv < 2^31 and 0 <= 3 nf = %d < 2^31)"
                             % (nv, nf, 3 * nf))
    if nf:
        lo, hi = (int(x) for x in torch.stack((faces.amin(), faces.amax())).tolist())
        if lo < 0 or hi >= nv:
            raise _capi.NfxError("mesh_components: the faces name vertices %d .. %d, outside [0, %d)" % (lo, hi, nv))
    if label is None:
        label = torch.empty((nv,), dtype=torch.int32, device=faces.device)
    elif not (isinstance(label, torch.Tensor) and label.is_cuda and label.dtype == torch.int32 and label.is_contiguous()
              and tuple(label.shape) == (nv,)):
        raise _capi.NfxError("mesh_components: `label` must be a contiguous CUDA int32 [%d] tensor" % nv)
    if ws is None:
        ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=faces.device)
    elif not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous() and ws.numel() * 4 >= nbytes):
        raise _capi.NfxError("mesh_components: the workspace must be a contiguous CUDA int32 tensor of at least %d words" % (nbytes // 4))
    check(lib.nfx_mesh_components(_ptr(faces), nf, nv, _ptr(label), _ptr(ws), ws.numel() * 4, _stream()), 'nfx_mesh_components')
    skipped = int(ws[0])
    if skipped:
        raise _capi.NfxError("mesh_components: %d of %d faces name a vertex outside [0, %d) and were skipped" % (skipped, nf, nv))
    return label


def mesh_filter_components(vertices, faces, keep_largest=0, min_faces=0, attrs=()):
    """(vertices', faces', attrs', info) on the device: the mesh without the components that fail the filter — labelled by
    mesh_components, selected and re-indexed by mesh.filter_by_labels (its rules and its `info`).  vertices [nv, 3] and the
    per-vertex attrs [nv, k] are CUDA tensors, faces a contiguous CUDA int32 [nf, 3] tensor."""
    from . import mesh as nfx_mesh
    if not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dim() == 2):
        raise _capi.NfxError("mesh_filter_components: vertices must be a CUDA/ROCm [nv, 3] tensor")
    nfx_mesh.check_filter(keep_largest, min_faces)
    label = mesh_components(faces, vertices.shape[0])
    return nfx_mesh.filter_by_labels(vertices, faces, label, keep_largest, min_faces, attrs)


# ------------------------------------------------------------------------------ image metrics
IMAGE_METRICS_TILE = (16, 32)                    # (TY, TX): the window positions one block scores (NFX_IMAGE_METRICS_TILE_*)
IMAGE_METRICS_MAX_PIXELS = 1 << 22               # H * W of one image (NFX_IMAGE_METRICS_MAX_PIXELS)
IMAGE_METRICS_SCALE = 2 ** 40                    # the fixed point of the integer sums


def _ssim_weights():
    """tf.image.ssim's default window along one axis: 11 taps, sigma 1.5, normalised; Python floats (fp64)."""
    import math
    e = [math.exp(-0.5 * (((i - 5) / 1.5) * ((i - 5) / 1.5))) for i in range(11)]
    s = sum(e)
    return tuple(x / s for x in e)


IMAGE_METRICS_WEIGHTS = _ssim_weights()


def image_metrics_finalize(totals, n_map, max_val):
    """One image's numbers from its eight integers (include/nfx.h): {'mse', 'psnr', 'ssim', 'n_px'}.  Python integers and floats only, so that every step is one correctly rounded fp64 operation:
    mse = ((se_total / 2^40) / n_px) * max_val^2, psnr = 10 log10(max_val^2 / mse) (inf at mse = 0), ssim = (ssim_total /
    2^40) / n_map.  NaN for all three when the image's flag is raised, NaN for mse and psnr when no pixel was selected."""
    import math
    t = [int(x) for x in totals]
    se, sm, n_px, flag = t[0] + t[1] + t[2], t[3] + t[4] + t[5], t[6], t[7]
    nan = float('nan')
    out = {'mse': nan, 'psnr': nan, 'ssim': nan, 'n_px': n_px}
    if flag:
        return out
    out['ssim'] = float(sm) / float(IMAGE_METRICS_SCALE) / float(n_map)
    if n_px:
        peak = float(max_val) * float(max_val)
        out['mse'] = float(se) / float(IMAGE_METRICS_SCALE) / float(n_px) * peak
        out['psnr'] = float('inf') if se == 0 else 10. * math.log10(peak / out['mse'])
    return out


def image_metrics(a, b, max_val, luma=True, mask=None, return_map=False, totals=None, ws=None, ssim_map=None):
    """PSNR and SSIM of B image pairs in one call (nfx_image_metrics).  a, b: contiguous CUDA tensors [B, H, W, C] of the same
    shape, both uint8 or both float32, C = 1 or 3; max_val: 255 for uint8 content, 1 for unit-range floats.  luma (and C = 3):
    both images are reduced to L = (0.2126 r + 0.7152 g) + 0.0722 b first (xiuminglib's rgb2lum, as xm.metric.PSNR / SSIM
    do); otherwise the channels are scored separately and averaged (tf.image.ssim).  mask: uint8 [B, H, W], restricts the
    squared error (never the SSIM) to its non-zero pixels.
    -> {'mse', 'psnr', 'ssim': float64 [B] (host tensors; the call reads the B x 8 integer totals back once), 'n_px': int64
    [B] (pixel, channel) errors summed, 'totals': the int64 [B, 8] words of include/nfx.h on the host, 'ssim_map': float64
    [B, H - 10, W - 10, C'] on the device with return_map, else None}.  An image holding a NaN or an Inf gives NaN for that
    image; so does a pair with |a - b| > max_val somewhere (outside the declared range).  `totals`, `ws` (int64) and `ssim_map` may be passed in; what they hold does not matter."""
    for name, t in (('a', a), ('b', b)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise _capi.NfxError("image_metrics: %s must be a CUDA/ROCm tensor (libnfx has no CPU path)" % name)
    if a.dtype != b.dtype or a.dtype not in (torch.uint8, torch.float32):
        raise _capi.NfxError("image_metrics: a is %s and b is %s (both uint8 or both float32)" % (a.dtype, b.dtype))
    if a.shape != b.shape or a.dim() != 4:
        raise _capi.NfxError("image_metrics: a is %s and b is %s (the same [B, H, W, C])" % (tuple(a.shape), tuple(b.shape)))
    if not (a.is_contiguous() and b.is_contiguous()):
        raise _capi.NfxError("image_metrics: a and b must be contiguous")
    B, H, W, C = (int(x) for x in a.shape)
    max_val = float(max_val)
    if not (max_val > 0. and max_val < float('inf')):
        raise _capi.NfxError("image_metrics: max_val = %r (positive and finite)" % max_val)
    if H < 11 or W < 11:
        raise _capi.NfxError("image_metrics: images of %d x %d pixels, the 11 x 11 window needs at least 11 x 11" % (H, W))
    if C not in (1, 3):
        raise _capi.NfxError("image_metrics: C = %d channels (1 or 3)" % C)
    if H * W > IMAGE_METRICS_MAX_PIXELS:
        raise _capi.NfxError("image_metrics: %d x %d = %d pixels per image, at most %d" % (H, W, H * W, IMAGE_METRICS_MAX_PIXELS))
    luma = bool(luma)
    cp = 1 if (luma and C == 3) else C
    nbytes = lib.nfx_image_metrics_workspace_bytes(B, H, W, C, int(luma))
    if nbytes == 0:
        raise _capi.NfxError("image_metrics: B = %d images of %d scored channels (1 <= B, B * channels <= 65535)" % (B, cp))
    dev = a.device

    def buffer(t, name, dtype, shape):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise _capi.NfxError("image_metrics: `%s` must be a contiguous CUDA %s tensor of shape %s" % (name, dtype, tuple(shape)))
        return t

    if mask is not None:
        mask = buffer(mask, 'mask', torch.uint8, (B, H, W))
    if return_map or ssim_map is not None:
        ssim_map = buffer(ssim_map, 'ssim_map', torch.float64, (B, H - 10, W - 10, cp))
    totals = buffer(totals, 'totals', torch.int64, (B, 8))
    if ws is None:
        ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    elif not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.int64 and ws.is_contiguous() and ws.numel() * 8 >= nbytes):
        raise _capi.NfxError("image_metrics: the workspace must be a contiguous CUDA int64 tensor of at least %d words" % (nbytes // 8))
    g = (ctypes.c_double * 11)(*IMAGE_METRICS_WEIGHTS)
    check(lib.nfx_image_metrics(_ptr(a), _ptr(b), int(a.dtype == torch.float32), B, H, W, C, max_val, int(luma), _ptr(mask),
                                _ptr(ssim_map), ctypes.cast(g, ctypes.c_void_p), _ptr(totals), _ptr(ws), ws.numel() * 8, _stream()),
          'nfx_image_metrics')
    host = totals.cpu()
    rows = [image_metrics_finalize(r, (H - 10) * (W - 10) * cp, max_val) for r in host.tolist()]
    out = {k: torch.tensor([r[k] for r in rows], dtype=torch.float64) for k in ('mse', 'psnr', 'ssim')}
    out['n_px'] = torch.tensor([r['n_px'] for r in rows], dtype=torch.int64)
    out['totals'] = host
    out['ssim_map'] = ssim_map
    return out


# ------------------------------------------------------------------------- antialiased resize
RESIZE_MAX_TAPS = 33                             # NFX_RESIZE_MAX_TAPS: an axis shrinks by at most 16
RESIZE_MAX_CHANNELS = 4096                       # NFX_RESIZE_MAX_CHANNELS
_RESIZE_TYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}
_resize_tables = {}


def resize_axis_table(n_in, n_out):
    """One axis of tf.image.resize(bilinear, antialias=True) from the host function nfx_resize_axis_table (no GPU):
    (first int32 [n_out], count int32 [n_out], weights float32 [n_out, taps]) as NumPy arrays, taps = the largest count."""
    n_in, n_out = int(n_in), int(n_out)
    taps = lib.nfx_resize_axis_table(n_in, n_out, None, None, None, 0)
    if taps < 0:
        raise _capi.NfxError("nfx_resize_axis_table failed (%d): %s" % (taps, _capi.last_error()))
    first, count = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    weights = np.empty((n_out, taps), np.float32)
    rc = lib.nfx_resize_axis_table(n_in, n_out, first.ctypes.data_as(ctypes.c_void_p), count.ctypes.data_as(ctypes.c_void_p),
                                   weights.ctypes.data_as(ctypes.c_void_p), taps)
    if rc != taps:
        raise _capi.NfxError("nfx_resize_axis_table failed (%d): %s" % (rc, _capi.last_error()))
    return first, count, weights


def _resize_device_table(n_in, n_out, dev):
    key = (int(n_in), int(n_out), str(dev))
    if key not in _resize_tables:
        if len(_resize_tables) >= 64:
            _resize_tables.clear()
        _resize_tables[key] = tuple(torch.from_numpy(a).to(dev) for a in resize_axis_table(n_in, n_out))
    return _resize_tables[key]


def resize_antialias(x, new_h=None, new_w=None, out_uint8=False, out=None):
    """tf.image.resize(bilinear, antialias=True) of channels-last images on the GPU (nfx_resize_antialias; the arithmetic is
    stated in include/nfx.h).  x: contiguous CUDA tensor [B, H, W, C] or [H, W, C], uint8, uint16 or float32; integer
    values enter as float32(v) * (1 / 255) or (1 / 65535), the product rounded to float32.  When only one of new_h / new_w is
    given the other is int(h / w * new_w) / int(w / h * new_h) as in util.light.resize_antialias.  -> float32 of the same
    rank, or uint8 with out_uint8: (uint8)(clip(v, 0, 1) * 255), truncated.  The axis tables are built once per (n_in,
    n_out, device) by the host function and kept on the device; `out` may be passed in, what it holds does not matter."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise _capi.NfxError("resize_antialias: x must be a CUDA/ROCm tensor (libnfx has no CPU path)")
    if x.dtype not in _RESIZE_TYPES:
        raise _capi.NfxError("resize_antialias: x is %s (uint8, uint16 or float32)" % x.dtype)
    if x.dim() not in (3, 4):
        raise _capi.NfxError("resize_antialias: x is %s ([B, H, W, C] or [H, W, C])" % (tuple(x.shape),))
    if not x.is_contiguous():
        raise _capi.NfxError("resize_antialias: x must be contiguous")
    x4 = x if x.dim() == 4 else x[None]
    B, H, W, C = (int(v) for v in x4.shape)
    if min(B, H, W, C) < 1:
        raise _capi.NfxError("resize_antialias: x is %s, every size must be at least 1" % (tuple(x.shape),))
    if new_h is None and new_w is None:
        raise _capi.NfxError("resize_antialias: at least one of new_h and new_w must be given")
    if new_h is None:
        new_h = int(H / W * new_w)
    if new_w is None:
        new_w = int(W / H * new_h)
    new_h, new_w = int(new_h), int(new_w)
    if new_h < 1 or new_w < 1:
        raise _capi.NfxError("resize_antialias: %d x %d -> %d x %d pixels, every size must be at least 1" % (H, W, new_h, new_w))
    if H > 16 * new_h or W > 16 * new_w:
        raise _capi.NfxError("resize_antialias: %d x %d -> %d x %d shrinks an axis by more than 16 (more than %d taps)"
                             % (H, W, new_h, new_w, RESIZE_MAX_TAPS))
    if C > RESIZE_MAX_CHANNELS:
        raise _capi.NfxError("resize_antialias: C = %d channels (1 .. %d)" % (C, RESIZE_MAX_CHANNELS))
    out_dtype = torch.uint8 if out_uint8 else torch.float32
    shape = (B, new_h, new_w, C)
    if out is None:
        out4 = torch.empty(shape, dtype=out_dtype, device=x.device)
    else:
        want = shape if x.dim() == 4 else shape[1:]
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == out_dtype and out.is_contiguous() and tuple(out.shape) == want):
            raise _capi.NfxError("resize_antialias: `out` must be a contiguous CUDA %s tensor of shape %s" % (out_dtype, want))
        out4 = out
    fy, cy, wy = _resize_device_table(H, new_h, x.device)
    fx, cx, wx = _resize_device_table(W, new_w, x.device)
    in_scale = {torch.uint8: 1. / 255., torch.uint16: 1. / 65535., torch.float32: 1.}[x.dtype]
    check(lib.nfx_resize_antialias(_ptr(x4), _RESIZE_TYPES[x.dtype], B, H, W, C, in_scale, _ptr(fy), _ptr(cy), _ptr(wy), int(wy.shape[1]),
                                   _ptr(fx), _ptr(cx), _ptr(wx), int(wx.shape[1]), _ptr(out4), int(bool(out_uint8)), new_h, new_w,
                                   _stream()), 'nfx_resize_antialias')
    if out is not None:
        return out
    return out4 if x.dim() == 4 else out4[0]


def _shade_common(xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, lvis_row=None):
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    if rough is not None and rough.dim() == 2:
        rough = rough.reshape(-1)
    if lvis_row is not None and (not lvis_row.is_cuda or lvis_row.dtype != torch.int32 or not lvis_row.is_contiguous()
                                 or lvis_row.shape != (n,)):
        raise _capi.NfxError("shade: `lvis_row` must be a contiguous CUDA int32 [%d] tensor" % n)
    return (xyz, _dev(cam, 'cam', (n, 3)), _dev(normal, 'normal', (n, 3)),
            _dev(albedo, 'albedo', (n, 3)), _dev(rough, 'rough', (n,)), _dev(spec, 'spec', (n, nl)),
            _dev(lvis, 'lvis', (n if lvis_row is None else None, nl)), lxyz, _dev(lareas.reshape(-1), 'lareas', (nl,)), n, nl)


def shade_fwd(xyz, cam, normal, albedo, lvis, lxyz, lareas, lights, rough=None, spec=None,
              spec_scale=1., f0=0.04, linear2srgb=True, lvis_row=None):
    """rgb[n, P, 3] for P lights [P, L, 3] (microfacet BRDF if `rough`, else albedo/pi + spec).  `lvis_row` [n] int32: the
    visibilities of point i are row lvis_row[i] of `lvis` (a full-size buffer written by lvis_fwd(out=, out_row=))."""
    xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, n, nl = _shade_common(
        xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, lvis_row)
    row_p = None if lvis_row is None else ctypes.c_void_p(lvis_row.data_ptr())
    lights = _dev(lights, 'lights', (None, nl, 3))
    p_total = lights.shape[0]
    out = torch.empty((n, p_total, 3), dtype=torch.float32, device=xyz.device)
    # all probes of one call must fit the LDS together; split if they do not
    p_max = p_total
    while p_max > 1 and lib.nfx_shade_lds_bytes(nl, p_max) > 160 * 1024:
        p_max -= 1
    for p0 in range(0, p_total, p_max):
        chunk = lights[p0:p0 + p_max].contiguous()
        dst = out if p_max == p_total else torch.empty((n, chunk.shape[0], 3), dtype=torch.float32,
                                                      device=xyz.device)
        check(lib.nfx_shade_fwd_rows(_ptr(xyz), _ptr(cam), _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(spec),
                                     spec_scale, f0, _ptr(lvis), row_p, _ptr(lxyz), _ptr(lareas), _ptr(chunk), n, nl,
                                     chunk.shape[0], int(linear2srgb), _ptr(dst), _stream()), 'nfx_shade_fwd')
        if dst is not out:
            out[:, p0:p0 + chunk.shape[0]] = dst
    return out


def shade_olat_fwd(xyz, cam, normal, albedo, lvis, lxyz, lareas, olat_inten, ambient, rough=None,
                   spec=None, spec_scale=1., f0=0.04, linear2srgb=True, lvis_row=None, out=None, out_row=None, nan_flag=None):
    """rgb_olat[n, L, 3]: one-light-at-a-time relighting (`lvis_row`: as in shade_fwd).  `out` [n_all, L, 3] + `out_row` [n]
    int32: the renders of point i go to out[out_row[i]] (the caller zeroes the other rows); `nan_flag` int32[1]: raised when a
    radiance is NaN before the clip."""
    xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, n, nl = _shade_common(
        xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, lvis_row)
    if out_row is not None:
        if out is None or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape[1:]) != (nl, 3):
            raise _capi.NfxError("shade_olat_fwd: `out` must be a contiguous CUDA float32 [n_all, %d, 3] tensor" % nl)
        if not out_row.is_cuda or out_row.dtype != torch.int32 or not out_row.is_contiguous() or out_row.shape != (n,):
            raise _capi.NfxError("shade_olat_fwd: `out_row` must be a contiguous CUDA int32 [%d] tensor" % n)
    else:
        out = torch.empty((n, nl, 3), dtype=torch.float32, device=xyz.device)
    as_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    check(lib.nfx_shade_olat_fwd_rows(_ptr(xyz), _ptr(cam), _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(spec),
                                      spec_scale, f0, _ptr(lvis), as_p(lvis_row), _ptr(lxyz), _ptr(lareas), olat_inten, ambient,
                                      n, nl, int(linear2srgb), as_p(out_row), _ptr(out), as_p(nan_flag), _stream()),
          'nfx_shade_olat_fwd')
    return out


def brdf_rows_geom_fwd(xyz, cam, normal, z, lxyz, n_freqs):
    """(rows [n L, z_dim + 3 + 6 n_freqs], front [n L]) of the learned BRDF in fp32: rows = [z | embed(rusink)] per (point,
    light), front = 1.0 where the light is in front of the surface (nerfactor.py:413-436)."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    cam, normal = _dev(cam, 'cam', (n, 3)), _dev(normal, 'normal', (n, 3))
    z = _dev(z, 'z', (n, None))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl, zd = lxyz.shape[0], z.shape[1]
    rows = torch.empty((n * nl, zd + 3 + 6 * n_freqs), dtype=torch.float32, device=xyz.device)
    front = torch.empty((n * nl,), dtype=torch.float32, device=xyz.device)
    check(lib.nfx_brdf_rows_geom_fwd(_ptr(xyz), _ptr(cam), _ptr(normal), _ptr(z), zd, _ptr(lxyz), nl, n, n_freqs, _ptr(rows),
                                     rows.shape[1], _ptr(front), _stream()), 'nfx_brdf_rows_geom_fwd')
    return rows, front


def brdf_rows_geom_bwd(xyz, cam, normal, z_dim, lxyz, n_freqs, d_rows):
    """(d_normal [n, 3], d_z [n, z_dim]) from dLoss/d rows of brdf_rows_geom_fwd, summed over each point's front-lit lights."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    cam, normal = _dev(cam, 'cam', (n, 3)), _dev(normal, 'normal', (n, 3))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    d_rows = _dev(d_rows, 'd_rows', (n * nl, z_dim + 3 + 6 * n_freqs))
    d_normal = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    d_z = torch.empty((n, z_dim), dtype=torch.float32, device=xyz.device)
    check(lib.nfx_brdf_rows_geom_bwd(_ptr(xyz), _ptr(cam), _ptr(normal), z_dim, _ptr(lxyz), nl, n, n_freqs, _ptr(d_rows),
                                     d_rows.shape[1], _ptr(d_normal), _ptr(d_z), _stream()), 'nfx_brdf_rows_geom_bwd')
    return d_normal, d_z


def dir2rusink(a, b):
    a = _dev(a, 'a', (None, 3))
    b = _dev(b, 'b', (a.shape[0], 3))
    out = torch.empty_like(a)
    check(lib.nfx_dir2rusink(_ptr(a), _ptr(b), a.shape[0], _ptr(out), _stream()), 'nfx_dir2rusink')
    return out


# ---------------------------------------------------------------------------- training ops
def pack_mlp128_train_weights(kernels, biases, in_kind, out_dim, prec='bf16'):
    """Train blob (forward + dgrad fragments) of a width-128 surface MLP, for mlp128_bwd."""
    if len(kernels) != 5 or len(biases) != 5:
        raise _capi.NfxError("pack_mlp128_train_weights: need 5 kernels and 5 biases")
    return _pack(lambda k, o, p: lib.nfx_mlp128_train_packed_bytes(k), lib.nfx_mlp128_pack_train_weights,
                 kernels, biases, (in_kind, out_dim, _PREC[prec]))


def mlp128_bwd(in_kind, xyz, dout, blob, dkernels, dbiases, out_act=None, xyz_scale=1., post_scale=1.,
               lxyz=None, xyz_dir=None, prec='bf16'):
    """Accumulate the weight gradients of one width-128 MLP call into `dkernels` / `dbiases`
    (lists of 5 fp32 CUDA tensors, Keras layout) given dout = dLoss/d(output)."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    nl = 0
    if in_kind == _capi.IN_XYZ_LDIR:
        lxyz = _dev(lxyz, 'lxyz', (None, 3))
        nl = lxyz.shape[0]
    rows = n if in_kind == _capi.IN_XYZ else n * nl
    dout = _dev(dout.reshape(rows, -1), 'dout', (rows, None))
    out_dim = dout.shape[1]
    xyz_dir = _dev(xyz_dir, 'xyz_dir', (n, 3))
    for t in list(dkernels) + list(dbiases):
        _dev(t, 'gradient buffer')
    ws_bytes = lib.nfx_mlp128_bwd_workspace_bytes(in_kind, n, nl)
    ws = torch.empty((max(ws_bytes, 16) // 2,), dtype=torch.bfloat16, device=xyz.device)
    karr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in dkernels])
    barr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in dbiases])
    check(lib.nfx_mlp128_bwd(in_kind, _ptr(xyz), _ptr(xyz_dir), n, xyz_scale, _ptr(lxyz), nl, _ptr(blob),
                             out_dim, _ACT[out_act], post_scale, _ptr(dout), _ptr(ws), ws.numel() * 2, karr,
                             barr, _PREC[prec], _stream()), 'nfx_mlp128_bwd')
    return ws



MLP128_MAX_HEADS = 4


def mlp128_bwd_heads(in_kind, xyz, heads, xyz_scale=1., lxyz=None, xyz_dir=None, prec='bf16'):
    """mlp128_bwd for up to MLP128_MAX_HEADS networks over the SAME rows in one launch pair (nfx_mlp128_bwd_heads).
    heads: [(dout, train_blob, dkernels, dbiases, out_act, post_scale), ...]; bit-identical to one mlp128_bwd per head."""
    if not 1 <= len(heads) <= MLP128_MAX_HEADS:
        raise _capi.NfxError("mlp128_bwd_heads: 1 .. %d heads" % MLP128_MAX_HEADS)
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    nl = 0
    if in_kind == _capi.IN_XYZ_LDIR:
        lxyz = _dev(lxyz, 'lxyz', (None, 3))
        nl = lxyz.shape[0]
    rows = n if in_kind == _capi.IN_XYZ else n * nl
    xyz_dir = _dev(xyz_dir, 'xyz_dir', (n, 3))
    douts, keep = [], []
    for dout, blob, dks, dbs, _, _ in heads:
        douts.append(_dev(dout.reshape(rows, -1), 'dout', (rows, None)))
        for t in list(dks) + list(dbs):
            _dev(t, 'gradient buffer')
        if len(dks) != 5 or len(dbs) != 5:
            raise _capi.NfxError("mlp128_bwd_heads: 5 kernel and 5 bias gradient buffers per head")
    nh = len(heads)
    ws_bytes = lib.nfx_mlp128_bwd_workspace_bytes(in_kind, n, nl) * nh
    ws = torch.empty((max(ws_bytes, 16) // 2,), dtype=torch.bfloat16, device=xyz.device)
    blobs = (ctypes.c_void_p * nh)(*[h[1].data_ptr() for h in heads])
    darr = (ctypes.c_void_p * nh)(*[d.data_ptr() for d in douts])
    dims = (ctypes.c_int * nh)(*[d.shape[1] for d in douts])
    acts = (ctypes.c_int * nh)(*[_ACT[h[4]] for h in heads])
    scales = (ctypes.c_float * nh)(*[float(h[5]) for h in heads])
    karr = (ctypes.c_void_p * (5 * nh))(*[t.data_ptr() for h in heads for t in h[2]])
    barr = (ctypes.c_void_p * (5 * nh))(*[t.data_ptr() for h in heads for t in h[3]])
    check(lib.nfx_mlp128_bwd_heads(in_kind, _ptr(xyz), _ptr(xyz_dir), n, xyz_scale, _ptr(lxyz), nl, nh, blobs, dims, acts, scales,
                                   darr, _ptr(ws), ws.numel() * 2, karr, barr, _PREC[prec], _stream()), 'nfx_mlp128_bwd_heads')
    return ws


# ------------------------------------------------------------------------------ NeRF training ops
def pack_nerf_train_weights(kernels, biases, prec='bf16'):
    """Train blob (forward + dgrad fragments) of one NeRF network, for nerf_mlp_bwd."""
    if len(kernels) != 12 or len(biases) != 12:
        raise _capi.NfxError("pack_nerf_train_weights: need 12 kernels and 12 biases")
    return _pack(lib.nfx_nerf_train_packed_bytes, lib.nfx_nerf_pack_train_weights, kernels, biases, (_PREC[prec],))


def composite_bwd(rgbs, z, rayd, d_rgb, white_bg=True, noise=None):
    """d_rgbs[N,S,4] = dLoss/d rgbs given d_rgb[N,3] = dLoss/d (composited rgb)."""
    rgbs = _dev(rgbs, 'rgbs', (None, None, 4))
    n, s = rgbs.shape[:2]
    z = _dev(z, 'z', (n, s))
    rayd = _dev(rayd, 'rayd', (n, 3))
    noise = _dev(noise, 'noise', (n, s))
    d_rgb = _dev(d_rgb, 'd_rgb', (n, 3))
    out = torch.empty_like(rgbs)
    check(lib.nfx_composite_bwd(_ptr(rgbs), _ptr(z), _ptr(rayd), _ptr(noise), n, s, int(white_bg), _ptr(d_rgb),
                                _ptr(out), _stream()), 'nfx_composite_bwd')
    return out


NERF_BWD_MAX_POINTS = 1 << 19   # ~5 GB of feature-major workspace per call; more rays are processed in slices


NERF_BWD_STATS = None   # a list: nerf_mlp_bwd appends (points with a gradient [device int32 copy], points) per call (bench.py)


def nerf_bwd_list_words(n_pts):
    """Word offsets of (count, per-1024-point counts, indices) and the total of the row list at the END of the workspace
    of nfx_nerf_mlp_bwd (nerf_bwd.hip:nfx_nerf_bwd_list_bytes)."""
    nb = (n_pts + 1023) // 1024
    b0 = 4 + (nb + 3) // 4 * 4
    return 0, 4, b0, b0 + (n_pts + 3) // 4 * 4


def nerf_mlp_bwd(rayo, rayd, z, d_rgbs, blob, dkernels, dbiases, prec='bf16'):
    """Accumulate the weight gradients of one nerf_mlp_fwd call into `dkernels` / `dbiases` (lists of 12 fp32
    CUDA tensors, Keras layout) given d_rgbs[N,S,4].  Only the points whose d_rgbs is not four zeros are differentiated
    (the library builds their list on the device; option nerf_bwd_rows = 0: every point)."""
    rayo = _dev(rayo, 'rayo', (None, 3))
    n = rayo.shape[0]
    rayd = _dev(rayd, 'rayd', (n, 3))
    z = _dev(z, 'z', (n, None))
    s = z.shape[1]
    d_rgbs = _dev(d_rgbs, 'd_rgbs', (n, s, 4))
    for t in list(dkernels) + list(dbiases):
        _dev(t, 'gradient buffer')
    karr = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in dkernels])
    barr = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in dbiases])
    rays_per_call = max(1, NERF_BWD_MAX_POINTS // s)
    ws = None
    for lo in range(0, n, rays_per_call):
        hi = min(n, lo + rays_per_call)
        ws_bytes = lib.nfx_nerf_bwd_workspace_bytes(hi - lo, s)
        if ws is None or ws.numel() * 2 < ws_bytes:
            ws = torch.empty((max(ws_bytes, 16) // 2,), dtype=torch.bfloat16, device=z.device)
        check(lib.nfx_nerf_mlp_bwd(_ptr(rayo[lo:hi]), _ptr(rayd[lo:hi]), _ptr(z[lo:hi]), hi - lo, s, _ptr(blob),
                                   _PREC[prec], _ptr(d_rgbs[lo:hi]), _ptr(ws), ws.numel() * 2, karr, barr,
                                   _stream()), 'nfx_nerf_mlp_bwd')
        if NERF_BWD_STATS is not None:
            first = ws_bytes // 4 - nerf_bwd_list_words((hi - lo) * s)[3]
            NERF_BWD_STATS.append((ws.view(torch.int32)[first:first + 1].clone(), (hi - lo) * s))
    return ws


# ------------------------------------------------------------------------------ geometry extraction ops
def pack_nerf_geom_weights(kernels, biases, prec='bf16'):
    """Blob of nerf_sigma_grad: encoder + sigma tile, transposed encoder, input-gradient tiles."""
    if len(kernels) != 12 or len(biases) != 12:
        raise _capi.NfxError("pack_nerf_geom_weights: need 12 kernels and 12 biases")
    return _pack(lib.nfx_nerf_geom_packed_bytes, lib.nfx_nerf_pack_geom_weights, kernels, biases, (_PREC[prec],))


def _ray_args(rayo, rayd, z, blob):
    rayo = _dev(rayo, 'rayo', (None, 3))
    n = rayo.shape[0]
    rayd = _dev(rayd, 'rayd', (n, 3))
    z = _dev(z, 'z', (n, None))
    if not blob.is_cuda or blob.dtype != torch.uint8:
        raise _capi.NfxError("blob must be a CUDA uint8 tensor")
    return rayo, rayd, z, n, z.shape[1]


def nerf_sigma_fwd(rayo, rayd, z, blob, prec='bf16'):
    """sigma_raw[N,S] (no relu) at rayo + rayd*z from the GEOM blob (pack_nerf_geom_weights); the rgb head is neither
    evaluated nor streamed."""
    rayo, rayd, z, n, s = _ray_args(rayo, rayd, z, blob)
    out = torch.empty((n, s), dtype=torch.float32, device=z.device)
    check(lib.nfx_nerf_sigma_fwd(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(blob), _PREC[prec], _ptr(out),
                                 _stream()), 'nfx_nerf_sigma_fwd')
    return out


def nerf_refine_last_sample(rayo, rayd, z, rgbs, geom_blob_fp32):
    """Overwrites the density of every ray's LAST sample in rgbs[N,S,4] (in place) with the fp32-class density kernel's
    value (nfx_nerf_sigma_refine_last: one launch, the kernel reads z[:, -1] and writes rgbs[:, -1, 3] itself; the bits of
    nerf_sigma_fwd(..., 'fp32') there).  That sample gets dist = 1e10 when compositing
    (nerf.py:186-191): alpha_last = [sigma_last > 0] exactly, so its SIGN is the only bit of the ray that a bf16 kernel
    can get wrong by a whole pixel value; 1 / S of the points at ~3x the cost."""
    n, s = z.shape
    if n == 0 or s < 2:
        return rgbs
    if not (isinstance(rgbs, torch.Tensor) and rgbs.is_contiguous()):
        raise _capi.NfxError("nerf_refine_last_sample: rgbs is updated in place and must be contiguous")
    rayo, rayd, z, n, s = _ray_args(rayo, rayd, z, geom_blob_fp32)
    check(lib.nfx_nerf_sigma_refine_last(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(geom_blob_fp32),
                                         _ptr(_dev(rgbs, 'rgbs', (n, s, 4))), _stream()), 'nfx_nerf_sigma_refine_last')
    return rgbs


# The selection of nfx_nerf_refine_select as the render uses it, calibrated on all 640 000 rays of a view of a fitted NeRF
# against the fp32-class render (scripts/coarse_refine_residual.py, profiles/r06/coarse_refine_residual*.json): 2195 rays above
# 3e-2 with the plain bf16 coarse pass; 0 (max 1.6e-2 = the fp32-class coarse pass's own figure) with T > 1e-2, alpha in
# (1e-2, 0.99), no dilation, |sigma| < 0.3 — 6.9 % of the coarse samples — and with every wider rule; 767 with alpha in
# (0.05, 0.95); 27 without the |sigma| rule however wide the rest.  Shipped: one notch wider than the cheapest rule that held.
REFINE_T_MIN, REFINE_A_LO, REFINE_A_HI, REFINE_DILATE = 1e-3, 1e-3, 0.999, 0
REFINE_MARGIN_FACTOR = 2.       # sigma_margin = factor x the measured 99.9 % quantile of |sigma_bf16 - sigma_fp32class|


def nerf_refine_coarse(rayo, rayd, z, rgbs, geom_blob_fp32, t_min=REFINE_T_MIN, a_lo=REFINE_A_LO, a_hi=REFINE_A_HI,
                       dilate=REFINE_DILATE, sigma_margin=0., want_count=False):
    """Overwrites, in place, the density in rgbs[N,S,4] of the coarse samples that decide where the inverse-CDF sampler
    (util/math.py:71-94) puts the fine samples with the fp32-class density kernel's value: samples that are visible
    (T_i > t_min) and either not saturated (a_lo < alpha_i < a_hi) or undecided (|sigma_i| < sigma_margin: which side of
    the relu the sample is on lies within the bf16 kernel's error — on a near-miss ray, whose weights sum to almost nothing,
    one such sample is the whole pdf), and `dilate` neighbours either way.  Two launches
    (nfx_nerf_refine_select, nfx_nerf_sigma_refine); the list and its length stay on the device.  Returns rgbs (and the
    1-element int32 count tensor if `want_count`)."""
    rayo, rayd, z, n, s = _ray_args(rayo, rayd, z, geom_blob_fp32)
    if not (isinstance(rgbs, torch.Tensor) and rgbs.is_contiguous()):
        raise _capi.NfxError("nerf_refine_coarse: rgbs is updated in place and must be contiguous")
    rgbs = _dev(rgbs, 'rgbs', (n, s, 4))
    count = torch.empty(1, dtype=torch.int32, device=z.device)
    if n == 0 or s < 2:
        count.zero_()
        return (rgbs, count) if want_count else rgbs
    lst = torch.empty(n * s, dtype=torch.int32, device=z.device)
    check(lib.nfx_nerf_refine_select(_ptr(rgbs), _ptr(z), _ptr(rayd), n, s, t_min, a_lo, a_hi, sigma_margin, dilate, _ptr(lst), _ptr(count),
                                     _stream()), 'nfx_nerf_refine_select')
    check(lib.nfx_nerf_sigma_refine(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(geom_blob_fp32), _ptr(lst), _ptr(count),
                                    _ptr(rgbs), _stream()), 'nfx_nerf_sigma_refine')
    return (rgbs, count) if want_count else rgbs


def nerf_coarse_error(rayo, rayd, z, rgbs, geom_blob_fp32, max_rays=4096, q=0.999, geom_blob_bf16=None):
    """(alpha_error, sigma_error) of the bf16 coarse pass for THESE weights: sigma_error = the q-quantile of
    |sigma_bf16 - sigma_fp32class| over the samples of up to `max_rays` rays of the batch; alpha_error = that times the mean
    sample spacing = how far the bf16 error can move a sample's alpha.  The render's `coarse_precision = auto` measures this
    once per weight version (one host read): the selective refinement is on when alpha_error exceeds `coarse_refine_gate`
    (measured: glorot "opaque" weights of the bench 1.5e-3, a NeRF fitted to a scene 1.0e-2), and sigma_error sizes the
    |sigma| < margin rule of nerf_refine_coarse.  `rgbs` = the bf16 pass's output for these rays, or None: then the bf16
    densities of the picked rays come from the bf16 density kernel (`geom_blob_bf16`; bit-identical to the MLP kernel's sigma)."""
    n = min(int(z.shape[0]), max_rays)
    if n == 0 or z.shape[1] < 2:
        return 0., 0.
    step = max(1, int(z.shape[0]) // n)
    pick = slice(0, n * step, step)
    o, d, zz = rayo[pick].contiguous(), rayd[pick].contiguous(), z[pick].contiguous()
    s32 = nerf_sigma_fwd(o, d, zz, geom_blob_fp32, 'fp32')
    s16 = rgbs[pick][..., 3] if rgbs is not None else nerf_sigma_fwd(o, d, zz, geom_blob_bf16, 'bf16')
    err = (s16 - s32).abs()[:, :-1].reshape(-1)
    spacing = ((zz[:, 1:] - zz[:, :-1]).mean() * d.norm(dim=1).mean())
    sig = torch.quantile(err[:4000000], q)
    both = torch.stack((sig * spacing, sig)).tolist()
    return float(both[0]), float(both[1])


SIGMA_GRAD_STATS = None   # a list: nerf_sigma_grad appends (samples with a density [device int32 copy], samples) per call (bench.py)


def nerf_sigma_grad(rayo, rayd, z, geom_blob, prec='bf16'):
    """(normal[N,S,3], sigma_raw[N,S]) with normal = -l2_normalize(d relu(sigma)/dx)."""
    rayo, rayd, z, n, s = _ray_args(rayo, rayd, z, geom_blob)
    out = torch.empty((n, s, 4), dtype=torch.float32, device=z.device)
    if _capi.get_option("sigma_grad_rows") != 0 and n * s < 2 ** 31:
        # the reverse sweep only over the samples with a positive density (every other sample's normal is zero: relu has no
        # slope there) — the same values, and most samples of a fitted scene are empty space
        ws_bytes = lib.nfx_nerf_sigma_grad_workspace_bytes(n, s)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=z.device)
        check(lib.nfx_nerf_sigma_grad_rows(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(geom_blob), _PREC[prec], _ptr(out),
                                           _ptr(ws), ws.numel(), _stream()), 'nfx_nerf_sigma_grad_rows')
        if SIGMA_GRAD_STATS is not None:
            first = (n * s * 4 + 15) // 16 * 4
            SIGMA_GRAD_STATS.append((ws.view(torch.int32)[first:first + 1].clone(), n * s))
    else:
        check(lib.nfx_nerf_sigma_grad(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(geom_blob), _PREC[prec], _ptr(out),
                                      _stream()), 'nfx_nerf_sigma_grad')
    return out[..., :3], out[..., 3]


# ------------------------------------------------------------------------------ occupancy grid
OCCGRID_MAX_RES, OCCGRID_MAX_PROBES = 1024, 1 << 30     # nfx.h: NFX_OCCGRID_MAX_RES, NFX_OCCGRID_MAX_PROBES


def _box6(box, name):
    box = [float(x) for x in box]
    if len(box) != 6:
        raise _capi.NfxError("%s: (x_min, x_max, y_min, y_max, z_min, z_max)" % name)
    return (ctypes.c_float * 6)(*box)


def occgrid_workspace(n_rays, n_samples, device):
    """The int32 workspace of occgrid_select for n_rays x n_samples samples."""
    nbytes = lib.nfx_occgrid_workspace_bytes(n_rays, n_samples)
    return torch.empty((max(nbytes, 16) // 4,), dtype=torch.int32, device=device)


def occgrid_list(ws, n_pts):
    """(list[n_pts], count[1]) views of an occgrid_select workspace: the ascending flat sample indices and their number
    (list[count:] is not written)."""
    first = 4 + ((n_pts + 1023) // 1024 + 3) // 4 * 4
    return ws[first:first + n_pts], ws[:1]


def occgrid_select(rayo, rayd, z, bits, res, box, bbox=None, out=None, ws=None):
    """(out[N, S], list, count): lists the samples rayo + rayd z that lie outside the grid's box or in a set cell of
    `bits` (int32 [ceil(res^3 / 32)], nfx.h's layout) and inside the optional scene bbox, and writes 0.0 to `out` at every
    other sample.  The list stays on the device."""
    rayo = _dev(rayo, 'rayo', (None, 3))
    n = rayo.shape[0]
    rayd = _dev(rayd, 'rayd', (n, 3))
    z = _dev(z, 'z', (n, None))
    s = z.shape[1]
    if not (bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and bits.numel() == (res ** 3 + 31) // 32):
        raise _capi.NfxError("occgrid_select: bits must be a contiguous CUDA int32 tensor of ceil(res^3 / 32) words")
    if out is None:
        out = torch.empty((n, s), dtype=torch.float32, device=z.device)
    if ws is None:
        ws = occgrid_workspace(n, s, z.device)
    lst, count = occgrid_list(ws, n * s)
    if n == 0:
        count.zero_()
        return out, lst, count
    check(lib.nfx_occgrid_select(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(bits), int(res), _box6(box, 'box'),
                                 None if bbox is None else _box6(bbox, 'bbox'), _ptr(out), _ptr(ws), ws.numel() * 4,
                                 _stream()), 'nfx_occgrid_select')
    return out, lst, count


def nerf_sigma_fwd_list(rayo, rayd, z, blob, lst, count, out, prec='bf16'):
    """out[N, S] at the flat sample indices lst[0 .. count[0]) = nerf_sigma_fwd's values there (in place; every other
    sample is left alone).  The count is read on the device."""
    rayo, rayd, z, n, s = _ray_args(rayo, rayd, z, blob)
    out = _dev(out, 'out', (n, s))
    for t, name in ((lst, 'list'), (count, 'count')):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise _capi.NfxError("nerf_sigma_fwd_list: %s must be a contiguous CUDA int32 tensor" % name)
    check(lib.nfx_nerf_sigma_fwd_list(_ptr(rayo), _ptr(rayd), _ptr(z), n, s, _ptr(blob), _PREC[prec], _ptr(lst),
                                      _ptr(count), _ptr(out), _stream()), 'nfx_nerf_sigma_fwd_list')
    return out


def nerf_sigma_fwd_grid(rayo, rayd, z, blob, bits, res, box, bbox=None, prec='bf16'):
    """(sigma_raw[N, S], count[1]): nerf_sigma_fwd evaluated only at the samples occgrid_select lists, 0.0 at the others;
    count = how many were evaluated (int32, on the device)."""
    out, lst, count = occgrid_select(rayo, rayd, z, bits, res, box, bbox)
    nerf_sigma_fwd_list(rayo, rayd, z, blob, lst, count, out, prec)
    return out, count


def occgrid_bake(probe_sigma, res, probes, margin=0., dilate=1):
    """The grid's bits (int32 [ceil(res^3 / 32)]) from the raw densities of the (res probes)^3 probe lattice (nfx.h:
    nfx_occgrid_bake): a cell is occupied when a probe has sigma_raw > -margin, then dilated by `dilate` cells."""
    m = res * probes
    if not (1 <= res <= OCCGRID_MAX_RES and 1 <= probes <= 16 and m ** 3 <= OCCGRID_MAX_PROBES and 0 <= dilate <= 16):
        raise _capi.NfxError("occgrid_bake: res = %d, probes = %d, dilate = %d (1 <= res <= %d, 1 <= probes <= 16, "
                             "(res probes)^3 <= %d, 0 <= dilate <= 16)" % (res, probes, dilate, OCCGRID_MAX_RES,
                                                                         OCCGRID_MAX_PROBES))
    probe_sigma = _dev(probe_sigma, 'probe_sigma')
    if probe_sigma.numel() != m ** 3:
        raise _capi.NfxError("occgrid_bake: %d probe densities, expected (res probes)^3 = %d" % (probe_sigma.numel(), m ** 3))
    bits = torch.empty(((res ** 3 + 31) // 32,), dtype=torch.int32, device=probe_sigma.device)
    ws = torch.empty_like(bits)
    check(lib.nfx_occgrid_bake(_ptr(probe_sigma), int(res), int(probes), float(margin), int(dilate), _ptr(bits), _ptr(ws),
                               _stream()), 'nfx_occgrid_bake')
    return bits


def amsgrad_step(p, g, m, v, vhat, lr, step, beta1=0.9, beta2=0.999, eps=1e-7):
    """In-place Keras Adam(amsgrad=True) update of the flat fp32 buffer `p` (step is 1-based)."""
    for t in (p, g, m, v, vhat):
        _dev(t, 'optimizer buffer')
    check(lib.nfx_amsgrad_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(vhat), p.numel(), lr, beta1, beta2,
                               eps, step, _stream()), 'nfx_amsgrad_step')


def amsgrad_step_size(lr, step, beta1=0.9, beta2=0.999):
    """lr_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step), evaluated as the library does (double, rounded once)."""
    return float(lib.nfx_amsgrad_step_size(lr, beta1, beta2, step))


def amsgrad_step_dev(p, g, m, v, vhat, lr_t_dev, beta1=0.9, beta2=0.999, eps=1e-7):
    """amsgrad_step with the step size read from the 1-element CUDA tensor `lr_t_dev` (hipGraph-replayable)."""
    for t in (p, g, m, v, vhat, lr_t_dev):
        _dev(t, 'optimizer buffer')
    check(lib.nfx_amsgrad_step_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(vhat), p.numel(), _ptr(lr_t_dev), beta1,
                                   beta2, eps, _stream()), 'nfx_amsgrad_step_dev')


def shade_bwd(xyz, cam, normal, albedo, lvis, lxyz, lareas, light, drgb, d_light, rough=None, spec=None,
              spec_scale=1., f0=0.04, linear2srgb=True):
    """Backward of shade_fwd for one light [L,3].  Returns (d_albedo, d_normal, d_lvis, d_rough|d_spec);
    adds the light's gradient to d_light [L,3] (order-independent fixed-point sum: bit-reproducible)."""
    xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas, n, nl = _shade_common(
        xyz, cam, normal, albedo, rough, spec, lvis, lxyz, lareas)
    light = _dev(light, 'light', (nl, 3))
    drgb = _dev(drgb, 'drgb', (n, 3))
    d_light = _dev(d_light, 'd_light', (nl, 3))
    dev_ = xyz.device
    d_albedo = torch.empty((n, 3), dtype=torch.float32, device=dev_)
    d_normal = torch.empty((n, 3), dtype=torch.float32, device=dev_)
    d_lvis = torch.empty((n, nl), dtype=torch.float32, device=dev_)
    d_rough = torch.empty((n,), dtype=torch.float32, device=dev_) if spec is None else None
    d_spec = torch.empty((n, nl), dtype=torch.float32, device=dev_) if spec is not None else None
    ws = torch.empty((max(lib.nfx_shade_bwd_workspace_bytes(nl), 8) // 8,), dtype=torch.int64, device=dev_)
    check(lib.nfx_shade_bwd(_ptr(xyz), _ptr(cam), _ptr(normal), _ptr(albedo), _ptr(rough), _ptr(spec), spec_scale,
                            f0, _ptr(lvis), _ptr(lxyz), _ptr(lareas), _ptr(light), n, nl, int(linear2srgb),
                            _ptr(drgb), _ptr(d_albedo), _ptr(d_rough), _ptr(d_spec), _ptr(d_normal), _ptr(d_lvis),
                            _ptr(d_light), _ptr(ws), ws.numel() * 8, _stream()), 'nfx_shade_bwd')
    return d_albedo, d_normal, d_lvis, (d_rough if spec is None else d_spec)


def pack_brdf_train_weights(kernels, biases, z_dim, prec='bf16'):
    """Train blob of the (frozen) learned-BRDF MLP: forward + dgrad + input-gradient fragments."""
    return _pack(lambda zd, p: lib.nfx_brdf_train_packed_bytes(), lib.nfx_brdf_pack_train_weights, kernels,
                 biases, (z_dim, _PREC[prec]))


def brdf_spec_bwd(xyz, cam, normal, z, lxyz, blob, dspec, prec='bf16'):
    """(d_z [n, z_dim], d_normal [n, 3]) from dspec [n, L] through the frozen BRDF prior."""
    xyz = _dev(xyz, 'xyz', (None, 3))
    n = xyz.shape[0]
    z = _dev(z, 'z', (n, None))
    lxyz = _dev(lxyz, 'lxyz', (None, 3))
    nl = lxyz.shape[0]
    dspec = _dev(dspec, 'dspec', (n, nl))
    d_z = torch.zeros_like(z)
    d_normal = torch.zeros((n, 3), dtype=torch.float32, device=xyz.device)
    ws = torch.empty((max(lib.nfx_brdf_spec_bwd_workspace_bytes(z.shape[1], n), 8) // 8,), dtype=torch.int64,
                     device=xyz.device)
    # round 6: only the rows with a non-zero upstream gradient are re-computed and differentiated (the shading backward zeroes
    # d spec of every back-facing light: half of the rows); option brdf_bwd_rows = 0 keeps every row (same bits)
    list_bytes = lib.nfx_brdf_spec_bwd_list_bytes(n, nl) if _capi.get_option("brdf_bwd_rows") != 0 else 0
    lws = torch.empty((list_bytes // 4,), dtype=torch.int32, device=xyz.device) if list_bytes else None
    check(lib.nfx_brdf_spec_bwd_rows(_ptr(xyz), _ptr(_dev(cam, 'cam', (n, 3))), _ptr(_dev(normal, 'normal', (n, 3))),
                                     _ptr(z), z.shape[1], _ptr(lxyz), nl, _ptr(blob), _PREC[prec], n, _ptr(dspec),
                                     _ptr(d_z), _ptr(d_normal), _ptr(ws), ws.numel() * 8,
                                     None if lws is None else ctypes.c_void_p(lws.data_ptr()), list_bytes, _stream()),
          'nfx_brdf_spec_bwd')
    return d_z, d_normal


def brdf_rows_fwd(z, rusink, blob, reci=True, prec='bf16'):
    """The BRDF prior on explicit rows: out[n] (reci=False) or out[2n] (rows n.. = the same inputs at phi_d + pi) =
    softplus(out(mlp([z, posenc2(rusink)]))).  `blob` = pack_brdf_train_weights(...)."""
    z = _dev(z, 'z', (None, None))
    n = z.shape[0]
    rusink = _dev(rusink, 'rusink', (n, 3))
    out = torch.empty(((2 if reci else 1) * n,), dtype=torch.float32, device=z.device)
    check(lib.nfx_brdf_rows_fwd(_ptr(z), z.shape[1], _ptr(rusink), n, int(bool(reci)), _ptr(blob), _PREC[prec],
                                _ptr(out), _stream()), 'nfx_brdf_rows_fwd')
    return out


def brdf_rows_bwd(z, rusink, blob, dout, dkernels, dbiases, reci=True, prec='bf16'):
    """d_z[rows, z_dim] (per row: sum the two halves for the gradient of z[n]) from dout[rows]; ACCUMULATES the weight
    gradients into `dkernels` / `dbiases` (5 fp32 CUDA tensors each, Keras layout)."""
    z = _dev(z, 'z', (None, None))
    n, zd = z.shape
    rows = (2 if reci else 1) * n
    rusink = _dev(rusink, 'rusink', (n, 3))
    dout = _dev(dout.reshape(rows), 'dout', (rows,))
    for t in list(dkernels) + list(dbiases):
        _dev(t, 'gradient buffer')
    d_z = torch.empty((rows, zd), dtype=torch.float32, device=z.device)
    ws_bytes = lib.nfx_brdf_rows_bwd_workspace_bytes(zd, n, int(bool(reci)))
    ws = torch.empty((max(ws_bytes, 16) // 2,), dtype=torch.bfloat16, device=z.device)
    karr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in dkernels])
    barr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in dbiases])
    check(lib.nfx_brdf_rows_bwd(_ptr(z), zd, _ptr(rusink), n, int(bool(reci)), _ptr(blob), _PREC[prec], _ptr(dout),
                                _ptr(ws), ws.numel() * 2, _ptr(d_z), karr, barr, _stream()), 'nfx_brdf_rows_bwd')
    return d_z


# ------------------------------------------------------------------------------ fused per-ray losses
class _LossTerm(ctypes.Structure):   # include/nfx.h: nfx_loss_term
    _fields_ = [('a', ctypes.c_void_p), ('b', ctypes.c_void_p), ('ga', ctypes.c_void_p), ('gb', ctypes.c_void_p),
                ('d', ctypes.c_int), ('w', ctypes.c_float), ('kind', ctypes.c_int), ('flags', ctypes.c_int)]


LOSS_KIND = {'mse': 0, 'mae': 1}
LOSS_BLEND_A, LOSS_BLEND_B, LOSS_ACCUM_A, LOSS_ACCUM_B = 1, 2, 4, 8


def _loss_table(terms, grads=None):
    """terms: [(a, b, weight, kind, blend_a, blend_b)]; grads: per term (ga, gb, accum_a, accum_b) or None."""
    if not 1 <= len(terms) <= 8:
        raise _capi.NfxError("pair_loss: 1..8 terms")
    n = terms[0][0].shape[0]
    table = (_LossTerm * len(terms))()
    for i, (a, b, w, kind, blend_a, blend_b) in enumerate(terms):
        a = _dev(a, 'loss operand', (n, None))
        b = _dev(b, 'loss operand', (n, a.shape[1]))
        flags = (LOSS_BLEND_A if blend_a else 0) | (LOSS_BLEND_B if blend_b else 0)
        ga = gb = None
        if grads is not None:
            ga, gb, acc_a, acc_b = grads[i]
            flags |= (LOSS_ACCUM_A if acc_a else 0) | (LOSS_ACCUM_B if acc_b else 0)
        table[i] = _LossTerm(a.data_ptr(), b.data_ptr(), ga.data_ptr() if ga is not None else None,
                             gb.data_ptr() if gb is not None else None, a.shape[1], float(w), LOSS_KIND[kind], flags)
    return table, n


def pair_loss_fwd(terms, alpha=None, bg=0.):
    """loss[n] = sum_t w_t mean_d f_t(A_t - B_t) with optional alpha blending of A / B onto `bg` (nfx.h)."""
    table, n = _loss_table(terms)
    dev = terms[0][0].device
    alpha = None if alpha is None else _dev(alpha.reshape(n), 'alpha', (n,))
    loss = torch.empty((n,), dtype=torch.float32, device=dev)
    check(lib.nfx_pair_loss_fwd(table, len(terms), _ptr(alpha), float(bg), n, _ptr(loss), _stream()),
          'nfx_pair_loss_fwd')
    return loss


def pair_loss_bwd(terms, grads, dloss, alpha=None, bg=0.):
    """Writes / accumulates d loss / d A, d loss / d B into the buffers of `grads` (see _loss_table)."""
    table, n = _loss_table(terms, grads)
    alpha = None if alpha is None else _dev(alpha.reshape(n), 'alpha', (n,))
    dloss = _dev(dloss.reshape(n), 'dloss', (n,))
    check(lib.nfx_pair_loss_bwd(table, len(terms), _ptr(alpha), float(bg), n, _ptr(dloss), _stream()),
          'nfx_pair_loss_bwd')
