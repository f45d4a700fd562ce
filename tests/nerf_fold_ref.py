"""NumPy restatements of the bottleneck fold of the NeRF render path (csrc/nerf_fold.hip, csrc/nerf_fold_layout.hpp) — test
infrastructure beside emu.py:
  fold_weights / fold_bias   the arithmetic, on logical [in, out] matrices (fp32 running sums in ascending m)
  eval_folded                the folded network on points, nerf_ref.bf16_round at the kernel's rounding points
  fold_blob                  the render blob, fragment by fragment, from a packed blob — what the device kernel must write
  nerf_tile_folded           lane-level walk of a render blob (the 70-tile kernels' dataflow), on emu.py's MFMA model"""
import numpy as np

from oracle import nerf_ref
from oracle.nerf_ref import bf16_round

from . import emu

N_FRAGS, N_BIAS = 1272, 2496                      # packed blob (nerf_layout.hpp)
BIAS_BOTT, BIAS_RGB0, BIAS_RGB1 = 2048, 2336, 2464
N_FRAGS_R = N_FRAGS - 128                         # render blob: the bottleneck's 8 x 16 fragments are gone


def chunk_frags(k):
    return 8 if k < 8 else 16 if k < 40 else 24 if k < 48 else 16 if k < 73 else 24 if k < 77 else 8


def chunk_off(k):
    return sum(chunk_frags(i) for i in range(k))


def src_chunk(k):
    """chunk of the packed blob behind render chunk k (70 chunks: encoder, sigma, 4 x rgb_out[0], rgb_out[1])"""
    return k if k < 64 else k + 8


def chunk_off_r(k):
    return sum(chunk_frags(src_chunk(i)) for i in range(k))


def hidden_feature(s, h, j):
    """input feature behind k-step s, lane half h, element j of a hidden layer's fragment (pack.hpp)"""
    return 16 * s + (j & 3) + 8 * (j >> 2) + 4 * h


def fold_weights(wb, w0a):
    """W'[k][c] = sum over m ascending of wb[k][m] * w0a[m][c], a plain fp32 running sum from 0 (the operands are bf16
    values, every product is exact in fp32).  Not rounded here."""
    wb, w0a = np.asarray(wb, np.float32), np.asarray(w0a, np.float32)
    acc = np.zeros((wb.shape[0], w0a.shape[1]), np.float32)
    for m in range(wb.shape[1]):
        acc = acc + wb[:, m:m + 1] * w0a[m:m + 1, :]
    return acc


def fold_bias(bb, w0a, b0):
    """b0'[c] = (sum over m ascending of fl(bb[m] * w0a[m][c])) + b0[c]: fp32 multiply, then fp32 add"""
    bb, w0a = np.asarray(bb, np.float32), np.asarray(w0a, np.float32)
    acc = np.zeros(w0a.shape[1], np.float32)
    for m in range(bb.shape[0]):
        acc = acc + bb[m] * w0a[m]
    return acc + np.asarray(b0, np.float32)


def eval_folded(pts, views, net, fold_from_fp32=False):
    """The folded network, pts / views [N, S, 3] -> [N, S, 4] — eval_nerf_at(quant=bf16_round) with the bottleneck and
    rgb_out[0] replaced by one layer.  fold_from_fp32: fold the fp32 weights instead of the bf16 ones of the blob."""
    q = bf16_round
    depth = len(net['enc'])
    pe = nerf_ref.embed(pts.reshape(-1, 3), 10)
    ve = nerf_ref.embed(views.reshape(-1, 3), 4)
    feat = nerf_ref.mlp(pe, net['enc'], ['relu'] * depth, skip_at=[depth // 2], quant=q)
    sigma = nerf_ref.mlp(feat, net['sigma_out'], [None], quant=q)
    (wb, bb), (w0, b0) = net['bottleneck'][0], net['rgb_out'][0]
    if fold_from_fp32:
        wf, bf = q((wb.astype(np.float64) @ w0[:256].astype(np.float64)).astype(np.float32)), \
            (bb.astype(np.float64) @ w0[:256].astype(np.float64) + b0).astype(np.float32)
    else:
        wf, bf = q(fold_weights(q(wb), q(w0[:256]))), fold_bias(bb, q(w0[:256]), b0)
    layer0 = (np.concatenate((wf, w0[256:]), 0), bf)
    rgb = nerf_ref.mlp(np.concatenate((feat, ve), -1), [layer0, net['rgb_out'][1]], ['relu', None], quant=q)
    return np.concatenate([rgb, sigma], -1).reshape(pts.shape[:2] + (4,))


def _bits(x):
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def fold_blob(blob):
    """packed bf16 blob (uint8 [1272 KiB + 2496 x 4]) -> render blob (uint8), walking the fragments as csrc/nerf_fold.hip is
    specified to: folded tile u, fragment s, lane (h, n), element j = bf16(W'[F(s, h, j)][32 u + n]) with
    Wb[F(s, h, j)][m] read from bottleneck chunk m >> 5, fragment s, lane (h, m & 31), element j and W0a[m][c] from
    rgb_out[0] chunk c >> 5, fragment m >> 4, lane (hm, c & 31), element jm where F(m >> 4, hm, jm) = m."""
    blob = np.ascontiguousarray(np.asarray(blob, np.uint8))
    assert blob.nbytes == N_FRAGS * 1024 + N_BIAS * 4
    w = blob[:N_FRAGS * 1024].view(np.uint16).reshape(N_FRAGS, 64, 8)
    fl = blob[N_FRAGS * 1024:].view(np.float32)
    f32 = emu.bf16_bits_to_f32
    bott = f32(w[chunk_off(64):chunk_off(72)]).reshape(8, 16, 2, 32, 8)             # [t, s, h, n, j]
    wb = bott.transpose(1, 2, 4, 0, 3).reshape(16, 2, 8, 256)                       # [s, h, j, m = 32 t + n]
    rgb0 = f32(w[chunk_off(73):chunk_off(77)]).reshape(4, 24, 2, 32, 8)             # [u, frag, h, n, j]
    w0a = np.zeros((256, 4, 32), np.float32)                                        # [m, u, n]
    for sm in range(16):
        for hm in range(2):
            for jm in range(8):
                w0a[hidden_feature(sm, hm, jm)] = rgb0[:, sm, hm, :, jm]
    acc = fold_weights(wb.reshape(-1, 256), w0a.reshape(256, 128)).reshape(16, 2, 8, 4, 32)   # [s, h, j, u, n]
    folded = _bits(acc).transpose(3, 0, 1, 4, 2).reshape(4, 16, 64, 8)              # [u, s, lane, j]
    out_w = np.zeros((N_FRAGS_R, 64, 8), np.uint16)
    for k in range(70):
        src, n = src_chunk(k), chunk_frags(src_chunk(k))
        out_w[chunk_off_r(k):chunk_off_r(k) + n] = w[chunk_off(src):chunk_off(src) + n]
        if 65 <= k < 69:
            out_w[chunk_off_r(k):chunk_off_r(k) + 16] = folded[k - 65]
    out_f = fl.copy()
    out_f[BIAS_RGB0:BIAS_RGB0 + 128] = fold_bias(fl[BIAS_BOTT:BIAS_BOTT + 256], w0a.reshape(256, 128),
                                                 fl[BIAS_RGB0:BIAS_RGB0 + 128])
    return np.concatenate([out_w.reshape(-1).view(np.uint8), out_f.view(np.uint8)])


def nerf_tile_folded(render_blob, pts, views):
    """pts, views [32, 3] -> raw [32, 4], the 70-tile walk of the folded kernels over a render blob: enc[7]'s output feeds
    the sigma tile AND the folded rgb_out[0]."""
    rd = emu.BlobReader(np.asarray(render_blob), N_FRAGS_R * 1024)
    bias = rd.b
    pe = emu.posenc_slots(pts.astype(np.float32), 10)
    pv = emu.posenc_slots(views.astype(np.float32), 4)
    h = emu.layer(rd, 8, bias, 0, pe, 8, True)
    for l in range(1, 8):
        h = emu.layer(rd, 24, bias, 256 * l, h + pe, 8, True) if l == 5 else emu.layer(rd, 16, bias, 256 * l, h, 8, True)
    sigma = emu.tile(rd, 16, bias, BIAS_BOTT + 256, h)[:32, 0]
    r0 = emu.layer(rd, 24, bias, BIAS_RGB0, h + pv, 4, True)
    acc = emu.tile(rd, 8, bias, BIAS_RGB1, r0)
    assert rd.pos == N_FRAGS_R
    return np.stack([acc[:32, 0], acc[:32, 1], acc[:32, 2], sigma], -1)
