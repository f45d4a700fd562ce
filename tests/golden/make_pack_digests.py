"""Writes tests/golden/pack_digests.json: SHA-256 digests of every blob the six tuned-network weight packers of libnfx
produce (nfx_nerf_pack_weights, nfx_nerf_pack_train_weights, nfx_nerf_pack_geom_weights, nfx_mlp128_pack_weights,
nfx_mlp128_pack_train_weights, nfx_brdf_pack_train_weights), so that a change to the packers that is meant to leave the
layouts alone can be held to "every blob byte unchanged" on a machine without a GPU (tests/test_cpu_pack_golden.py).

    python -m tests.golden.make_pack_digests [label]

The digests are those of the library that nerfactor_amd._capi loads: the tree's, or with NFX_LIB_PATH=... the library of
another checkout (`python -m nerfactor_amd.build --out ...`).  Regenerate the file from the library of the commit BEFORE a
packer change, never from the changed one; `label` (that commit's hash) is recorded in the file.

Every packer is called through the C-ABI with ctypes, into an exactly-sized buffer, twice: once pre-filled with 0x00 and
once with 0xA5.  The two digests together pin which bytes a packer writes, which it leaves to the caller, and their
values.  Beside each SHA-256 the file keeps the CRC-32 of every KiB of the blob (one weight fragment = 1 KiB), so that a
mismatch can be traced to a fragment — a layer — and not just to a hash.

Inputs: kernels and biases from a counter-based integer hash (no dependence on a library's random streams), uniform in
[-1, 1) with all 24 significand bits in use.  Every kernel also carries, at fixed positions, the values that exercise
f32_to_bf16_rne and the residual W - bf16(W) of the fp32-class blobs: -0.0, a subnormal, two values exactly halfway
between two bf16 numbers (one rounds down to even, one up), +inf, and a quiet and a signalling NaN."""
import base64
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'pack_digests.json')
FILLS = (('00', 0x00), ('a5', 0xA5))
IN_XYZ, IN_XYZ_LDIR, IN_Z_RUSINK = 0, 1, 2
BF16, FP32 = 0, 1
NERF_SHAPES = [(63, 256)] + [(256, 256)] * 4 + [(319, 256)] + [(256, 256)] * 2 + [(256, 1), (256, 256), (283, 128), (128, 3)]
# -0.0 | subnormal | 1 + 2^-8: halfway, even below | 1 + 3 * 2^-8: halfway, even above | +inf | quiet NaN | signalling NaN
SPECIAL_BITS = (0x80000000, 0x00012345, 0x3F808000, 0x3F818000, 0x7F800000, 0x7FC00001, 0x7F800001)


def _m128_shapes(in_dims, out_dim):
    return [(in_dims, 128), (128, 128), (128, 128), (128 + in_dims, 128), (128, out_dim)]


def cases():
    """[(name, size function, its arguments, pack function, its arguments between biases and blob, kernel shapes)]"""
    out = []
    for p, prec in ((BF16, 'bf16'), (FP32, 'fp32')):
        out.append(('nerf_' + prec, 'nfx_nerf_packed_bytes', (p,), 'nfx_nerf_pack_weights', (p,), NERF_SHAPES))
        out.append(('nerf_geom_' + prec, 'nfx_nerf_geom_packed_bytes', (p,), 'nfx_nerf_pack_geom_weights', (p,), NERF_SHAPES))
    out.append(('nerf_train_bf16', 'nfx_nerf_train_packed_bytes', (BF16,), 'nfx_nerf_pack_train_weights', (BF16,), NERF_SHAPES))
    for kind, kname, ind in ((IN_XYZ, 'xyz', 63), (IN_XYZ_LDIR, 'xyz_ldir', 90)):
        for od in (1, 3, 8):
            for p, prec in ((BF16, 'bf16'), (FP32, 'fp32')):
                out.append(('mlp128_%s_out%d_%s' % (kname, od, prec), 'nfx_mlp128_packed_bytes', (kind, 0, od, p),
                            'nfx_mlp128_pack_weights', (kind, 0, od, p), _m128_shapes(ind, od)))
            out.append(('mlp128_train_%s_out%d' % (kname, od), 'nfx_mlp128_train_packed_bytes', (kind,),
                        'nfx_mlp128_pack_train_weights', (kind, od, BF16), _m128_shapes(ind, od)))
    for zd in (1, 2, 3, 9):
        for p, prec in ((BF16, 'bf16'), (FP32, 'fp32')):
            out.append(('mlp128_brdf_z%d_%s' % (zd, prec), 'nfx_mlp128_packed_bytes', (IN_Z_RUSINK, zd, 1, p),
                        'nfx_mlp128_pack_weights', (IN_Z_RUSINK, zd, 1, p), _m128_shapes(zd + 15, 1)))
        out.append(('brdf_train_z%d' % zd, 'nfx_brdf_train_packed_bytes', (), 'nfx_brdf_pack_train_weights', (zd, BF16),
                    _m128_shapes(zd + 15, 1)))
    return out


def _uniform(seed, n):
    """n floats in [-1, 1), a function of (seed, index) alone: splitmix64's finaliser over a counter."""
    with np.errstate(over='ignore'):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return ((x >> np.uint64(40)).astype(np.float32) * np.float32(2. ** -23) - np.float32(1.)).astype(np.float32)


def inputs(name, shapes):
    """-> (kernels, biases) of one case: float32, C-contiguous; the special values at SPECIAL positions of every kernel."""
    seed = zlib.crc32(name.encode()) << 8
    kernels, biases = [], []
    for i, (rows, cols) in enumerate(shapes):
        k = _uniform(seed + 2 * i, rows * cols)
        for j, bits in enumerate(SPECIAL_BITS):     # spread evenly over the kernel (the smallest has 128 entries)
            k.view(np.uint32)[(j * rows * cols) // len(SPECIAL_BITS) + j] = bits
        kernels.append(k.reshape(rows, cols))
        biases.append(_uniform(seed + 2 * i + 1, cols))
    return kernels, biases


def _pointers(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def pack(capi, case, fill):
    """The blob of one case as a uint8 array: packed through the C-ABI into an exactly-sized buffer pre-filled with `fill`."""
    name, size_fn, size_args, pack_fn, pack_args, shapes = case
    kernels, biases = inputs(name, shapes)
    nbytes = getattr(capi.lib, size_fn)(*size_args)
    assert nbytes > 0, name
    blob = np.full(nbytes, fill, np.uint8)
    capi.check(getattr(capi.lib, pack_fn)(_pointers(kernels), _pointers(biases), *pack_args, blob.ctypes.data, nbytes), name)
    return blob


def kib_crcs(blob):
    return np.array([zlib.crc32(blob[o:o + 1024].tobytes()) for o in range(0, blob.size, 1024)], np.uint32)


def digest(blob):
    return {'bytes': int(blob.size), 'sha256': hashlib.sha256(blob.tobytes()).hexdigest(),
            'kib_crc32': base64.b64encode(kib_crcs(blob).astype('<u4').tobytes()).decode()}


def first_difference(blob, want):
    """-> (index of the first KiB of blob whose CRC-32 is not the recorded one, or None; recorded size)."""
    crcs = np.frombuffer(base64.b64decode(want['kib_crc32']), '<u4')
    got = kib_crcs(blob)
    n = min(got.size, crcs.size)
    bad = np.flatnonzero(got[:n] != crcs[:n])
    return (int(bad[0]) if bad.size else (n if got.size != crcs.size else None)), want['bytes']


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from nerfactor_amd import _capi
    out = {'library': sys.argv[1] if len(sys.argv) > 1 else 'unlabelled', 'cases': {}}
    for case in cases():
        out['cases'][case[0]] = {tag: digest(pack(_capi, case, fill)) for tag, fill in FILLS}
    with open(OUT, 'w') as h:
        json.dump(out, h, indent=1, sort_keys=True)
        h.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes,', len(out['cases']), 'cases, library', _capi.LIB_PATH)


if __name__ == '__main__':
    main()
