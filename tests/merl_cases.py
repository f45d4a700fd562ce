"""Synthetic MERL tables and the query sets of the measured-BRDF tests (host only, no GPU, no reference).

No MERL file ships with the repository, so every table is made here.  synthetic_cube uses IEEE-exact operations only
(+ - * / sqrt on the integer indices, integer hashing for the holes): every machine makes the same bits, which is what lets
tests/golden/reference_merl.npz store the reference's answers for tables and queries that are rebuilt at test time."""
import numpy as np

SHAPE = (180, 90, 90)
N_CELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
HALF_PI = np.pi / 2
HOLE_ONE_IN = 500          # 0.2 % of the entries are measurement holes


def _hash32(x, salt):
    """Integer hash of uint64 values into [0, 2^32): multiply / xor-shift rounds on exact integers."""
    x = (np.asarray(x, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(30)
    x = (x * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(27)
    x = (x * np.uint64(0x94D049BB133111EB)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(31)
    return x >> np.uint64(32)


def uniform01(n, salt):
    """[n] float64 in [0, 1), exact: a 32-bit integer hash of the row number divided by 2^32."""
    with np.errstate(over='ignore'):
        return _hash32(np.arange(n), salt).astype(np.float64) / 4294967296.0


def synthetic_cube(seed):
    """[180, 90, 90, 3] float64: a diffuse floor plus a rational lobe in theta_h, tinted per channel and modulated by a
    polynomial in theta_d; the block below the horizon (theta_h + theta_d |1 - 2 phi_d / pi| > pi / 2, in index arithmetic)
    and one entry in 500 (a hash of its flat index) are -1.  Every valid entry is > 0."""
    i, j, k = np.meshgrid(np.arange(SHAPE[0], dtype=np.float64), np.arange(SHAPE[1], dtype=np.float64),
                          np.arange(SHAPE[2], dtype=np.float64), indexing='ij')
    th_n = ((j + 0.105) / SHAPE[1]) * ((j + 0.105) / SHAPE[1])       # theta_h / (pi / 2)
    td_n = k / (SHAPE[2] - 1)                                          # theta_d / (pi / 2)
    ph_n = np.abs(1.0 - 2.0 * i / (SHAPE[0] - 1))
    w = (3.0 + (seed % 7)) / 100.0                                     # lobe width, as a fraction of pi / 2
    t = th_n / w
    lobe = 1.0 / ((1.0 + t * t) * (1.0 + t * t))
    fres = 1.0 + 2.0 * td_n * td_n * td_n * td_n                       # brighter towards grazing
    tint = np.array((1.0, 0.8 + (seed % 3) / 10.0, 0.6 + (seed % 5) / 10.0))
    floor = np.array((0.05 + (seed % 4) / 50.0, 0.08, 0.03 + (seed % 2) / 20.0))
    cube = floor[None, None, None, :] * (1.0 + ph_n[..., None] / 8.0) + (4.0 * lobe * fres)[..., None] * tint[None, None, None, :]
    horizon = th_n + td_n * ph_n > 1.0
    with np.errstate(over='ignore'):
        hole = (_hash32(np.arange(N_CELLS), 1000 + seed) % np.uint64(HOLE_ONE_IN) == 0).reshape(SHAPE)
    cube[horizon | hole] = -1.0
    return cube


def grid_rusink(flat):
    """Flat cube indices -> float64 [n, 3] Rusinkiewicz coordinates (brdf.merl.merl_to_rusink)."""
    flat = np.asarray(flat, dtype=np.int64)
    i, j, k = flat // (SHAPE[1] * SHAPE[2]), (flat // SHAPE[2]) % SHAPE[1], flat % SHAPE[2]
    return np.stack((i / (SHAPE[0] - 1) * np.pi, np.square((j + 0.105) / SHAPE[1]) * HALF_PI, k / (SHAPE[2] - 1) * HALF_PI), axis=1)


def cslice_queries():
    """[8100, 3] float32: the grid points of the characteristic slice (phi_d index 90), theta_h-major."""
    j, k = np.meshgrid(np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing='ij')
    flat = (90 * SHAPE[1] + j.reshape(-1)) * SHAPE[2] + k.reshape(-1)
    return grid_rusink(flat).astype(np.float32), flat.astype(np.int64)


def uniform_queries(n=4096, salt=11):
    """[n, 3] float32 uniform over [0, pi] x [0, pi / 2]^2."""
    return np.stack((uniform01(n, salt) * np.pi, uniform01(n, salt + 1) * HALF_PI, uniform01(n, salt + 2) * HALF_PI), axis=1).astype(np.float32)


def outside_queries(per_side=256, salt=23):
    """[6 per_side, 3] float32: for each of the cube's six sides, queries up to 0.3 rad beyond it and uniform in the other two."""
    out = []
    hi = (np.pi, HALF_PI, HALF_PI)
    for side in range(6):
        ax, upper = side >> 1, side & 1
        q = np.stack([uniform01(per_side, salt + 10 * side + a) * hi[a] for a in range(3)], axis=1)
        beyond = 1e-3 + 0.3 * uniform01(per_side, salt + 10 * side + 5)
        q[:, ax] = hi[ax] + beyond if upper else -beyond
        out.append(q)
    return np.concatenate(out, 0).astype(np.float32)


def query_sets(scene_rusink_f32):
    """name -> float32 [n, 3]; `scene_rusink_f32`: reference_sphere.npz['a_rusink'], the front-lit rows of scene (16, 1)."""
    return {'cslice': cslice_queries()[0], 'uniform': uniform_queries(), 'outside': outside_queries(),
            'scene': np.asarray(scene_rusink_f32, dtype=np.float32)}


def nearest_cell(q):
    """Flat index of the per-axis nearest cell of float64 queries [n, 3] (no validity): what the fast path answers."""
    q = np.asarray(q, dtype=np.float64)
    i = np.clip(np.rint(q[:, 0] / np.pi * (SHAPE[0] - 1)), 0, SHAPE[0] - 1).astype(np.int64)
    k = np.clip(np.rint(q[:, 2] / HALF_PI * (SHAPE[2] - 1)), 0, SHAPE[2] - 1).astype(np.int64)
    gh = np.square((np.arange(SHAPE[1]) + 0.105) / SHAPE[1]) * HALF_PI
    j = np.abs(q[:, 1:2] - gh[None, :]).argmin(1)
    return (i * SHAPE[1] + j) * SHAPE[2] + k
