"""Rays, shape lists and NumPy references for the ray-march stages of csrc/raymarch.hip (gen_z, composite, composite_bwd,
sample_fine) at the shapes where their loops change course.  No GPU: tests/test_cpu_raymarch_cases.py checks the cases and
the room every tolerance leaves, tests/test_gpu_raymarch_edges.py holds the kernels to the references.

What the kernels branch on:
  * composite / composite_bwd walk a ray in chunks of 64 samples (one per lane) and carry the running product from chunk
    to chunk: S = 63 / 64 / 65, 128 / 129, 200, 257 put a whole, an empty-but-one and a partly filled last chunk behind
    one, two and four full ones; S = 1 and 2 are the shortest rays (the last sample's interval is 1e10);
  * composite_bwd opts in to more than 64 KiB of LDS above S = 2048 (32 S bytes per workgroup; the API stops at 4096);
  * every kernel gives a workgroup four rays, one per wave: n = 1, 2, 3, 5 leave waves of the last workgroup idle;
  * sample_fine sums its n_coarse - 2 pdf bins in up to four segments of 64: n_coarse = 66 / 67, 130 / 131, 194 / 195
    are the two sides of every segment boundary, 3 and 258 the limits of the API.

Everything here is written from the comments and formulas of raymarch.hip and oracle/nerf_ref.py.
"""
import functools

import numpy as np

from oracle import nerf_ref

NEAR, FAR = 2., 6.

# ------------------------------------------------------------------------------------------------ the shape lists
COMPOSITE_S = (1, 2, 7, 63, 64, 65, 128, 129, 200, 257)
BWD_BIG_S = (2048, 2049, 4096)          # backward only: an fp32 product of thousands of factors no longer fits 2e-5
BWD_BIG_N = 5
RAY_COUNTS = (1, 2, 3, 5, 13, 129)
N_ALL = 13                              # every S runs at this ray count ...
S_ALL = 65                              # ... and every ray count at this S
COMPOSITE_CASES = tuple((N_ALL, s) for s in COMPOSITE_S) + tuple((n, S_ALL) for n in RAY_COUNTS if n != N_ALL)
BWD_CASES = COMPOSITE_CASES + tuple((BWD_BIG_N, s) for s in BWD_BIG_S)
FINE_SHAPES = ((3, 2), (4, 2), (16, 8), (64, 128), (66, 64), (67, 65), (130, 3), (131, 128), (194, 64), (195, 64),
               (258, 320))
FINE_CASES = tuple((N_ALL, nc, nf) for nc, nf in FINE_SHAPES) + tuple((n, 67, 65) for n in (1, 2, 3, 5))

# the tolerances of the GPU file, each the figure of a test the project already has
TOL_FWD = 2e-5                          # rgb, occu, weights: tests/test_gpu_nerf.py::test_composite_vs_oracle
TOL_DEPTH = 1e-5 * FAR                  # tests/test_gpu_render_from_nerf.py::_check_surface, the same sum
BWD_RTOL, BWD_ATOL = 2e-3, 2e-5         # x max |want|: tests/test_gpu_train.py::test_composite_backward_vs_autograd
TOL_NORMALIZE = 2e-7                    # tests/test_gpu_nerf.py::test_normalize_and_gen_z

N_RANDOM = 3        # a case keeps at least this many plain random rays: the named rays are written over the first rows
                    # only as far as that allows (n = 1, 2, 3 are all random, n = 5 has two named rays, n >= 13 all)
OPAQUE_SIGMA, OPAQUE_GAP = 500., 0.1    # along a unit direction: alpha = 1 - exp(-50) = 1 in fp32

EDGE_NAMES = ('empty', 'zero', 'negzero', 'opaque_first', 'opaque_mid', 'last_only', 'saturated', 'repeated_z',
              'dir_small', 'dir_large')
FINE_NAMES = ('all_zero', 'one_inner', 'outer_first', 'outer_last', 'mostly_zero', 'tiny', 'repeated_z', 'uniform')


def _rows(names, n):
    return {name: i for i, name in enumerate(names) if i < n - N_RANDOM}


def edge_rows(n, s):
    """name -> row of the named rays edge_rays(n, s, .) holds."""
    return _rows([k for k in EDGE_NAMES if k != 'repeated_z' or s > 2], n)


def fine_rows(n):
    return _rows(FINE_NAMES, n)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def edge_rays(n, s, seed=0):
    """(rgbs [n, s, 4], z [n, s], rayd [n, 3], noise [n, s], g [n, 3]) in float32, read-only.  The base of every ray is
    the recipe of tests/test_gpu_train.py::test_composite_backward_vs_autograd (raw colours N(0, 1), raw density
    3 N(0, 1) + 0.5, z sorted uniform in [near, far], directions N(0, 1), not normalised); edge_rows(n, s) names the rays
    written over the first rows.  `noise` is there for the caller to pass or not."""
    rng = np.random.default_rng(1000003 * seed + 4099 * s + n)
    rgbs = rng.normal(size=(n, s, 4)).astype(np.float32)
    rgbs[..., 3] = rgbs[..., 3] * 3. + 0.5
    z = np.sort(rng.uniform(NEAR, FAR, size=(n, s)).astype(np.float32), 1)
    rayd = rng.normal(size=(n, 3)).astype(np.float32)
    noise = rng.normal(size=(n, s)).astype(np.float32)
    g = rng.normal(size=(n, 3)).astype(np.float32)

    def opaque_at(r, k):
        # the interval behind sample k is at least OPAQUE_GAP long along a unit direction (the last one is 1e10 anyway)
        z[r] = NEAR + (z[r] - NEAR) * np.float32((FAR - NEAR - OPAQUE_GAP) / (FAR - NEAR))
        z[r, k + 1:] += np.float32(OPAQUE_GAP)
        rayd[r] = nerf_ref.l2_normalize(rayd[r:r + 1], 1, 1e-12)[0]
        rgbs[r, k, 3] = OPAQUE_SIGMA

    for name, r in edge_rows(n, s).items():
        if name == 'empty':
            rgbs[r, :, 3] = -1.
        elif name == 'zero':
            rgbs[r, :, 3] = 0.
        elif name == 'negzero':
            rgbs[r, :, 3] = -0.
        elif name == 'opaque_first':
            opaque_at(r, 0)
        elif name == 'opaque_mid':                  # nothing in front of it: the weight of sample s // 2 is the ray's
            rgbs[r, :, 3] = -1.
            opaque_at(r, s // 2)
        elif name == 'last_only':                   # 1e-3 x the last interval of 1e10: opaque all the same
            rgbs[r, :, 3] = -1.
            rgbs[r, -1, 3] = 1e-3
        elif name == 'saturated':
            rgbs[r, :, 3] = 30.
        elif name == 'repeated_z':                  # dist = 0 on every interval but the first and the last
            z[r, 1:] = z[r, 1]
        elif name == 'dir_small':
            rayd[r] *= np.float32(1e-3)
        elif name == 'dir_large':
            rayd[r] *= np.float32(1e3)
    return _frozen(rgbs, z, rayd, noise, g)


@functools.lru_cache(maxsize=None)
def fine_cases(nc, nf, seed=0, n=N_ALL):
    """(z [n, nc], w [n, nc]) in float32, read-only, for sample_fine: z = stratified depths in [near, far], w = uniform^6;
    fine_rows(n) names the rays written over the first rows (nf only enters the seed)."""
    rng = np.random.default_rng(1000003 * seed + 7919 * nc + 31 * nf + n)
    z = nerf_ref.gen_z(NEAR, FAR, nc, n, u=rng.uniform(size=(n, nc)).astype(np.float32)).copy()
    w = rng.uniform(size=(n, nc)).astype(np.float32) ** 6
    keep = rng.uniform(size=nc) > 0.7
    for name, r in fine_rows(n).items():
        if name == 'all_zero':
            w[r] = 0.
        elif name == 'one_inner':
            w[r] = 0.
            w[r, 1 + (nc - 2) // 2] = 1.
        elif name == 'outer_first':                 # the pdf is weights[1:-1]: this ray counts as empty
            w[r] = 0.
            w[r, 0] = 1.
        elif name == 'outer_last':
            w[r] = 0.
            w[r, -1] = 1.
        elif name == 'mostly_zero':                 # roughly 70 % of the bins exactly zero
            w[r] = w[r] * keep
        elif name == 'tiny':
            w[r] = 1e-30
        elif name == 'repeated_z':
            z[r, nc // 2:] = z[r, nc // 2]
        elif name == 'uniform':                     # every inner weight exactly 0.25
            w[r, 1:-1] = 0.25
    return _frozen(z, w)


def linspace_u(n, nf):
    """U[r, i] = float32(i) * (float32(1) / float32(nf - 1)): linspace01 of the kernel and of the oracle, as an explicit u."""
    return np.broadcast_to(nerf_ref.linspace01(nf, np.float32), (n, nf)).copy()


def fine_pdf_cdf(w_row):
    """(pdf [nc - 2], cdf [nc - 1]) of one ray in the oracle's order (inv_transform_sample: sequential sums in float32)."""
    inner = np.asarray(w_row, np.float32)[None, 1:-1]
    pdf = inner / (nerf_ref.seq_cumsum(inner)[:, -1:] + np.float32(1e-5))
    return pdf[0], np.concatenate((np.zeros(1, np.float32), nerf_ref.seq_cumsum(pdf)[0]))


def fine_samples(z, w, nf, u=None):
    """The oracle's fine samples before the sort: [n, nf]."""
    z = np.asarray(z, np.float32)
    mid = np.float32(.5) * (z[:, 1:] + z[:, :-1])
    return nerf_ref.inv_transform_sample(mid, np.asarray(w, np.float32)[:, 1:-1], nf, u=u)


def chosen_u_case():
    """(z, w, u, row): fine_cases at n_coarse = 6, whose `uniform` ray `row` has four equal pdf bins, and a u (the same for
    every ray) that holds 0, that ray's interior cdf entries bit for bit, their float neighbours on both sides, the next
    float below 1 and 0.5, in no particular order: the oracle's `<=` search decides every one of them."""
    nc = 6
    below, above = np.float32(0), np.float32(1)
    u_of = lambda cdf: np.concatenate(([0.], cdf[1:], np.nextafter(cdf[1:], below), np.nextafter(cdf[1:], above),
                                       [np.nextafter(above, below), 0.5])).astype(np.float32)
    nf = u_of(np.zeros(nc - 1, np.float32)).size
    z, w = fine_cases(nc, nf)
    row = fine_rows(N_ALL)['uniform']
    u = u_of(fine_pdf_cdf(w[row])[1])
    u = u[np.random.default_rng(6).permutation(nf)]
    return z, w, np.broadcast_to(u, (N_ALL, nf)).copy(), row


# ------------------------------------------------------------------------------------------------ sample_fine's ranks
def rank_general(zall):
    """sample_fine's all-pairs rule on one ray (1-D): rank[i] = #{j : zall[j] < zall[i], or equal and j < i}."""
    zall = np.asarray(zall)
    j = np.arange(zall.size)
    o, v = zall[None, :], zall[:, None]
    return np.sum((o < v) | ((o == v) & (j[None, :] < j[:, None])), 1)


def _count_by_bisection(lst, v, or_equal):
    """The kernel's binary search, step for step: on a sorted list the number of elements < v (<= v with or_equal)."""
    lo, hi = 0, len(lst)
    while lo < hi:
        m = (lo + hi) >> 1
        if (lst[m] <= v) if or_equal else (lst[m] < v):
            lo = m + 1
        else:
            hi = m
    return lo


def rank_sorted_lists(zc, zf):
    """sample_fine's rule for two sorted lists (deterministic sampling), ranks in the order of concat(zc, zf): a coarse
    element gets its index plus the number of fine elements strictly below it, a fine element its index plus the number
    of coarse elements below or equal (the coarse list comes first in the concatenation, so it wins ties)."""
    rc = [i + _count_by_bisection(zf, v, False) for i, v in enumerate(zc)]
    rf = [i + _count_by_bisection(zc, v, True) for i, v in enumerate(zf)]
    return np.array(rc + rf)


# ------------------------------------------------------------------------------------------------ compositing
def _exp_moved_one_ulp(x, rng, cap=np.inf):
    """exp(x) with every value one ulp up, one ulp down or unchanged, at random, kept inside [0, cap]; exp(0) stays
    exactly 1, as it is in every implementation (an empty sample's alpha is exactly 0 in the kernel and in the oracle)."""
    e = np.exp(x)
    move = np.where(x == 0, 0, rng.integers(-1, 2, size=e.shape))
    up, down = np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))
    return np.clip(np.where(move > 0, up, np.where(move < 0, down, e)), np.float32(0), np.float32(cap)).astype(np.float32)


def _wave_sum(v):
    """wave_sum of nfx_common.hpp on [n, 64] lane values: butterfly over lane ^ 32, 16, ..., 1; what lane 0 holds."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def composite_scan_emulation(rgbs, z, rayd, noise=None, white_bg=True, ulp_rng=None):
    """composite_kernel's evaluation order in NumPy float32: chunks of 64 samples, a Hillis-Steele inclusive product inside
    a chunk, `carry` across chunks, padding lanes holding t = 1, per-lane partial sums over the chunks and the butterfly
    wave_sum.  ulp_rng: move every exp value (the density's and the sigmoids') by +-1 ulp at random, standing in for the
    device's expf.  -> dict(rgb, occu, depth, disp, weights)."""
    f = np.float32
    rgbs, z, rayd = (np.asarray(a, f) for a in (rgbs, z, rayd))
    n, S = z.shape
    n_chunks = (S + 63) // 64
    P = n_chunks * 64
    # (cap: exp of a non-positive number stays inside [0, 1])
    exp = (lambda x, cap=np.inf: _exp_moved_one_ulp(x, ulp_rng, cap)) if ulp_rng is not None else (lambda x, cap=None: np.exp(x))
    dx, dy, dz = rayd[:, 0], rayd[:, 1], rayd[:, 2]
    dnorm = np.sqrt(dx * dx + dy * dy + dz * dz)
    dist = np.concatenate((z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10, f)), 1) * dnorm[:, None]
    sg = rgbs[..., 3] if noise is None else rgbs[..., 3] + np.asarray(noise, f)
    with np.errstate(over='ignore', under='ignore'):
        alpha = f(1) - exp(-np.maximum(sg, f(0)) * dist, 1.)
        t = np.ones((n, P), f)
        t[:, :S] = f(1) - alpha + f(1e-6)
        incl = t.reshape(n, n_chunks, 64).copy()
        o = 1
        while o < 64:
            nxt = incl.copy()
            nxt[..., o:] = incl[..., o:] * incl[..., :-o]
            incl, o = nxt, o * 2
        excl = np.concatenate((np.ones((n, n_chunks, 1), f), incl[..., :-1]), 2)
        T = np.empty((n, n_chunks, 64), f)
        carry = np.ones(n, f)
        for c in range(n_chunks):
            T[:, c] = carry[:, None] * excl[:, c]
            carry = carry * incl[:, c, 63]
        w = np.zeros((n, P), f)
        w[:, :S] = alpha * T.reshape(n, P)[:, :S]
        col = np.zeros((n, P, 3), f)
        col[:, :S] = f(1) / (f(1) + exp(-rgbs[..., :3]))
        zp = np.zeros((n, P), f)
        zp[:, :S] = z
        lane = lambda a: a.reshape(n, n_chunks, 64)
        sums = [np.zeros((n, 64), f) for _ in range(5)]
        terms = [lane(w), lane(w * col[..., 0]), lane(w * col[..., 1]), lane(w * col[..., 2]), lane(w * zp)]
        for c in range(n_chunks):
            for k in range(5):
                sums[k] = sums[k] + terms[k][:, c]
        s_w, s_r, s_g, s_b, s_d = (_wave_sum(v) for v in sums)
    bg = f(1) if white_bg else f(0)
    k = f(1) - s_w
    rgb = np.stack((s_r * s_w + bg * k, s_g * s_w + bg * k, s_b * s_w + bg * k), 1)
    return dict(rgb=rgb, occu=s_w, depth=s_d, disp=f(1) / np.maximum(s_d, f(1e-10)), weights=w[:, :S])


def torch_composite_all(rgbs, z, rayd, white_bg, noise=None):
    """tests/test_gpu_train.py::torch_composite (nerf.py:184-254 in torch, any dtype, for autograd), returning
    (rgb, occu, depth, weights); unlike the NumPy oracle it takes S = 1."""
    import torch
    dist = torch.cat((z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)), 1) * rayd.norm(dim=1, keepdim=True)
    sg = rgbs[..., 3] if noise is None else rgbs[..., 3] + noise
    alpha = 1. - torch.exp(-torch.relu(sg) * dist)
    t = 1. - alpha + 1e-6
    T = torch.cat((torch.ones_like(t[:, :1]), torch.cumprod(t, 1)[:, :-1]), 1)
    w = alpha * T
    occu = w.sum(1, keepdim=True)
    rgb = (w[..., None] * torch.sigmoid(rgbs[..., :3])).sum(1)
    return rgb * occu + (1. if white_bg else 0.) * (1. - occu), occu[:, 0], (w * z).sum(1), w


BWD_COMBOS = ((True, False), (False, True), (True, True), (False, False))      # (white_bg, use_noise)


@functools.lru_cache(maxsize=None)
def backward_ref(n, s, white_bg, use_noise, dtype='float64'):
    """(d_rgbs [n, s, 4], rgb [n, 3]) of edge_rays(n, s) by torch autograd in `dtype`, as NumPy arrays, read-only."""
    import torch
    dt = getattr(torch, dtype)
    rgbs, z, rayd, noise, g = edge_rays(n, s)
    t = torch.tensor(rgbs, dtype=dt, requires_grad=True)
    rgb = torch_composite_all(t, torch.tensor(z, dtype=dt), torch.tensor(rayd, dtype=dt), white_bg,
                              torch.tensor(noise, dtype=dt) if use_noise else None)[0]
    rgb.backward(torch.tensor(g, dtype=dt))
    return _frozen(t.grad.numpy(), rgb.detach().numpy())


def forward_compared_rays(n, s, white_bg, use_noise):
    """Rays whose composited colour is compared with the FLOAT64 formula at TOL_FWD (tests/shade_cases.py::compared_set): those
    where the same formula in float32 stays within half of it.  The others are rays with a long run of empty samples in
    front of an opaque one (last_only, repeated_z, opaque_mid at S >= 200): every empty sample multiplies the transmittance
    by 1 + 1e-6, which float32 rounds to 1 + 8 ulp = 1 + 9.54e-7, so that 256 of them leave float32 — the reference's own
    and the kernel's alike — 1.2e-5 of the product from float64, and the colour up to twice that.  Those rays are still
    held to the float32 oracle at TOL_FWD by the forward tests.  "In float32" = in torch's order and in the kernel's."""
    rgbs, z, rayd, noise, _ = edge_rays(n, s)
    rgb64 = backward_ref(n, s, white_bg, use_noise)[1]
    emu = composite_scan_emulation(rgbs, z, rayd, noise if use_noise else None, white_bg)['rgb']
    d = np.maximum(np.abs(backward_ref(n, s, white_bg, use_noise, 'float32')[1] - rgb64), np.abs(emu - rgb64)).max(1)
    return d <= 0.5 * TOL_FWD


def bwd_error_ratio(got, want):
    """max |got - want| / (atol + rtol |want|) with the backward tolerance: <= 1 is what assert_allclose accepts."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (BWD_ATOL * np.abs(want).max() + BWD_RTOL * np.abs(want) + 1e-300)))
