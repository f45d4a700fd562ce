"""Inputs and float64 references for the shading kernels of csrc/shade.hip (shade_kernel, shade_olat_kernel,
shade_bwd_kernel) at every light count and launch shape they branch on.  No GPU: tests/test_cpu_shade_cases.py checks the
conditions on these inputs, tests/test_gpu_shade_shapes.py holds the kernels to the references.

Why not the recipe of tests/test_gpu_nerfactor.py::_shade_inputs: at roughness down to 0.05 GGX cancels in fp32, the fp32
oracle sits up to 9e-4 from the float64 one, and behind such a bound one lost light of 512 (3e-4) cannot be seen.  Here

  * the roughness is uniform(0.3, 1), the visibilities uniform(0.1, 1), the albedo uniform(0.03, 0.8): the two oracles then
    agree to ~1e-5 on (almost) every output, and the few outputs where they do not are left out of the tight comparison
    and counted (compared_set);
  * the lights are L random unit directions x 100 with random solid angles that sum to 4 pi: any L, no lat-long structure;
  * besides two "natural" probes there are ONE-HOT probes, intensity L / 4 at one light and 0 elsewhere, at the lights on
    both sides of every boundary of the kernels' light loops (a lane keeps 8 lights, a pass covers 512): such an output IS
    the transport of that one light, so a lost or shifted light is an error of the whole value, not of 1 / L of it.
"""
import functools

import numpy as np

from oracle import nerf_ref, nerfactor_ref as R

F0 = 0.04
SPEC_SCALE = 0.7
OLAT_AMBIENTS = (0., 0.05)
KINDS = ('microfacet', 'spec')
# (BRDF, linear2srgb) of the OLAT cases.  Microfacet without the tonemap is left out: the oracle pair's distance there is set
# by the brightest highlights (up to 1e-5), 100 x the bound is then 8e-3, and 11-13 % of the LINEAR front-lit outputs are
# dimmer than that whatever the seed (grazing lights on dark albedo) — the sensitivity condition of the CPU file cannot
# hold.  The sRGB curve lifts those outputs (12.92 x near 0); the branch without it runs with the given-specular BRDF.
OLAT_COMBOS = (('microfacet', True), ('spec', True), ('spec', False))

FWD_LIGHTS = (1, 21, 63, 64, 65, 511, 512, 513, 577, 1100, 2048)
BWD_LIGHTS = (21, 65, 512, 577, 2048)
N_SMALL = 41                 # five workgroups of 8 waves plus one wave
SMALL_NS = (1, 7, 8, 9)      # at L = 65
N_STRIDE_FWD, L_STRIDE_FWD = 4096 + 13, 64      # shade_kernel: 512 workgroups x 8 waves, then the grid-stride loop
N_STRIDE_BIG, L_STRIDE_BIG = 16384 + 13, 32     # OLAT and backward: 2048 workgroups x 8 waves
L_ROWS = 577

# (L, n) of every case of the GPU file, per entry point
FWD_CASES = tuple((L, N_SMALL) for L in FWD_LIGHTS) + tuple((65, n) for n in SMALL_NS) + ((L_STRIDE_FWD, N_STRIDE_FWD),)
OLAT_CASES = tuple((L, N_SMALL) for L in FWD_LIGHTS) + tuple((65, n) for n in SMALL_NS) + ((L_STRIDE_BIG, N_STRIDE_BIG),)
BWD_CASES = tuple((L, N_SMALL) for L in BWD_LIGHTS) + ((L_STRIDE_BIG, N_STRIDE_BIG),)

# Cases whose first draw broke a condition of tests/test_cpu_shade_cases.py (a condition on the inputs): drawn again
RESEED = {(65, 41): 3, (512, 41): 3}

COMPARED_DIST = 1e-5         # fp32 oracle vs float64 oracle: outputs farther apart are not compared tightly
BOUND_FACTOR = 8.
BOUND_FLOOR = 1e-6


def hot_lights(L):
    """The lights a one-hot probe names: both sides of the 64-lane group, of the 512-light pass and of its first tail group."""
    return sorted({l for l in (0, 63, 64, 511, 512, 575, 576) if l < L} | {L - 1})


def bwd_columns(L):
    return sorted({l for l in (0, 63, 64, 511, 512) if l < L} | {L - 1})


class Case:
    """float32 inputs of one (L, n); `probes` [P, L, 3]: 2 natural ones, then one one-hot probe per hot_lights(L) (none for
    the grid-stride cases, which run with P = 2)."""

    def __init__(self, L, n):
        self.L, self.n = L, n
        rng = np.random.default_rng(7000 + 13 * L + n + 100000 * RESEED.get((L, n), 0))
        d = rng.normal(size=(L, 3))
        self.lxyz = (100. * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        a = rng.uniform(.5, 1.5, size=L)
        self.lareas = (a * (4 * np.pi / a.sum())).astype(np.float32)
        # the points of tests/test_gpu_nerfactor.py::scene
        self.xyz = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
        cam = (np.array([2.4, -2.6, 1.8]) * 4 / np.linalg.norm([2.4, -2.6, 1.8])).astype(np.float32)
        self.cam = np.broadcast_to(cam, (n, 3)).copy()
        self.normal = nerf_ref.l2_normalize(rng.normal(size=(n, 3)).astype(np.float32), 1, 1e-6)
        self.albedo = rng.uniform(.03, .8, size=(n, 3)).astype(np.float32)
        self.rough = rng.uniform(.3, 1., size=(n, 1)).astype(np.float32)
        self.lvis = rng.uniform(.1, 1., size=(n, L)).astype(np.float32)
        self.spec = (rng.uniform(size=(n, L)) ** 4).astype(np.float32)
        natural = (np.exp(rng.normal(size=(2, L, 3))) * .3).astype(np.float32)
        self.hot = hot_lights(L) if n < 1000 else []
        self.olat_inten = L / 4.
        one_hot = [R.one_hot_light(1, L, 0, l, self.olat_inten, 0.).reshape(L, 3) for l in self.hot]
        self.probes = np.concatenate((natural, np.stack(one_hot).astype(np.float32)), 0) if one_hot else natural
        self.n_natural = 2
        # backward: the trained light and the upstream gradient
        self.light = (natural[0] * .5).astype(np.float32)
        self.drgb = rng.normal(size=(n, 3)).astype(np.float32)

    def __repr__(self):
        return 'L%d_n%d' % (self.L, self.n)


@functools.lru_cache(maxsize=None)
def case(L, n):
    return Case(L, n)


@functools.lru_cache(maxsize=None)
def _geometry(L, n, kind, dtype):
    """(surf2l [n, L, 3], brdf [n, L, 3]) of the oracle in `dtype`."""
    c = case(L, n)
    f = lambda a: a.astype(dtype)
    surf2l = R.calc_ldir(f(c.xyz), f(c.lxyz))
    if kind == 'microfacet':
        brdf = R.microfacet(surf2l, R.calc_vdir(f(c.cam), f(c.xyz)), f(c.normal), f(c.albedo), f(c.rough), f0=F0)
    else:
        brdf = f(c.albedo)[:, None, :] / dtype(np.pi) + f(c.spec)[:, :, None] * dtype(SPEC_SCALE)
    return surf2l, brdf


def forward_ref(c, kind, to_srgb, dtype, probes=None):
    """rgb [n, P, 3]: oracle.nerfactor_ref.integrate per probe, evaluated in `dtype`."""
    surf2l, brdf = _geometry(c.L, c.n, kind, dtype)
    probes = c.probes if probes is None else probes
    return np.stack([R.integrate(brdf, c.lvis.astype(dtype), surf2l, c.normal.astype(dtype), p.astype(dtype),
                                 c.lareas.astype(dtype), to_srgb) for p in probes], 1)


@functools.lru_cache(maxsize=None)
def _transport(L, n, kind, dtype):
    c = case(L, n)
    surf2l, brdf = _geometry(L, n, kind, dtype)
    cos = np.einsum('ijk,ik->ij', surf2l, c.normal.astype(dtype))
    lv = (cos > 0).astype(dtype) * c.lvis.astype(dtype)
    return brdf * lv[:, :, None] * cos[:, :, None] * c.lareas.astype(dtype).reshape(1, -1, 1)


def transport(c, kind, dtype=np.float64):
    """T[n, l, c] = brdf * lvis * [cos > 0] * cos * area: what light l carries to point n per unit of intensity."""
    return _transport(c.L, c.n, kind, dtype)


def light_cosines(c):
    surf2l, _ = _geometry(c.L, c.n, 'spec', np.float64)
    return np.einsum('ijk,ik->ij', surf2l, c.normal.astype(np.float64))


def front_lit(c):
    return light_cosines(c) > 0


def tonemap(x, to_srgb):
    x = np.clip(x, 0., 1.)
    return R.linear2srgb(x) if to_srgb else x


def olat_ref(c, kind, ambient, to_srgb, dtype=np.float64, without_own_light=False):
    """rgb_olat [n, L, 3]: column l is the render under one_hot_light(l, inten, ambient) = inten T[:, l] + ambient sum_l' T.
    without_own_light: column l with light l deleted from the integral (the sensitivity of the CPU file)."""
    T = transport(c, kind, dtype)
    tot = T.sum(1, keepdims=True)
    r = dtype(ambient) * (tot - T) if without_own_light else dtype(c.olat_inten) * T + dtype(ambient) * tot
    return tonemap(r, to_srgb)


def compared_set(ref32, ref64):
    """(mask of the outputs compared tightly, d_ref = the oracle pair's own distance on them, share left out)."""
    d = np.abs(ref32.astype(np.float64) - ref64)
    mask = d <= COMPARED_DIST
    return mask, float(d[mask].max()) if mask.any() else 0., 1. - float(mask.mean())


def bound(d_ref):
    """8 x the oracle pair's own distance: another operation order in the same fp32 class (the per-point terms hoisted into
    microfacet_point, a wave tree sum against NumPy's pairwise sum, tonemap_fast's 1e-6 before the sRGB slope of 12.92)."""
    return BOUND_FACTOR * max(d_ref, BOUND_FLOOR)


# ------------------------------------------------------------------------------------------------------- backward
def _torch_render_spec(xyz, normal, albedo, spec, lvis, lxyz, lareas, light, to_srgb):
    """tests/test_gpu_train.py::_torch_render with the given-specular BRDF albedo / pi + spec * scale."""
    import torch
    from nerfactor_amd.nerfactor.util import img as imgutil
    d = lxyz[None] - xyz[:, None]
    surf2l = d * torch.rsqrt(torch.clamp((d * d).sum(2, keepdim=True), min=1e-6))
    brdf = albedo[:, None, :] / np.pi + spec[:, :, None] * SPEC_SCALE
    cos = torch.einsum('ijk,ik->ij', surf2l, normal)
    rgb = (brdf * (((cos > 0).double() * lvis)[:, :, None] * light[None]) * cos[:, :, None] * lareas[None, :, None]).sum(1)
    rgb = torch.clamp(rgb, 0., 1.)
    return imgutil.linear2srgb(rgb) if to_srgb else rgb


def inside_points(c, kind, to_srgb):
    """Points whose three channels are away from the clip kinks, before the tonemap and after it."""
    pre = np.einsum('nlc,lc->nc', transport(c, kind), c.light.astype(np.float64))
    post = tonemap(pre, to_srgb)
    ok = lambda v: ((v > 1e-4) & (v < 1 - 1e-4)).all(1)
    return ok(pre) & ok(post)


@functools.lru_cache(maxsize=None)
def _backward_ref(L, n, kind, to_srgb):
    import torch
    from tests.test_gpu_train import _torch_render
    c = case(L, n)
    inside = inside_points(c, kind, to_srgb)
    idx = np.nonzero(inside)[0]
    out = {'inside': inside}
    for which, sel in (('all', np.arange(n)), ('inside', idx)):
        t = lambda a, g=False: torch.tensor(a[sel], dtype=torch.float64, requires_grad=g)     # per-point arrays only
        tn, ta, tr, tv, ts = t(c.normal, True), t(c.albedo, True), t(c.rough, True), t(c.lvis, True), t(c.spec, True)
        tl = torch.tensor(c.light, dtype=torch.float64, requires_grad=True)
        lxyz, lareas = torch.tensor(c.lxyz, dtype=torch.float64), torch.tensor(c.lareas, dtype=torch.float64)
        if kind == 'microfacet':
            rgb = _torch_render(t(c.xyz), t(c.cam), tn, ta, tr, tv, lxyz, lareas, tl, to_srgb)
        else:
            rgb = _torch_render_spec(t(c.xyz), tn, ta, ts, tv, lxyz, lareas, tl, to_srgb)
        rgb.backward(t(c.drgb))
        if which == 'all':
            out.update(d_albedo=ta.grad.numpy(), d_normal=tn.grad.numpy(), d_lvis=tv.grad.numpy(),
                       d_param=(tr.grad.numpy()[:, 0] if kind == 'microfacet' else ts.grad.numpy()))
        else:
            out['d_light_inside'] = tl.grad.numpy()
    return out


def backward_ref(c, kind, to_srgb):
    """float64 autograd: d_albedo, d_normal, d_lvis, d_param (d_rough [n] | d_spec [n, L]) of every point, `inside`, and
    d_light_inside [L, 3] summed over the inside points only (outside the clip range the gradient is 0 or at a kink)."""
    return _backward_ref(c.L, c.n, kind, bool(to_srgb))
