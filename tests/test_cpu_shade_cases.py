"""Conditions on the inputs and references of tests/shade_cases.py, for every case tests/test_gpu_shade_shapes.py uses.

These are conditions on the REFERENCE, not measurements of a kernel.  A case that breaks one is a badly chosen case: change
its seed or the case, not the cap.

  * compared set: at most 1 % of a case's outputs have the fp32 oracle farther than 1e-5 from the float64 one (they are left
    out of the tight comparison and counted);
  * of the front-lit one-hot / OLAT outputs at least 95 % lie strictly inside (0, 1): the clip hides nothing there (the
    back-lit ones are exactly 0, which is right and is compared too);
  * sensitivity: deleting the ONE light a one-hot probe or an OLAT column names moves at least 90 % of its front-lit points by
    at least 100 x the bound the GPU file asserts.  The OLAT columns at hot_lights(L) are held to that one by one, all
    columns together as a pool (a single column of the 41-point cases has ~20 front-lit points: 90 % of each of 2048
    columns is a statement about the luck of the draw, not about the bound);
  * backward: at least half the points are away from the clip kinks.
"""
import numpy as np
import pytest

from oracle import nerfactor_ref as R
from tests import shade_cases as S

ids = lambda cases: ['L%d-n%d' % c for c in cases]


@pytest.mark.parametrize("L,n", S.FWD_CASES, ids=ids(S.FWD_CASES))
def test_forward_cases_are_well_conditioned_and_see_single_lights(L, n):
    c = S.case(L, n)
    front = S.front_lit(c)
    for kind in S.KINDS:
        linear = S.forward_ref(c, kind, False, np.float64)       # (saturation is decided before the tonemap)
        for to_srgb in (True, False):
            ref32, ref64 = S.forward_ref(c, kind, to_srgb, np.float32), S.forward_ref(c, kind, to_srgb, np.float64)
            assert ref64.shape == (n, c.probes.shape[0], 3)
            mask, d_ref, left_out = S.compared_set(ref32, ref64)
            assert left_out <= 0.01, (kind, to_srgb, left_out)
            tol = S.bound(d_ref)
            print('%r %s srgb=%d: d_ref %.2e, left out %.3f %%' % (c, kind, to_srgb, d_ref, 100 * left_out))
            inside, total = 0, 0
            for j, l in enumerate(c.hot):
                got = ref64[front[:, l], c.n_natural + j]        # the one-hot probe of light l at its front-lit points
                assert np.all(ref64[~front[:, l], c.n_natural + j] == 0)
                lin = linear[front[:, l], c.n_natural + j]
                inside += int(((lin > 0) & (lin < 1)).sum())
                total += got.size
                # without light l the probe is dark: the effect of deleting it is the output itself
                if n >= S.N_SMALL:
                    assert (got.min(1) >= 100 * tol).mean() >= 0.9, (kind, to_srgb, l, tol, np.sort(got.min(1))[:6])
            if c.hot and n >= S.N_SMALL:
                assert inside >= 0.95 * total, (kind, to_srgb, inside, total)
            # the natural probes: what one light of L is worth there (the reason for the one-hot probes)
            nat = c.probes[:c.n_natural].copy()
            nat[:, L - 1] = 0
            effect = np.abs(S.forward_ref(c, kind, to_srgb, np.float64, probes=nat) - ref64[:, :c.n_natural]).max()
            print('    natural probes without light %d: worst point moves by %.2e (bound %.1e)' % (L - 1, effect, tol))


@pytest.mark.parametrize("L,n", S.OLAT_CASES, ids=ids(S.OLAT_CASES))
def test_olat_cases_are_well_conditioned_and_see_single_lights(L, n):
    c = S.case(L, n)
    front = S.front_lit(c)
    for kind, to_srgb in S.OLAT_COMBOS:
        for ambient in S.OLAT_AMBIENTS:
            if True:
                ref32 = S.olat_ref(c, kind, ambient, to_srgb, np.float32)
                ref64 = S.olat_ref(c, kind, ambient, to_srgb)
                mask, d_ref, left_out = S.compared_set(ref32, ref64)
                assert left_out <= 0.01, (kind, ambient, to_srgb, left_out)
                tol = S.bound(d_ref)
                print('%r %s ambient=%g srgb=%d: d_ref %.2e, left out %.3f %%' % (c, kind, ambient, to_srgb, d_ref, 100 * left_out))
                if n < S.N_SMALL:
                    continue
                lit = S.olat_ref(c, kind, ambient, False)[front]
                assert ((lit > 0) & (lit < 1)).mean() >= 0.95, (kind, ambient, to_srgb)
                effect = np.abs(ref64 - S.olat_ref(c, kind, ambient, to_srgb, without_own_light=True)).min(2)
                assert (effect[front] >= 100 * tol).mean() >= 0.9, (kind, ambient, to_srgb, tol)
                for l in S.hot_lights(L):
                    e = effect[front[:, l], l]
                    assert (e >= 100 * tol).mean() >= 0.9, (kind, ambient, to_srgb, l, tol, np.sort(e)[:6])


def test_olat_reference_is_the_oracle_integral_under_a_one_hot_light():
    """inten T[:, l] + ambient sum T is oracle.nerfactor_ref.integrate under one_hot_light(l), in float64 to rounding."""
    c = S.case(577, S.N_SMALL)
    f = lambda a: a.astype(np.float64)
    for kind in S.KINDS:
        surf2l, brdf = S._geometry(c.L, c.n, kind, np.float64)
        for ambient in S.OLAT_AMBIENTS:
            ref = S.olat_ref(c, kind, ambient, True)
            for l in (0, 511, 512, 576):
                env = R.one_hot_light(1, c.L, 0, l, c.olat_inten, ambient, dtype=np.float64)
                want = R.integrate(brdf, f(c.lvis), surf2l, f(c.normal), env, f(c.lareas), True)
                assert np.abs(ref[:, l] - want).max() < 1e-12


@pytest.mark.parametrize("L,n", S.BWD_CASES, ids=ids(S.BWD_CASES))
def test_backward_cases_keep_half_the_points_inside_the_clip_range(L, n):
    c = S.case(L, n)
    for kind in S.KINDS:
        for to_srgb in (True, False):
            inside = S.inside_points(c, kind, to_srgb)
            assert inside.mean() >= 0.5, (kind, to_srgb, inside.mean())


def test_backward_reference_matches_a_central_difference():
    """The float64 autograd of both BRDF forms against (f(x + h) - f(x - h)) / 2h of the float64 forward in one light."""
    c = S.case(21, S.N_SMALL)
    for kind in S.KINDS:
        ref = S.backward_ref(c, kind, True)
        idx = np.nonzero(ref['inside'])[0]
        assert ref['d_lvis'].shape == (c.n, c.L) and ref['d_light_inside'].shape == (c.L, 3)
        T = S.transport(c, kind)
        loss = lambda light: (S.tonemap(np.einsum('nlc,lc->nc', T[idx], light), True) * c.drgb[idx]).sum()
        light = c.light.astype(np.float64)
        for l, ch in ((0, 0), (20, 2), (7, 1)):
            h = np.zeros_like(light)
            h[l, ch] = 1e-6
            fd = (loss(light + h) - loss(light - h)) / 2e-6
            assert abs(fd - ref['d_light_inside'][l, ch]) <= 1e-6 * max(1., abs(fd)), (kind, l, ch)


def test_shade_bwd_argument_check_counts_what_the_launcher_allocates(nfx_lib):
    """nfx_shade_bwd needs 28 bytes of LDS per light and 24 more with a light gradient; its argument check (made before
    anything touches the GPU, here with n = 0 points) and the launcher size it from one expression.  It used to count 28
    either way: 3151 ... 5851 lights with d_light passed the check and failed inside the launcher with a bare HIP error."""
    import ctypes

    def call(n_lights, with_d_light):
        d_light = ctypes.c_void_p(8) if with_d_light else None      # only ever compared with null: there are no points
        return nfx_lib.lib.nfx_shade_bwd(None, None, None, None, None, None, 1., 0.04, None, None, None, None, 0, n_lights, 1,
                                         None, None, None, None, None, None, d_light, None, 0, None)
    for n_lights, with_d_light, ok in ((5851, False, True), (5852, False, False), (3150, True, True), (3151, True, False),
                                       (4608, False, True), (4608, True, False), (512, True, True)):
        rc = call(n_lights, with_d_light)
        assert (rc == 0) == ok, (n_lights, with_d_light, rc)
        if not ok:
            assert 'too many lights (%d)' % n_lights in nfx_lib.last_error()
