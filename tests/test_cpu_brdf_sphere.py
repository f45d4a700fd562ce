"""The host side of the sphere preview of the BRDF prior against tests/golden/reference_sphere.npz, which the reference's own
SphereRenderer / MERL wrote (tests/golden/make_reference_sphere_golden.py): scene geometry, light probes, light contributions,
the analytic render, the characteristic slice, and the id list that the data set and explore_brdf_space share.  float64
against float64: 1e-12 relative.  (The front-lit rows' Rusinkiewicz coordinates are stored as float32 to keep the fixture
under 1 MiB — they are compared at float32's spacing row by row, and through their float64 per-sample sums at 1e-12.)"""
import os

import numpy as np
import pytest

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_sphere.npz'))
SCENES = {'a': (16, 1), 'b': (6, 4)}
PROBES = {'point': 40., 'white': 1.}
COUNTS = {'a': (124, 31646), 'b': (80, 20410)}
RTOL = 1e-12


def close(got, want, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max() if got.size else 0.
    assert err <= rtol * max(1., np.abs(want).max()), err


_CACHE = {}


def renderer(s, probe):
    from nerfactor_amd.brdf.renderer import SphereRenderer
    if (s, probe) not in _CACHE:
        ims, spp = SCENES[s]
        _CACHE[s, probe] = SphereRenderer(probe, envmap_inten=PROBES[probe], envmap_h=None, ims=ims, spp=spp)
    return _CACHE[s, probe]


@pytest.mark.parametrize('probe', sorted(PROBES))
def test_load_light_equals_the_reference(probe):
    from nerfactor_amd.brdf.renderer import load_light
    got = load_light(probe, envmap_inten=PROBES[probe])
    assert got.dtype == np.float64 and np.array_equal(got, GOLD['light_' + probe])
    if probe == 'point':
        assert int((got != 0).any(2).sum()) == 16
        h8 = load_light('point', envmap_h=8)       # the negative-index block at another size
        want = np.zeros((8, 16, 3))
        want[-2 - 2:-2 + 2, -14 - 2:-14 + 2] = 1
        assert np.array_equal(h8, want)


@pytest.mark.parametrize('s', sorted(SCENES))
def test_scene_geometry_equals_the_reference(s):
    from nerfactor_amd.brdf import merl
    r = renderer(s, 'point')
    fg = GOLD[s + '_is_fg']
    assert np.array_equal(r.is_fg, fg) and int(fg.sum()) == COUNTS[s][0]
    close(r.cam_loc, GOLD['cam_loc'])
    close(r.xyz[fg], GOLD[s + '_xyz'])
    close(r.normal[fg], GOLD[s + '_normal'])
    radii = np.linalg.norm(r.xyz[fg], axis=1)     # "close to, but not exactly" the sphere's 0.4
    # (the depth comes from the sample grid, the lateral position from the back-projection's pixel centres at that depth)
    assert np.all(np.abs(radii - 0.4) < 0.02) and np.abs(radii - 0.4).max() > 1e-6
    assert np.all(r.xyz[~fg] == 0)
    lvis = r.lvis.astype(bool)
    want_lvis = np.unpackbits(GOLD[s + '_lvis'])[:fg.sum() * 512].reshape(-1, 512).astype(bool)
    assert np.array_equal(lvis[fg], want_lvis) and not lvis[~fg].any() and int(lvis.sum()) == COUNTS[s][1]
    assert np.array_equal(r.lcos > 0, lvis | (~fg[:, :, None] & (r.lcos > 0)))
    full = merl.dir2rusink(r.ldir, r.vdir)
    rows = full[lvis]
    want = GOLD[s + '_rusink']
    assert rows.shape == want.shape
    assert np.abs(rows - want).max() <= 2.4e-7     # half a float32 spacing at pi
    close(np.where(lvis[..., None], full, 0.).sum(2)[fg], GOLD[s + '_rusink_sum'])
    # the kernels take (light, view), the reference's tooling (view, light): the same angles on these scenes
    assert np.abs(merl.directions_to_rusink(r.ldir[lvis], np.broadcast_to(r.vdir[:, :, None], r.ldir.shape)[lvis]) - rows).max() < 1e-12
    assert min(rows[:, 0].min(), np.pi - rows[:, 0].max()) > 1e-3   # no row on the phi_d wrap


@pytest.mark.parametrize('probe', sorted(PROBES))
@pytest.mark.parametrize('s', sorted(SCENES))
def test_light_contributions_and_analytic_render(s, probe):
    from nerfactor_amd.brdf import merl
    r = renderer(s, probe)
    fg, lvis = r.is_fg, r.lvis.astype(bool)
    assert r.lcontrib.shape == lvis.shape + (3,)
    close(r.lcontrib.sum(2)[fg], GOLD['%s_%s_lcontrib_sum' % (s, probe)])
    assert np.all(r.lcontrib[~lvis] == 0)
    dark = ~(r.lcontrib.sum(3) != 0).any(2) & fg
    assert int(dark.sum()) == ({'a': 5, 'b': 4}[s] if probe == 'point' else 0)     # the kernel's exact-zero pixels
    theta_h = merl.dir2rusink(r.ldir, r.vdir)[..., 1]
    brdf = np.where(lvis, 0.1 + np.cos(theta_h) ** 8, 0.)[..., None]
    want = GOLD['%s_%s_render_analytic' % (s, probe)]
    assert want.shape == (SCENES[s][0],) * 2 + (3,)
    close(r.render(brdf), want)
    close(r.render(np.repeat(brdf, 3, axis=3), white_bg=False)[0, 0], np.zeros(3))
    assert np.all(r.render(brdf)[0, 0] == 1.)


def test_characteristic_slice():
    from nerfactor_amd.brdf import merl
    coords = merl.characteristic_slice_rusink()
    assert coords.shape == (90, 90, 3)
    close(coords, GOLD['cslice_rusink'])
    img = merl.characteristic_slice_as_img(GOLD['prior_cslice'])
    assert img.dtype == np.uint8 and np.array_equal(img, GOLD['prior_cslice_img'])


def test_spp_must_be_a_square():
    from nerfactor_amd.brdf.renderer import SphereRenderer
    with pytest.raises(ValueError):
        SphereRenderer('white', ims=4, spp=2)


def test_the_shared_id_list_is_the_data_sets(tmp_path):
    """datasets/brdf_merl.py:split_test_identities on a three-material toy root: what the data set's test split listed before the
    list moved into a function (seen materials, then the RandomState(0) walk, 11 steps per leg), and still lists."""
    import configparser
    from nerfactor_amd.nerfactor.datasets import brdf_merl
    names = ['alum-bronze', 'blue_rubber', 'pvc']
    for n in names:
        np.savez(tmp_path / ('train_%s.npz' % n), name=n)
    np.savez(tmp_path / 'test.npz', rusink=np.zeros((4, 3), np.float32), envmap_h=16, ims=4, spp=1)
    ids = brdf_merl.split_test_identities(names)
    mats = np.random.RandomState(0).choice(names, 3, replace=False)
    want = list(names)
    k = 0
    for leg in range(2):
        for a in np.linspace(1, 0, 11, endpoint=True):
            want.append('%06d_%f_%s_%f_%s' % (k, a, mats[leg], 1 - a, mats[leg + 1]))
            k += 1
    assert ids == want and len(ids) == 3 + 22
    assert ids[3].startswith('000000_1.000000_') and ids[13].split('_', 2)[1] == '0.000000'
    cfg = configparser.ConfigParser()
    cfg['DEFAULT'] = {'data_root': str(tmp_path), 'n_rays_per_step': '4'}
    ds = brdf_merl.Dataset.__new__(brdf_merl.Dataset)
    try:
        brdf_merl.Dataset.__init__(ds, cfg, 'test', device='cpu')
    except Exception:        # the base class may want more of the config than this toy has: the list is built before that
        pass
    assert ds.paths['test'] == want and ds.brdf_names == names
