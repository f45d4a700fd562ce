"""nfx_merl_query and nfx_merl_sphere_fwd (csrc/merl.hip), brdf.merl.MERL and data_gen.merl.make_dataset on the GPU, against
the reference's k-d tree and renders in tests/golden/reference_merl.npz (tests/golden/make_reference_merl_golden.py; the
material is tests/merl_cases.synthetic_cube(0), rebuilt here bit for bit).

1. the lookup is exact on four query sets;  2. degenerate tables and queries;  3. both kernels are position-independent, bit
for bit;  4. a fused pixel is the sum of its rows;  5. the fused kernel's rows are the reference's rows;  6. the renders against
the reference's float64 renders;  7. MERL.query / MERL.render_sphere;  8. the drivers;  9. the C-ABI's rejections.

Measured on an MI355X (profiles/merl/errors.txt): on every row of 1, 5 and 6 the kernels chose the k-d tree's entry itself —
no index differed, the largest distance excess was 0.0 rad; 4.: at most 0.071 of the bound; 6.: at most 0.032 of the tolerance,
PSNR 153 to 159 dB.

Set NFX_MERL_ERRORS to a file name and the figures these tests print are appended to it."""
import ctypes
import glob
import json
import os
from os.path import exists, join

import numpy as np
import pytest
import torch

from tests import common
from tests import merl_cases as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(join(HERE, 'golden', 'reference_merl.npz'))
SPHERE = np.load(join(HERE, 'golden', 'reference_sphere.npz'))
SCENES = {'a': (16, 1), 'b': (6, 4)}
PROBES = {'point': 40., 'white': 1.}
CAM = SPHERE['cam_loc'].astype(np.float32)
# 5.: the fused rows were measured on the GPU to be the reference's rows exactly (largest scaled excess 0.0 rad over both scenes
# and both probes); four times that, rounded up to the resolution of the lookup itself — the 1e-6 rad of 1., below which the
# fp32 grid coordinates cannot tell two entries apart.  It may not exceed 1e-4 rad.
ROW_MARGIN = 1e-6
assert ROW_MARGIN <= 1e-4


def record(line):
    print(line)
    if os.environ.get('NFX_MERL_ERRORS'):
        with open(os.environ['NFX_MERL_ERRORS'], 'a') as h:
            h.write(line + '\n')


def dev(a, cuda, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(cuda)


class Material:
    """synthetic_cube(0) as a MERL object, its host tables and the device tables."""
    def __init__(self, cuda):
        from nerfactor_amd.brdf import merl
        self.m = merl.MERL()
        self.m.cube_rgb = mc.synthetic_cube(0)
        self.m.name = 'synth0'
        self.valid = self.m.valid
        self.host = {a: self.m.packed_table(achromatic=a) for a in (False, True)}
        self.dev = {a: self.m.device_table(cuda, achromatic=a) for a in (False, True)}


@pytest.fixture(scope='module')
def mat(nfx_lib, cuda):
    return Material(cuda)


@pytest.fixture(scope='module')
def scenes():
    """(scene, probe) -> the float64 host renderer; per scene the float64 rows dir2rusink(ldir, vdir)[fg] and lvis[fg]."""
    from nerfactor_amd.brdf import merl
    from nerfactor_amd.brdf.renderer import SphereRenderer
    out = {}
    for s, (ims, spp) in SCENES.items():
        for probe, inten in PROBES.items():
            out[s, probe] = SphereRenderer(probe, envmap_inten=inten, envmap_h=None, ims=ims, spp=spp)
        r = out[s, 'white']
        out[s] = (merl.dir2rusink(r.ldir, r.vdir)[r.is_fg], r.lvis[r.is_fg] > 0)
    return out


def run_sphere(r, table, cuda, return_idx=False, pick=None):
    from nerfactor_amd import ops
    sc = r.device_scene(cuda)
    sel = (lambda t: t) if pick is None else (lambda t: t[torch.as_tensor(pick, device=cuda)].contiguous())
    return ops.merl_sphere_fwd(sel(sc['xyz']), sel(sc['normal']), r.cam_loc, table, sc['lxyz'], sc['lweight'], return_idx=return_idx)


def dist_to(q64, idx):
    return np.linalg.norm(q64 - mc.grid_rusink(idx), axis=1)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('name', ['cslice', 'uniform', 'outside', 'scene'])
def test_lookup_is_exact(mat, cuda, name):
    """Every row: idx is a valid entry, rgb is table[idx] bit for bit, and the float64 distance from the query (float32 ->
    float64) to entry idx is within 1e-6 rad of the k-d tree's nearest distance — the fp32 grid coordinates carry at most
    pi 2^-24 = 1.9e-7 per axis and the squared-distance arithmetic a few ulp on top.  idx may differ from the tree's only where
    the second neighbour is within 2e-6 of the first; a grid point whose own cell is valid returns that cell."""
    from nerfactor_amd import ops
    q = mc.query_sets(SPHERE['a_rusink'])[name]
    rgb, idx = ops.merl_query(mat.dev[False], dev(q, cuda), return_idx=True)
    rgb, idx = rgb.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    assert idx.shape == (q.shape[0],) and (idx >= 0).all() and (idx < mc.N_CELLS).all()
    assert mat.valid[idx].all()
    assert np.array_equal(rgb.view(np.uint32), mat.host[False][idx, :3].view(np.uint32))
    ref_idx, ref_dist, gap = GOLD['q_%s_idx' % name].astype(np.int64), GOLD['q_%s_dist' % name], GOLD['q_%s_gap' % name]
    excess = dist_to(q.astype(np.float64), idx) - ref_dist
    differ = idx != ref_idx
    record("lookup %-8s rows %6d  idx differs from the tree's on %d rows (%d of them with a second neighbour beyond 2e-6)  "
           "largest distance excess %.3e rad" % (name, q.shape[0], differ.sum(), (differ & (gap >= 2e-6)).sum(), excess.max()))
    assert excess.max() <= 1e-6
    assert not (differ & (gap >= 2e-6)).any()
    if name == 'cslice':
        own = mc.cslice_queries()[1]
        assert np.array_equal(idx[mat.valid[own]], own[mat.valid[own]])
    # the achromatic table answers with the same entries
    rgb_a, idx_a = ops.merl_query(mat.dev[True], dev(q, cuda), return_idx=True)
    assert np.array_equal(idx_a.cpu().numpy(), idx)
    assert np.array_equal(rgb_a.cpu().numpy().view(np.uint32), mat.host[True][idx, :3].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2
def test_degenerate_tables_and_queries(nfx_lib, cuda):
    from nerfactor_amd import ops
    from nerfactor_amd.brdf import merl
    q = np.concatenate((mc.uniform_queries(48, salt=77), mc.outside_queries(2, salt=99), mc.cslice_queries()[0][[0, 4000, 8000, 8099]]))
    assert q.shape == (64, 3)
    qd = dev(q, cuda)
    m = merl.MERL()
    # one valid entry in the whole cube: in a corner, in the opposite corner, in the middle
    for flat in (0, mc.N_CELLS - 1, (90 * 90 + 45) * 90 + 45):
        cube = np.full((180, 90, 90, 3), -1.)
        cube.reshape(-1, 3)[flat] = (.5, .25, .125)
        m.cube_rgb = cube
        rgb, idx = ops.merl_query(m.device_table(cuda), qd, return_idx=True)
        assert bool((idx == flat).all()), flat
        assert np.array_equal(rgb.cpu().numpy(), np.tile(np.float32((.5, .25, .125)), (64, 1)))
    # all entries valid: the per-axis nearest cell (where the fp32 and the float64 grid agree on it: not within 1e-6 of a tie)
    m.cube_rgb = np.ones((180, 90, 90, 3)) * np.arange(1, 4)
    rgb, idx = ops.merl_query(m.device_table(cuda), qd, return_idx=True)
    idx = idx.cpu().numpy().astype(np.int64)
    q64 = q.astype(np.float64)
    assert (dist_to(q64, idx) <= dist_to(q64, mc.nearest_cell(q64)) + 1e-6).all()
    assert np.array_equal(rgb.cpu().numpy(), np.tile(np.float32((1, 2, 3)), (64, 1)))
    # non-finite queries: idx -1, rgb NaN; their neighbours in the launch are untouched
    bad = q.copy()
    bad[3, 0], bad[17, 1], bad[40, 2], bad[63] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 0.)
    rows = [3, 17, 40, 63]
    rgb_b, idx_b = ops.merl_query(m.device_table(cuda), dev(bad, cuda), return_idx=True)
    idx_b, rgb_b = idx_b.cpu().numpy(), rgb_b.cpu().numpy()
    assert (idx_b[rows] == -1).all() and np.isnan(rgb_b[rows]).all()
    keep = np.setdiff1d(np.arange(64), rows)
    assert np.array_equal(idx_b[keep], idx[keep]) and np.array_equal(rgb_b[keep], rgb.cpu().numpy()[keep])
    # n = 0 is a no-op
    rgb0, idx0 = ops.merl_query(m.device_table(cuda), torch.empty((0, 3), device=cuda), return_idx=True)
    assert rgb0.shape == (0, 3) and idx0.shape == (0,)
    torch.cuda.synchronize()
    # a table without a valid entry is refused on the host
    m.cube_rgb = np.full((180, 90, 90, 3), -1.)
    with pytest.raises(ValueError, match='no valid entry'):
        m.device_table(cuda)


# ------------------------------------------------------------------------------------------------ 3
def test_both_kernels_are_position_independent_bit_for_bit(mat, scenes, cuda):
    from nerfactor_amd import ops
    q = dev(SPHERE['a_rusink'], cuda)
    n = q.shape[0]
    rgb, idx = ops.merl_query(mat.dev[False], q, return_idx=True)
    rev = torch.arange(n - 1, -1, -1, device=cuda)
    rgb_r, idx_r = ops.merl_query(mat.dev[False], q[rev].contiguous(), return_idx=True)
    common.assert_same_bits(rgb[rev], rgb_r, "merl_query, rows reversed")
    assert torch.equal(idx[rev], idx_r)
    slow = np.nonzero(~mat.valid[mc.nearest_cell(SPHERE['a_rusink'].astype(np.float64))])[0]
    for k in (1, 63, 64, 65):
        for start in (0, min(int(slow[0]), n - k), int(slow[-1]) - k + 1, n - k):      # windows that hold rows of the cooperative search too
            rgb_k, idx_k = ops.merl_query(mat.dev[False], q[start:start + k].contiguous(), return_idx=True)
            common.assert_same_bits(rgb[start:start + k], rgb_k, "merl_query, rows %d..%d alone" % (start, start + k))
            assert torch.equal(idx[start:start + k], idx_k)
    r = scenes['a', 'white']
    assert r.lxyz.reshape(-1, 3).shape[0] == 512
    full, full_idx = run_sphere(r, mat.dev[False], cuda, return_idx=True)
    ns = full.shape[0]
    assert ns > 65 and bool(torch.isfinite(full).all())
    order = np.arange(ns)[::-1].copy()
    got, got_idx = run_sphere(r, mat.dev[False], cuda, return_idx=True, pick=order)
    common.assert_same_bits(full[torch.as_tensor(order, device=cuda)], got, "merl_sphere_fwd, samples reversed")
    assert torch.equal(full_idx[torch.as_tensor(order, device=cuda)], got_idx)
    for k in (1, 63, 64, 65):
        for start in (0, ns - k):
            pick = np.arange(start, start + k)
            got = run_sphere(r, mat.dev[False], cuda, pick=pick)
            common.assert_same_bits(full[start:start + k], got, "merl_sphere_fwd, samples %d..%d alone" % (start, start + k))


# ------------------------------------------------------------------------------------------------ 4
def kernel_cos(r):
    """The cosine of every (foreground sample, light) pair as the kernel computes it, statement for statement in float32
    (geom.hpp: dir_to, the normal's row of world2local, mat3_apply; the library is built without contraction, its division
    and square root are correctly rounded, so NumPy's float32 operations are the same bits).  The float64 cosine will not do
    here: at grazing light it differs from the fp32 one by the geometry's conditioning (1e-7 absolute on a cosine of 1e-2),
    which is neither the product nor the sum that 4. bounds."""
    f = np.float32
    fg = r.is_fg
    x, n, l = r.xyz[fg].astype(f), r.normal[fg].astype(f), r.lxyz.reshape(-1, 3).astype(f)

    def normalize3(v):
        d = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
        return v * (f(1) / np.sqrt(np.maximum(d, f(1e-6))))[..., None]
    nn = normalize3(n)
    ldir = normalize3(l[None, :, :] - x[:, None, :])
    lz = nn[:, None, 0] * ldir[..., 0] + nn[:, None, 1] * ldir[..., 1] + nn[:, None, 2] * ldir[..., 2]
    assert lz.dtype == f
    return lz.astype(np.float64)


@pytest.mark.parametrize('probe', sorted(PROBES))
@pytest.mark.parametrize('s', sorted(SCENES))
def test_a_fused_pixel_is_the_sum_of_its_rows(mat, scenes, cuda, s, probe):
    """With dev_idx: each sample equals the float64 sum of table[idx] lweight cos (kernel_cos) over its rows to within an fp32
    product and an m-term fp32 sum, (m + 8) 2^-23 sum |terms|; the rows with idx >= 0 are the lit front-facing rows of the float64
    renderer (but for |l.z| < 1e-6); and rgb is the same bits with and without dev_idx."""
    r = scenes[s, probe]
    rgb, idx = run_sphere(r, mat.dev[False], cuda, return_idx=True)
    common.assert_same_bits(rgb, run_sphere(r, mat.dev[False], cuda), "merl_sphere_fwd with and without dev_idx")
    rgb, idx = rgb.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    fg = r.is_fg
    lweight = (r.light.reshape(-1, 3) * r.lareas.reshape(-1, 1)).astype(np.float32).astype(np.float64)
    lit = (lweight != 0).any(1)
    want_set = (r.lvis[fg] > 0) & lit[None, :]
    edge = np.abs(r.lcos[fg]) < 1e-6
    assert np.array_equal((idx >= 0) | edge, want_set | edge)
    assert mat.valid[idx[idx >= 0]].all()
    cos = kernel_cos(r)
    assert np.abs(cos - r.lcos[fg]).max() < 1e-6
    tab = mat.host[False][:, :3].astype(np.float64)
    terms = np.where((idx >= 0)[..., None], tab[np.maximum(idx, 0)] * lweight[None] * cos[..., None], 0.)
    m = (idx >= 0).sum(1)
    bound = (m + 8)[:, None] * 2. ** -23 * np.abs(terms).sum(1)
    err = np.abs(rgb - terms.sum(1))
    worst = float((err / np.where(bound > 0, bound, 1.))[bound > 0].max()) if (bound > 0).any() else 0.
    record("fused sample - sum of its rows (%s, %s): worst error / bound %.3f" % (s, probe, worst))
    assert np.all(err <= bound)
    assert np.all(rgb[m == 0] == 0.)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize('probe', sorted(PROBES))
@pytest.mark.parametrize('s', sorted(SCENES))
def test_fused_rows_are_the_references_rows(mat, scenes, cuda, s, probe):
    """For each contributing row: the float64 distance from brdf.merl.dir2rusink's float64 coordinate to the entry the kernel
    chose, minus the distance to the k-d tree's entry, scaled by 1 / (1 + 1 / sin theta_d) (phi_d is conditioned by
    sin theta_d), is at most ROW_MARGIN."""
    r = scenes[s, probe]
    _, idx = run_sphere(r, mat.dev[False], cuda, return_idx=True)
    idx = idx.cpu().numpy().astype(np.int64)
    rows, lvis = scenes[s]
    ref = np.full(lvis.shape, -1, dtype=np.int64)
    ref[lvis] = GOLD[s + '_ref_idx']
    sel = (idx >= 0) & lvis
    q = rows[sel]
    excess = (dist_to(q, idx[sel]) - dist_to(q, ref[sel])) / (1. + 1. / np.sin(q[:, 2]))
    record("fused rows vs the tree's (%s, %s): %d rows, %d with another entry, largest scaled distance excess %.3e rad, "
           "smallest theta_d %.3f" % (s, probe, q.shape[0], (idx[sel] != ref[sel]).sum(), excess.max(), q[:, 2].min()))
    assert excess.max() <= ROW_MARGIN


def pixels(r, per_sample_fg, background):
    """[ims, ims, 3] mean over a pixel's samples of a per-foreground-sample quantity [n_fg, 3], `background` elsewhere."""
    full = np.full(r.is_fg.shape + (3,), float(background))
    full[r.is_fg] = per_sample_fg
    return full.reshape(r.ims, r.sps, r.ims, r.sps, 3).sum(axis=(1, 3)) / r.sps ** 2


def averaging_bound(r, magnitude_fg):
    """The fp32 mean over a pixel's sps^2 samples (SphereRenderer.assemble), background samples being 1: sps^2 roundings of
    the sum and one of the division, relative to the mean magnitude."""
    return (r.sps ** 2 + 1) * 2. ** -24 * pixels(r, magnitude_fg, 1.)


# ------------------------------------------------------------------------------------------------ 6
def neighbourhood_range(tab, valid, flat):
    """[n, 3]: max - min of the table over the valid entries of the 3 x 3 x 3 neighbourhood of each entry `flat`."""
    i, j, k = flat // 8100, (flat // 90) % 90, flat % 90
    hi = np.full((flat.shape[0], 3), -np.inf)
    lo = np.full((flat.shape[0], 3), np.inf)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for dk in (-1, 0, 1):
                nb = (np.clip(i + di, 0, 179) * 90 + np.clip(j + dj, 0, 89)) * 90 + np.clip(k + dk, 0, 89)
                ok = valid[nb][:, None]
                hi = np.where(ok, np.maximum(hi, tab[nb]), hi)
                lo = np.where(ok, np.minimum(lo, tab[nb]), lo)
    return hi - lo


@pytest.mark.parametrize('achro', [False, True])
@pytest.mark.parametrize('probe', sorted(PROBES))
@pytest.mark.parametrize('s', sorted(SCENES))
def test_renders_against_the_references(mat, scenes, cuda, s, probe, achro):
    """Per pixel |gpu - ref| <= sum_l |lcontrib_l| (max - min of the table over the 3 x 3 x 3 valid neighbourhood of the
    reference's entry: a row can only land in an adjacent cell) + the fp32 bound (m + 8) 2^-23 sum_l |lcontrib_l table|, both
    averaged over the pixel's samples, + the fp32 rounding of that average."""
    r = scenes[s, probe]
    got = mat.m.render_sphere(r, achromatic=achro, device=cuda)
    assert got.is_cuda and got.shape == (r.ims, r.ims, 3)
    got = got.cpu().numpy().astype(np.float64)
    want = GOLD['%s_%s_render%s' % (s, probe, '_achromatic' if achro else '')]
    tab = mat.host[achro][:, :3].astype(np.float64)
    _, lvis = scenes[s]
    ref_idx = GOLD[s + '_ref_idx'].astype(np.int64)
    rng_rows = np.zeros(lvis.shape + (3,))
    rng_rows[lvis] = neighbourhood_range(tab, mat.valid, ref_idx)
    val_rows = np.zeros(lvis.shape + (3,))
    val_rows[lvis] = tab[ref_idx]
    lc = np.abs(r.lcontrib[r.is_fg])
    m = (lc != 0).any(2).sum(1)
    tol_fg = (lc * rng_rows).sum(1) + (m + 8)[:, None] * 2. ** -23 * (lc * val_rows).sum(1)
    tol = pixels(r, tol_fg, 0.) + averaging_bound(r, (lc * val_rows).sum(1))
    err = np.abs(got - want)
    mse = float(np.mean(np.square(np.clip(got, 0, 1) - np.clip(want, 0, 1))))
    record("render vs the reference (%s, %s%s): max error %.3e, max error / tolerance %.3f, PSNR %s dB"
           % (s, probe, ', achromatic' if achro else '', err.max(), (err / np.maximum(tol, 1e-300))[tol > 0].max(),
              'inf' if mse == 0 else '%.1f' % (10 * np.log10(1 / mse))))
    assert np.all(err <= tol)
    assert np.all(got[0, 0] == 1.)                                     # white background
    black = mat.m.render_sphere(r, achromatic=achro, white_bg=False, device=cuda)
    assert np.all(black[0, 0].cpu().numpy() == 0.)


# ------------------------------------------------------------------------------------------------ 7
def test_merl_query_and_render_sphere_plumbing(mat, scenes, cuda):
    from nerfactor_amd.brdf import merl
    q = mc.uniform_queries(100, salt=5)
    out_np = mat.m.query(q)
    assert isinstance(out_np, np.ndarray) and out_np.shape == (100, 3)
    out_t = mat.m.query(dev(q, cuda))
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and out_t.shape == (100, 3)
    assert np.array_equal(out_np, out_t.cpu().numpy())
    assert mat.m.device_table(cuda) is mat.m.device_table(cuda)          # built once
    lum = mat.m.query(dev(q, cuda), achromatic=True).cpu().numpy()
    assert np.all(lum[:, 0] == lum[:, 1]) and np.all(lum[:, 0] == lum[:, 2])
    # the Lambertian material renders sum lcontrib, as SphereRenderer.render(ones) does, to the fp32 sum bound
    lamb = merl.MERL()
    for s in sorted(SCENES):
        for probe in sorted(PROBES):
            r = scenes[s, probe]
            got = lamb.render_sphere(r, device=cuda).cpu().numpy().astype(np.float64)
            want = r.render(np.ones(r.lcontrib.shape[:3] + (1,)))
            lc = np.abs(r.lcontrib[r.is_fg])
            m = (lc != 0).any(2).sum(1)
            bound = pixels(r, (m + 8)[:, None] * 2. ** -23 * lc.sum(1), 0.) + averaging_bound(r, lc.sum(1))
            assert np.all(np.abs(got - want) <= bound), (s, probe)


# ------------------------------------------------------------------------------------------------ 8
def test_make_dataset_and_explore_with_measured_spheres(nfx_lib, cuda, tmp_path):
    from PIL import Image
    from nerfactor_amd.brdf import merl
    from nerfactor_amd.data_gen.merl import make_dataset
    from nerfactor_amd.nerfactor import explore_brdf_space
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    from nerfactor_amd.nerfactor.models import get_model_class
    indir = tmp_path / 'binary'
    os.makedirs(indir)
    for seed, name in ((0, 'synth0'), (1, 'synth1')):
        merl.write_merl_binary(str(indir / (name + '.binary')), mc.synthetic_cube(seed))
    (indir / 'readme.txt').write_text('not a table')
    root = str(tmp_path / 'data')
    assert make_dataset.main(['--indir', str(indir / '*'), '--outdir', root, '--ims', '16']) == root
    files = sorted(os.path.relpath(p, root) for p in glob.glob(join(root, '**', '*'), recursive=True) if os.path.isfile(p))
    want_files = sorted(['test.npz'] + ['%s_%s.npz' % (sp, n) for sp in ('train', 'vali') for n in ('synth0', 'synth1')]
                        + [join('vis', d, n + '.png') for d in ('cslice', 'cslice_achromatic', 'render', 'render_achromatic')
                           for n in ('synth0', 'synth1')])
    assert files == want_files
    assert [f for f in files if 'synth0' in f or f == 'test.npz'] == list(GOLD['ds_files'])
    test = np.load(join(root, 'test.npz'))
    assert sorted(test.files) == ['envmap_h', 'ims', 'rusink', 'spp'] and (int(test['envmap_h']), int(test['ims']), int(test['spp'])) == (16, 16, 1)
    assert test['rusink'].dtype == np.float32 and test['rusink'].shape == (int(GOLD['ds_test_n']), 3)
    assert np.abs(test['rusink'][::997] - GOLD['ds_test_rusink']).max() <= 2.4e-7
    for i, name in enumerate(('synth0', 'synth1')):
        for split in ('train', 'vali'):
            d = np.load(join(root, '%s_%s.npz' % (split, name)))
            assert sorted(d.files) == ['envmap_h', 'i', 'ims', 'name', 'refl', 'rusink', 'spp']
            assert int(d['i']) == i and str(d['name']) == name and d['refl'].shape == (d['rusink'].shape[0], 1)
            if name == 'synth0':
                assert d['rusink'].shape == (int(GOLD['ds_%s_n' % split]), 3)
                assert np.array_equal(d['rusink'][::997], GOLD['ds_%s_rusink' % split])
                assert np.array_equal(d['refl'][::997], GOLD['ds_%s_refl' % split])
    for d in ('cslice', 'cslice_achromatic', 'render', 'render_achromatic'):
        a, b = (np.asarray(Image.open(join(root, 'vis', d, n + '.png'))) for n in ('synth0', 'synth1'))
        assert a.shape == b.shape == ((90, 90, 3) if 'cslice' in d else (16, 16, 3)) and not np.array_equal(a, b), d
    grey = np.asarray(Image.open(join(root, 'vis', 'render_achromatic', 'synth0.png')))
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])
    # the data set reads what the driver wrote
    cfg = make_config('brdf', data_root=root, n_rays_per_step=64)
    tr = get_dataset_class('brdf_merl')(cfg, 'train', device='cpu')
    assert tr.brdf_names == ['synth0', 'synth1']
    batch = next(iter(tr.build_pipeline(no_batch=True, seed=0)))
    assert batch[5].shape == (64, 3) and batch[6].shape == (64, 1) and bool((batch[6] > 0).all())
    assert exists(join(make_dataset.main(['--indir', str(indir), '--outdir', root, '--ims', '16', '--overwrite']), 'vali_synth1.npz'))

    # explore_brdf_space: without --merl_dir the three files of today, with it render_measured.png and a PSNR besides
    torch.manual_seed(1)
    model = get_model_class('brdf')(cfg).to(cuda)
    model.latent_code._z.data.mul_(60.)
    ckpts = {}
    for run in ('plain', 'measured'):
        rd = tmp_path / run / 'lr1e-2'
        os.makedirs(rd / 'checkpoints')
        with open(str(rd) + '.ini', 'w') as h:
            cfg.write(h)
        ckpts[run] = str(rd / 'checkpoints' / 'ckpt-1')
        torch.save({'net': model.state_dict()}, ckpts[run])
    os.remove(str(indir / 'synth1.binary'))                               # only synth0 is found
    plain = explore_brdf_space.main(['--ckpt=' + ckpts['plain'], '--ims', '16', '--batch', '4'])
    meas = explore_brdf_space.main(['--ckpt=' + ckpts['measured'], '--ims', '16', '--batch', '4', '--merl_dir', str(indir)])
    pd, md = sorted(glob.glob(join(plain, 'batch*'))), sorted(glob.glob(join(meas, 'batch*')))
    assert len(pd) == len(md) == 2 + 11
    for k, (a, b) in enumerate(zip(pd, md)):
        assert sorted(os.listdir(a)) == sorted(explore_brdf_space.EXPECTS)
        assert sorted(os.listdir(b)) == sorted(explore_brdf_space.EXPECTS + (('render_measured.png',) if k == 0 else ()))
        for f in ('cslice.png', 'render.png'):
            assert open(join(a, f), 'rb').read() == open(join(b, f), 'rb').read()
        ma, mb = json.load(open(join(a, 'metadata.json'))), json.load(open(join(b, 'metadata.json')))
        assert sorted(ma) == ['id', 'z']
        assert open(join(a, 'metadata.json')).read() == json.dumps(ma, indent=4, sort_keys=True)
        if k == 0:
            assert sorted(mb) == ['id', 'psnr_measured', 'z'] and np.isfinite(mb['psnr_measured']) and mb['psnr_measured'] > 0
            assert np.asarray(Image.open(join(b, 'render_measured.png'))).shape == (16, 16, 3)
        else:
            assert open(join(a, 'metadata.json')).read() == open(join(b, 'metadata.json')).read()


# ------------------------------------------------------------------------------------------------ 9
def test_the_c_abi_rejects_bad_arguments(mat, scenes, cuda):
    nfx_lib = __import__('nerfactor_amd._capi', fromlist=['_capi'])
    lib = nfx_lib.lib
    r = scenes['a', 'white']
    sc = r.device_scene(cuda)
    xyz, normal = sc['xyz'][:3].contiguous(), sc['normal'][:3].contiguous()
    pad = torch.zeros((mc.N_CELLS * 4 + 4,), dtype=torch.float32, device=cuda)
    pad[1:1 + mc.N_CELLS * 4] = mat.dev[False].reshape(-1)
    misaligned = pad[1:1 + mc.N_CELLS * 4]
    assert misaligned.data_ptr() % 16 == 4
    q = dev(mc.uniform_queries(3, salt=1), cuda)
    out = torch.full((3, 3), 7., device=cuda)
    oidx = torch.full((3,), 7, dtype=torch.int32, device=cuda)
    cam = (ctypes.c_float * 3)(*CAM.tolist())
    camp = ctypes.cast(cam, ctypes.c_void_p)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def query(table=mat.dev[False], rusink=q, n=3, rgb=out):
        return lib.nfx_merl_query(ptr(table), ptr(rusink), n, ptr(rgb), ptr(oidx), None)

    def sphere(xyz=xyz, normal=normal, n=3, cam=camp, table=mat.dev[False], lxyz=sc['lxyz'], lweight=sc['lweight'], n_lights=512, rgb=out):
        return lib.nfx_merl_sphere_fwd(ptr(xyz), ptr(normal), n, cam, ptr(table), ptr(lxyz), ptr(lweight), n_lights, ptr(rgb), None, None)

    for fn, name, cases in ((query, 'nfx_merl_query', (dict(table=None), dict(rusink=None), dict(rgb=None), dict(table=misaligned), dict(n=-1))),
                            (sphere, 'nfx_merl_sphere_fwd',
                             (dict(xyz=None), dict(normal=None), dict(cam=None), dict(table=None), dict(lxyz=None), dict(lweight=None),
                              dict(rgb=None), dict(table=misaligned), dict(n_lights=48), dict(n_lights=1056), dict(n_lights=0), dict(n=-1)))):
        for kw in cases:
            rc = fn(**kw)
            assert rc != 0, (name, kw)
            assert name in nfx_lib.last_error(), (name, kw, nfx_lib.last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.).all()) and bool((oidx == 7).all()), (name, kw)       # nothing was launched
        assert fn() == 0
        torch.cuda.synchronize()
        assert bool((out != 7.).all())
        out.fill_(7.)
        if name == 'nfx_merl_query':
            assert bool((oidx != 7).all())
            oidx.fill_(7)
    # the Python layer refuses a table of another shape before the library sees it
    from nerfactor_amd import ops
    with pytest.raises(nfx_lib.NfxError):
        ops.merl_query(mat.dev[False][:100], q)
