"""nfx_brdf_sphere_fwd (csrc/brdf_sphere.hip), Model.render_spheres and explore_brdf_space on the GPU.

1. position-independence, bit for bit: a pixel depends on its own (identity, sample) pair and on nothing else in the launch;
2. against the shipped row kernel: the fused pixel is the float64 sum of nfx_brdf_spec_fwd's rows to within an fp32
   product and an m-term fp32 sum;
3. against the reference's own render of the same prior (tests/golden/reference_sphere.npz);
4. the fused and the explicit-row route agree;
5. the drivers; 6. the C-ABI's rejections."""
import ctypes
import glob
import json
import os
from os.path import exists, join

import numpy as np
import pytest
import torch

from oracle import nerfactor_ref as R
from tests import common
from tests.golden import golden_inputs as gi

pytestmark = pytest.mark.gpu
GOLD = np.load(join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_sphere.npz'))
SCENES = {'a': (16, 1), 'b': (6, 4)}
PROBES = {'point': 40., 'white': 1.}


def dev(a, cuda):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(cuda)


def net128(seed, zd):
    rng = np.random.default_rng(seed)
    layers, out = R.init_mlp128(rng, zd + 15, 1)
    for lst in (layers, out):
        for i, (k, b) in enumerate(lst):
            lst[i] = (k, rng.uniform(-.2, .2, size=b.shape).astype(np.float32))
    return layers, out


def pack(nfx_lib, layers, out, zd, cuda):
    from nerfactor_amd import ops
    ks = [k for k, _ in layers] + [out[0][0]]
    bs = [b for _, b in layers] + [out[0][1]]
    return ops.pack_mlp128_weights(ks, bs, nfx_lib.IN_Z_RUSINK, 1, z_dim=zd).to(cuda)


def samples(which):
    """(xyz, normal) float32 of the fixture scenes' foreground samples, or of the first 1 / 3 of scene 'a'."""
    if which in SCENES:
        return GOLD[which + '_xyz'].astype(np.float32), GOLD[which + '_normal'].astype(np.float32)
    x, n = samples('a')
    return x[40:40 + which], n[40:40 + which]


def lights(nl_h, kind):
    """(lxyz [L, 3], lweight [L, 3]) float32: L = nl_h x 2 nl_h lights, weight = light x area."""
    from nerfactor_amd.brdf.renderer import gen_light_xyz, load_light
    lxyz, areas = gen_light_xyz(nl_h, 2 * nl_h)
    L = lxyz.shape[0] * lxyz.shape[1]
    if kind in PROBES:
        light = load_light(kind, envmap_inten=PROBES[kind], envmap_h=nl_h).reshape(L, 3)
    elif kind == 'hdr':
        light = np.exp(np.random.default_rng(7).normal(size=(L, 3)))
    elif kind == 'zeros':
        light = np.zeros((L, 3))
    else:   # 'last': one single lit light, in the last 32-light tile (its green channel dark)
        light = np.zeros((L, 3))
        light[L - 5] = (3., 0., .5)
    return lxyz.reshape(L, 3).astype(np.float32), (light * areas.reshape(L, 1)).astype(np.float32)


CAM = GOLD['cam_loc'].astype(np.float32)


def front_cos(xyz, normal, lxyz):
    """float64 cosine of every (sample, light) pair in the sample's local frame, from the oracle's gen_world2local."""
    x, n, l = xyz.astype(np.float64), normal.astype(np.float64), lxyz.astype(np.float64)
    return np.einsum('nij,nlj->nli', R.gen_world2local(n), R.calc_ldir(x, l))[..., 2]


class Case:
    def __init__(self, nfx_lib, cuda, which, nl_h, kind, zd, n_iden, seed=3):
        self.xyz, self.normal = samples(which)
        self.lxyz, self.lweight = lights(nl_h, kind)
        self.zd, self.cuda = zd, cuda
        self.z = np.random.default_rng(seed).normal(0, .6, (n_iden, zd)).astype(np.float32)
        self.blob = pack(nfx_lib, *net128(60 + zd, zd), zd, cuda)
        self.d = {k: dev(getattr(self, k), cuda) for k in ('xyz', 'normal', 'lxyz', 'lweight', 'z')}

    def run(self, si=None, bi=None, out=None):
        from nerfactor_amd import ops
        d = self.d
        pick = lambda t, idx: t if idx is None else t[torch.as_tensor(idx, device=self.cuda)].contiguous()
        return ops.brdf_sphere_fwd(pick(d['xyz'], si), pick(d['normal'], si), CAM, pick(d['z'], bi), d['lxyz'], d['lweight'],
                                   self.blob, out=out)


# ------------------------------------------------------------------------------------------------ 1
CASES = [('a', 16, 'point', 3, 11), ('b', 16, 'white', 3, 3), ('a', 8, 'hdr', 1, 3), ('b', 16, 'last', 1, 1),
         (3, 8, 'point', 3, 11), (1, 16, 'hdr', 3, 1), ('a', 16, 'zeros', 3, 3), (3, 8, 'last', 1, 3)]


@pytest.mark.parametrize('which,nl_h,kind,zd,n_iden', CASES)
def test_a_pixel_depends_on_its_own_pair_only(nfx_lib, cuda, nfx_opt, which, nl_h, kind, zd, n_iden):
    c = Case(nfx_lib, cuda, which, nl_h, kind, zd, n_iden)
    n = c.xyz.shape[0]
    full = c.run()
    assert full.shape == (n_iden, n, 3) and bool(torch.isfinite(full).all())
    # poisoned output buffers: every element is written, and to the same bits
    for byte in (0xFF, 0x00):
        buf = torch.empty((n_iden, n, 3), dtype=torch.float32, device=cuda)
        buf.view(torch.uint8).fill_(byte)
        common.assert_same_bits(full, c.run(out=buf), "output buffer pre-filled with 0x%02X" % byte)
    # every pair launched alone
    alone = torch.empty_like(full)
    for b in range(n_iden):
        for i in range(n):
            alone[b, i] = c.run([i], [b])[0, 0]
    common.assert_same_bits(full, alone, "each (identity, sample) pair launched alone against the batch")
    # samples and identities reversed and shuffled
    rng = np.random.default_rng(11)
    for name, si, bi in (('reversed', np.arange(n)[::-1].copy(), np.arange(n_iden)[::-1].copy()),
                         ('shuffled', rng.permutation(n), rng.permutation(n_iden))):
        got = c.run(si, bi)
        want = full[torch.as_tensor(bi, device=cuda)][:, torch.as_tensor(si, device=cuda)]
        common.assert_same_bits(want, got, "samples and identities " + name)
    # 1 and 3 workgroups
    for blocks in (1, 3):
        nfx_opt.set('m128_blocks', blocks)
        common.assert_same_bits(full, c.run(), "m128_blocks = %d against the default grid" % blocks)
    nfx_opt.unset('m128_blocks')
    # pairs without a lit front-facing light are exact zeros; a pair with one (clear of the fp32 decision) is positive
    cos = front_cos(c.xyz, c.normal, c.lxyz)
    lit = (c.lweight != 0).any(1)
    surely_dark = ~((cos > -1e-4) & lit[None, :]).any(1)
    surely_lit = ((cos > 1e-4) & lit[None, :]).any(1)
    got = full.cpu().numpy()
    assert np.all(got[:, surely_dark] == 0.)
    if kind in ('point', 'white', 'hdr'):
        assert np.all(got[:, surely_lit].sum(-1) > 0.)
    if kind == 'zeros':
        assert np.all(got == 0.)
    if kind == 'last':
        assert np.all(got[..., 1] == 0.) and (surely_lit.any() == bool((got[..., 0] > 0).any()))
    if kind == 'point' and which == 'a':
        assert int(surely_dark.sum()) == 5      # the fixture's five samples that the block of lit lights does not reach


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('which,nl_h,kind,zd,n_iden', [c for c in CASES if c[2] != 'zeros'])
def test_the_fused_pixel_is_the_sum_of_the_row_kernels_rows(nfx_lib, cuda, which, nl_h, kind, zd, n_iden):
    """S = nfx_brdf_spec_fwd on the same samples with z[b] repeated; the float64 sum over lights of S * lweight * cos with the
    oracle's cosine; the fused pixel within (m + 8) 2^-23 sum |S lweight cos|, m = the sample's lit front-facing lights:
    the row values are the same bits, what is left is an fp32 product and an m-term fp32 sum."""
    from nerfactor_amd import ops
    c = Case(nfx_lib, cuda, which, nl_h, kind, zd, n_iden)
    n = c.xyz.shape[0]
    got = c.run().cpu().numpy().astype(np.float64)
    cos = front_cos(c.xyz, c.normal, c.lxyz)
    cam = dev(np.broadcast_to(CAM, (n, 3)), cuda)
    w = c.lweight.astype(np.float64)
    worst = 0.
    for b in range(n_iden):
        zb = c.d['z'][b:b + 1].expand(n, -1).contiguous()
        S = ops.brdf_spec_fwd(c.d['xyz'], cam, c.d['normal'], zb, c.d['lxyz'], c.blob).cpu().numpy().astype(np.float64)
        terms = S[:, :, None] * w[None, :, :] * cos[:, :, None]
        m = ((S > 0) & (w != 0).any(1)[None, :]).sum(1)
        bound = (m + 8)[:, None] * 2. ** -23 * np.abs(terms).sum(1)
        err = np.abs(got[b] - terms.sum(1))
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.), np.where(err > 0, np.inf, 0.))
        worst = max(worst, float(ratio.max()))
    print("fused pixel - sum of rows, worst error / bound: %.3f (%s, %d lights, %s, z_dim %d)" % (worst, which, 2 * nl_h * nl_h, kind, zd))
    assert worst <= 1., worst


# ------------------------------------------------------------------------------------------------ 3, 4
@pytest.fixture(scope='module')
def prior(nfx_lib, cuda, tmp_path_factory):
    """models.brdf.Model with the fixture's seeded glorot prior (golden_inputs.brdf_net, z_dim 3)."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    root = tmp_path_factory.mktemp('merl_names')
    for name in gi.BRDF_NAMES:
        (root / ('train_%s.npz' % name)).write_bytes(b'')
    torch.manual_seed(0)
    model = get_model_class('brdf')(make_config('brdf', data_root=str(root))).to(cuda)
    net = gi.brdf_net()
    for part in ('brdf_mlp', 'brdf_out'):
        for layer, (k, b) in zip(model.net[part].layers, net[part]):
            layer.kernel.data.copy_(torch.from_numpy(k))
            layer.bias.data.copy_(torch.from_numpy(b))
    assert model.tuned
    return model


def reference_tolerance(r, rows_max):
    """Per pixel and channel: 3e-2 max(1, max spec) sum |lcontrib| / sps^2 (the bound test_brdf_spec_vs_oracle holds every bf16
    row to, carried through the sum) + max spec sum_l lweight 1e-4 [|lcos| <= 1e-4] / sps^2 (lights whose front-lit decision
    may differ between fp32 and float64, each scaled by its cosine)."""
    s = r.sps
    pix = lambda a: a.reshape(r.ims, s, r.ims, s, 3).sum(axis=(1, 3)) / s ** 2
    lweight = r.light.reshape(-1, 3) * r.lareas.reshape(-1, 1)
    edge = (np.abs(r.lcos) <= 1e-4) & r.is_fg[:, :, None]
    return (3e-2 * max(1., rows_max) * pix(np.abs(r.lcontrib).sum(2))
            + rows_max * 1e-4 * pix((edge[..., None] * lweight[None, None]).sum(2)))


@pytest.mark.parametrize('probe', sorted(PROBES))
@pytest.mark.parametrize('s', sorted(SCENES))
def test_render_spheres_vs_the_reference(prior, cuda, s, probe):
    ims, spp = SCENES[s]
    z = dev(GOLD['prior_z'][None], cuda)
    got = prior.render_spheres(z, probe, PROBES[probe], None, ims, spp)
    assert got.is_cuda and got.shape == (1, ims, ims, 3)
    want = GOLD['%s_%s_render_prior' % (s, probe)]
    r = prior._sphere_scene(probe, PROBES[probe], None, ims, spp, cuda)['renderer']
    tol = reference_tolerance(r, float(GOLD[s + '_prior_rows'].max()))
    err = np.abs(got[0].cpu().numpy() - want)
    print("render_spheres vs the reference (%s, %s): max error %.3e, max error / tolerance %.3f"
          % (s, probe, err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol)
    assert np.all(got[0, 0, 0].cpu().numpy() == 1.)                   # white background
    black = prior.render_spheres(z, probe, PROBES[probe], None, ims, spp, white_bg=False)
    assert np.all(black[0, 0, 0].cpu().numpy() == 0.)


def test_the_fused_and_the_explicit_row_route_agree(prior, cuda):
    """Scene (16, 1), both probes: nfx_dir2rusink + nfx_brdf_rows_fwd (an independent kernel) + SphereRenderer.render on the
    host against the fused launch, within twice the tolerance of the comparison with the reference."""
    from nerfactor_amd import ops
    for probe in sorted(PROBES):
        z = dev(GOLD['prior_z'][None], cuda)
        fused = prior.render_spheres(z, probe, PROBES[probe], None, 16, 1)[0].cpu().numpy()
        r = prior._sphere_scene(probe, PROBES[probe], None, 16, 1, cuda)['renderer']
        lvis = r.lvis.astype(bool)
        si = np.nonzero(lvis)
        ldir, vdir = r.ldir[lvis], r.vdir[si[0], si[1]]
        rusink = ops.dir2rusink(dev(ldir, cuda), dev(vdir, cuda))
        rows = ops.brdf_rows_fwd(z.expand(rusink.shape[0], -1).contiguous(), rusink, prior._train_blob(), reci=False)
        brdf = np.zeros(lvis.shape + (1,))
        brdf[lvis] = rows.cpu().numpy().astype(np.float64)[:, None]
        explicit = r.render(brdf)
        tol = 2 * reference_tolerance(r, float(GOLD['a_prior_rows'].max()))
        err = np.abs(fused - explicit)
        print("fused vs explicit rows (%s): max error / tolerance %.3f" % (probe, (err / np.maximum(tol, 1e-300)).max()))
        assert np.all(err <= tol)


def test_characteristic_slices_vs_the_reference(prior, cuda):
    z = dev(np.stack((GOLD['prior_z'], gi.latent_codes()[0])), cuda)
    got = prior.characteristic_slices(z)
    assert got.shape == (2, 90, 90)
    want = GOLD['prior_cslice']
    assert np.abs(got[0].cpu().numpy() - want).max() < 3e-2 * max(1., want.max())     # the bf16 rows' bound
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------ 5
def test_explore_brdf_space_and_vis_batch(nfx_lib, cuda, tmp_path):
    """A three-material toy root and a saved checkpoint: the driver writes the three files of every id of the test split, its
    render.png of a seen identity is vis_batch(mode='test')'s, and a second run rewrites nothing."""
    from PIL import Image
    from nerfactor_amd.brdf import merl
    from nerfactor_amd.nerfactor import explore_brdf_space
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets.brdf_merl import split_test_identities
    from nerfactor_amd.nerfactor.models import get_model_class
    from tests import synth_scene
    root = str(tmp_path / 'merl')
    names = sorted(synth_scene.write_merl(root, n_rows=64))
    cfg = make_config('brdf', data_root=root)
    torch.manual_seed(1)
    model = get_model_class('brdf')(cfg).to(cuda)
    model.latent_code._z.data.mul_(60.)          # (initialised with std 0.01: materials one could not tell apart)
    run = tmp_path / 'out' / 'lr1e-2'
    os.makedirs(run / 'checkpoints')
    with open(str(run) + '.ini', 'w') as h:
        cfg.write(h)
    ckpt = str(run / 'checkpoints' / 'ckpt-1')
    torch.save({'net': model.state_dict()}, ckpt)

    out = explore_brdf_space.main(['--ckpt=' + ckpt, '--ims', '16', '--batch', '4'])
    ids = split_test_identities(names)
    bdirs = sorted(glob.glob(join(out, 'batch?????????')))
    assert out == join(str(run), 'vis_test', 'ckpt-1') and len(bdirs) == len(ids) == 3 + 2 * 11
    for d, id_ in zip(bdirs, ids):
        assert all(exists(join(d, f)) for f in explore_brdf_space.EXPECTS), d
        with open(join(d, 'metadata.json')) as h:
            meta = json.load(h)
        assert meta['id'] == id_ and len(meta['z']) == 3
        assert np.asarray(Image.open(join(d, 'render.png'))).shape == (16, 16, 3)
        assert np.asarray(Image.open(join(d, 'cslice.png'))).shape == (90, 90)
    # the walk starts at a seen identity and moves: its first step renders that material's sphere
    seen = names.index(model._split_interp_id(ids[3].split('_', 2)[2])[0])
    assert np.array_equal(np.asarray(Image.open(join(bdirs[3], 'render.png'))), np.asarray(Image.open(join(bdirs[seen], 'render.png'))))

    # vis_batch(mode='test') of the seen identity 1, on a batch in the reference's test order: slice coordinates, then rows
    coords = np.vstack((merl.characteristic_slice_rusink().reshape(-1, 3), np.full((5, 3), .3))).astype(np.float32)
    m = coords.shape[0]
    ints = lambda v: torch.full((m,), v, dtype=torch.int32, device=cuda)
    batch = ([names[1]] * m, ints(1), ints(16), ints(16), ints(1), dev(coords, cuda), dev(np.zeros((m, 1)), cuda))
    _, _, _, to_vis = model(batch, mode='test')
    vdir = str(tmp_path / 'vis')
    model.vis_batch(to_vis, vdir, mode='test')
    assert exists(join(vdir, 'raw.npz'))
    for f in ('render.png', 'cslice.png'):
        assert np.array_equal(np.asarray(Image.open(join(vdir, f))), np.asarray(Image.open(join(bdirs[1], f)))), f
    with open(join(vdir, 'metadata.json')) as h:
        assert json.load(h) == json.load(open(join(bdirs[1], 'metadata.json')))

    stamps = {f: os.stat(f).st_mtime_ns for d in bdirs for f in glob.glob(join(d, '*'))}
    os.remove(join(bdirs[2], 'cslice.png'))                  # an unfinished batch is done again, and only that one
    explore_brdf_space.main(['--ckpt=' + ckpt, '--ims', '16', '--batch', '4'])
    again = {f: os.stat(f).st_mtime_ns for d in bdirs for f in glob.glob(join(d, '*'))}
    assert set(again) == set(stamps)
    changed = {f for f in stamps if again[f] != stamps[f]}
    assert changed and all(os.path.dirname(f) == bdirs[2] for f in changed)


# ------------------------------------------------------------------------------------------------ 6
def test_the_c_abi_rejects_bad_arguments(nfx_lib, cuda):
    c = Case(nfx_lib, cuda, 3, 8, 'white', 3, 1)
    lib, d = nfx_lib.lib, c.d
    out = torch.full((1, 3, 3), 7., device=cuda)
    cam = (ctypes.c_float * 3)(*CAM.tolist())
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(z_dim=3, n_lights=128, blob=c.blob):
        return lib.nfx_brdf_sphere_fwd(ptr(d['xyz']), ptr(d['normal']), 3, ctypes.cast(cam, ctypes.c_void_p), ptr(d['z']), z_dim, 1,
                                       ptr(d['lxyz']), ptr(d['lweight']), n_lights, ptr(blob) if blob is not None else None,
                                       ptr(out), None)
    for kw in (dict(z_dim=0), dict(z_dim=9), dict(n_lights=48), dict(blob=None)):
        rc = call(**kw)
        assert rc != 0, kw
        assert nfx_lib.last_error() != '' and 'nfx_brdf_sphere_fwd' in nfx_lib.last_error(), kw
        torch.cuda.synchronize()
        assert bool((out == 7.).all()), kw           # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.).all())
