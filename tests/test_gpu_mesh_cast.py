"""nfx_mesh_cast / nfx_mesh_lvis (csrc/mesh_cast.hip) on the GPU against the two oracles of tests/mesh_cases.py, and the
DTU driver end to end.

Tolerances (measured): the kernel equals the fp32 emulation bit for bit, so its error against the
float64 oracle is the emulation's: the largest |xyz - oracle| over the view on S1 and S2 is 3.67e-4 (o + t d in fp32 at
coordinates of ~1000, where one ulp is 6.1e-5), allowed 4 x = 1.5e-3; the largest |normal . dir| error of the fp32 shadow
direction is 1.27e-7, so pairs with |normal . dir| <= 4 x = 5.1e-7 are not compared."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu

XYZ_TOL = 4 * 3.67e-4
COS_MARGIN = 4 * 1.27e-7


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _intersector(scene, max_leaf):
    from nerfactor_amd.mesh import RayMeshIntersector, TriMesh
    v, f = mc.scene(scene)
    return RayMeshIntersector(TriMesh(v, f), max_leaf=max_leaf, device='cuda:0')


@functools.lru_cache(maxsize=None)
def _emu(scene, n):
    v, f = mc.scene(scene)
    return mc.emu_cast_brute(v, f, *mc.rays(n))


def _cast(scene, max_leaf, o, d):
    t, tri = _intersector(scene, max_leaf).cast(o, d)
    return t.cpu().numpy(), tri.cpu().numpy()


@pytest.mark.parametrize('n', mc.RAY_COUNTS)
@pytest.mark.parametrize('scene', mc.SCENES)
def test_cast_is_the_emulation_for_every_tree(cuda, nfx_lib, scene, n):
    """max_leaf 1, 4 and nf (one leaf: brute force) give the same bits, and those are the emulation's: a box test that culls
    a triangle, a walk that skips a subtree or a tie broken by order shows here."""
    o, d = mc.rays(n)
    want_t, want_tri = _emu(scene, n)
    nf = mc.scene(scene)[1].shape[0]
    for max_leaf in (4, 1, nf):
        t, tri = _cast(scene, max_leaf, o, d)
        np.testing.assert_array_equal(tri, want_tri, err_msg='max_leaf %d' % max_leaf)
        np.testing.assert_array_equal(_bits(t), _bits(want_t), err_msg='max_leaf %d' % max_leaf)
    if scene == 'S2' and n == 1280:
        assert (want_tri == mc.DUP).sum() >= 1 and not (want_tri == nf - 2).any()      # the duplicate never wins the tie
        assert not (want_tri == nf - 3).any()                                        # the zero-area triangle is never hit


@pytest.mark.parametrize('scene', ['S1', 'S2'])
def test_cast_against_the_float64_oracle(cuda, nfx_lib, scene):
    v, f = mc.scene(scene)
    o, d = mc.rays(1280)
    t, tri = _cast(scene, 4, o, d)
    ref = mc.oracle64(v, f, o, d)
    assert ref['edge'].mean() <= 0.01
    keep = ~ref['edge']
    np.testing.assert_array_equal(tri[keep], ref['tri'][keep])
    hit = keep & (tri >= 0)
    assert hit.sum() > 400 and (tri < 0).sum() > 400
    xyz = o[hit] + t[hit][:, None] * d[hit]
    err = np.abs(xyz.astype(np.float64) - (o[hit].astype(np.float64) + ref['t'][hit][:, None] * d[hit].astype(np.float64))).max()
    print('%s: max |xyz - oracle| = %.3e (allowed %.3e)' % (scene, err, XYZ_TOL))
    assert err <= XYZ_TOL


def test_rays_at_vertices_and_edge_midpoints_all_hit(cuda, nfx_lib):
    """Watertightness: rays aimed exactly at every vertex and every edge midpoint of S1's sphere, 0 misses allowed."""
    o, d = mc.watertight_rays()
    for max_leaf in (4, 1):
        t, tri = _cast('S1', max_leaf, o, d)
        assert (tri >= 0).all(), np.nonzero(tri < 0)[0]


@functools.lru_cache(maxsize=None)
def _lvis_case(name):
    xyz, normal, alpha = mc.surface_rows('S1')
    if name == 'L32':
        lxyz = mc.light_xyz(4)
    else:
        rows = np.arange(70) * 18
        xyz, normal, alpha, lxyz = xyz[rows], normal[rows], alpha[rows], mc.light_xyz(16)
    v, f = mc.scene('S1')
    return xyz, normal, alpha, lxyz, mc.emu_lvis(v, f, xyz, normal, alpha, lxyz, mc.LVIS_EPS)[0], \
        mc.oracle_lvis64(v, f, xyz, normal, alpha, lxyz, mc.LVIS_EPS)


@pytest.mark.parametrize('case', ['L32', 'L512'])
def test_lvis_is_the_emulation_and_the_oracle(cuda, nfx_lib, case):
    xyz, normal, alpha, lxyz, emu, ref = _lvis_case(case)
    assert lxyz.shape[0] == {'L32': 32, 'L512': 512}[case] and xyz.shape[0] == {'L32': 1280, 'L512': 70}[case]
    for max_leaf in (4, 448):
        got = _intersector('S1', max_leaf).light_visibility(xyz, normal, alpha, lxyz, mc.LVIS_EPS).cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(emu), err_msg='max_leaf %d' % max_leaf)
    excluded = ref['edge'] | (np.abs(ref['cos']) <= COS_MARGIN)
    assert excluded.mean() <= 0.02
    np.testing.assert_array_equal(got[~excluded], ref['lvis'][~excluded])
    lit_side = ~excluded & (ref['cos'] > 0) & (alpha[:, None] != 0)
    assert (got[lit_side] == 1).sum() >= 100 and (got[lit_side] == 0).sum() >= 100      # a test where nothing is occluded shows nothing


def test_outputs_are_written_whatever_they_held_and_rows_are_independent(cuda, nfx_lib):
    from nerfactor_amd import ops
    inter = _intersector('S2', 4)
    blob, header = inter.mesh.bvh(4, 'cuda:0')
    o, d = mc.rays(1280)
    want_t, want_tri = _emu('S2', 1280)
    to = lambda a: torch.as_tensor(np.array(a), device='cuda:0')
    # a permuted subset gives the permuted subset
    idx = np.random.RandomState(3).permutation(1280)[:333]
    t, tri = _cast('S2', 4, o[idx], d[idx])
    np.testing.assert_array_equal(tri, want_tri[idx])
    np.testing.assert_array_equal(_bits(t), _bits(want_t[idx]))
    # non-finite and zero-direction rays miss; their neighbours do not notice
    o2, d2 = o[:8].copy(), d[:8].copy()
    d2[1] = 0
    d2[2, 1] = np.nan
    o2[3, 0] = np.inf
    d2[4, 2] = -np.inf
    o2[5, 2] = np.nan
    t, tri = _cast('S2', 4, o2, d2)
    bad = [1, 2, 3, 4, 5]
    assert (tri[bad] == -1).all() and np.isposinf(t[bad]).all()
    good = [0, 6, 7]
    np.testing.assert_array_equal(tri[good], want_tri[:8][good])
    np.testing.assert_array_equal(_bits(t[good]), _bits(want_t[:8][good]))
    # light visibility: NaN-filled and 0x7f-filled outputs end up the same; alpha-0 rows are 0 even with NaN xyz
    xyz, normal, alpha = (a.copy() for a in mc.surface_rows('S1'))
    xyz[alpha == 0] = np.nan
    lxyz = mc.light_xyz(4)[:31]                                   # a light count that is no multiple of anything
    inter1 = _intersector('S1', 4)
    blob1, header1 = inter1.mesh.bvh(4, 'cuda:0')
    outs = []
    for fill in (float('nan'), None):
        out = torch.full((1280, 31), float('nan'), device='cuda:0') if fill is not None else \
            torch.full((1280 * 31 * 4,), 0x7f, dtype=torch.uint8, device='cuda:0').view(torch.float32).reshape(1280, 31)
        ops.mesh_lvis(blob1, header1, to(xyz), to(normal), to(alpha), to(lxyz), mc.LVIS_EPS, out=out)
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.isfinite(outs[0]).all() and (outs[0][alpha == 0] == 0).all() and (outs[0] == 1).any()
    v, f = mc.scene('S1')
    clean = np.where(alpha[:, None] != 0, xyz, 0).astype(np.float32)
    np.testing.assert_array_equal(_bits(outs[0]), _bits(mc.emu_lvis(v, f, clean, normal, alpha, lxyz, mc.LVIS_EPS)[0]))
    # ... and the same for the cast's outputs
    res, od, dd = [], to(o), to(d)
    for byte in (0x7f, 0xff):
        t = torch.full((1280 * 4,), byte, dtype=torch.uint8, device='cuda:0').view(torch.float32)
        tri = torch.full((1280 * 4,), byte, dtype=torch.uint8, device='cuda:0').view(torch.int32)
        nfx_lib.check(nfx_lib.lib.nfx_mesh_cast(ops._ptr(blob), blob.numel(), header.ctypes.data, ops._ptr(od), ops._ptr(dd), 1280,
                                                ops._ptr(t), ops._ptr(tri), ops._stream()), 'nfx_mesh_cast')
        res.append((t.cpu().numpy(), tri.cpu().numpy()))
    for t, tri in res:
        np.testing.assert_array_equal(tri, want_tri)
        np.testing.assert_array_equal(_bits(t), _bits(want_t))


def test_driver_end_to_end(cuda, nfx_lib, tmp_path):
    """A synthetic DTU-layout scan through surf_from_mvs, then the MVS dataset and the shape model read what it wrote."""
    from PIL import Image
    from nerfactor_amd.data_gen.dtu_mvs import surf_from_mvs
    from nerfactor_amd.mesh import PerspCam, write_ply
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.datasets import get_dataset_class
    from nerfactor_amd.nerfactor.models import get_model_class
    v, f = mc.scene('S1')
    cam_dir, surf_dir, img_dir, out = (str(tmp_path / p) for p in ('cams', 'surf', 'scan7', 'out'))
    for p in (cam_dir, surf_dir, img_dir):
        os.makedirs(p)
    write_ply(surf_from_mvs.mesh_path_of(surf_dir, img_dir), v, f, binary=True)
    rng = np.random.RandomState(5)
    for i in range(6):
        ang = 2 * np.pi * i / 6
        cam = PerspCam(f_pix=80., im_res=(64, 80), loc=mc.CENTRE + (1300 * np.cos(ang), 1300 * np.sin(ang), -900.), lookat=mc.CENTRE,
                       up=(0, 0, -1))
        np.savetxt(os.path.join(cam_dir, 'pos_%03d.txt' % (i + 1)), cam.int_mat.dot(cam.ext_mat))
        Image.fromarray(rng.randint(0, 255, size=(64, 80, 3)).astype(np.uint8)).save(os.path.join(img_dir, 'rect_%03d_3_r5000.png' % (i + 1)))
    surf_from_mvs.main(['--cam_dir', cam_dir, '--surf_dir', surf_dir, '--img_dir', img_dir, '--outdir', out, '--h', '32', '--light_h', '4',
                        '--n_test', '4', '--n_vali', '2'])
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, '*_???'))) == \
        ['test_%03d' % i for i in range(4)] + ['train_%03d' % i for i in range(4)] + ['val_000', 'val_001']
    assert os.path.exists(os.path.join(out, 'test_000', 'nn.png')) and not os.path.exists(os.path.join(out, 'test_000', 'rgba.png'))
    cfg = make_config('shape_mvs', mvs_root=out, outroot=str(tmp_path / 'o'), imh=32, light_h=4)
    for mode, n_views in (('train', 4), ('vali', 2), ('test', 4)):
        assert get_dataset_class('mvs_shape')(cfg, mode, device='cpu').get_n_views() == n_views      # nothing skipped
    model = get_model_class('shape')(cfg)
    lights = np.load(os.path.join(out, 'lights.npz'))
    np.testing.assert_array_equal(model.lxyz.numpy(), lights['lxyzs'].astype(np.float32))
    assert lights['lxyzs'].shape == (4, 8, 3) and lights['lareas'].shape == (4, 8)
    # one view against the float64 oracle: a test view, whose alpha the dataset takes from alpha.png (a training view's comes
    # from its image).  Its camera is the last training camera moved onto the lat / lng path.
    from nerfactor_amd.mesh import sph2cart
    ds = get_dataset_class('mvs_shape')(cfg, 'test', device='cpu')
    batch = next(iter(ds.build_pipeline(no_batch=True, no_shuffle=True)))
    assert batch[0][0] == 'test_000' and tuple(batch[1].numpy().ravel()[:2]) == (32, 40)
    alpha, xyz, normal, lvis = (b.numpy() for b in batch[5:9])
    centre = v.astype(np.float64).mean(axis=0)
    train_locs = [surf_from_mvs.camera_from_projection(np.loadtxt(p), 2., (32, 40)).loc for p in sorted(glob.glob(os.path.join(cam_dir, '*.txt')))]
    cam_dist = 1.5 * np.mean([np.linalg.norm(x - centre) for x in train_locs])
    lats, lngs = surf_from_mvs.test_cam_path(cam_dist, 4)
    cam0 = PerspCam(f_pix=40., im_res=(32, 40), loc=sph2cart((cam_dist, lats[0], lngs[0])) + centre, lookat=centre, up=(0, 0, -1))
    meta = json.load(open(os.path.join(out, 'test_000', 'metadata.json')))
    np.testing.assert_allclose(meta['cam_loc'], cam0.loc, atol=1e-6)
    assert (meta['imh'], meta['imw'], meta['id']) == (32, 40, 'test_000')
    d = cam0.gen_rays().reshape(-1, 3).astype(np.float32)
    o = np.tile(cam0.loc, (d.shape[0], 1)).astype(np.float32)
    ref = mc.oracle64(v, f, o, d)
    keep = ~ref['edge']
    assert ref['edge'].mean() <= 0.01
    hit = ref['tri'] >= 0
    np.testing.assert_array_equal(alpha.reshape(-1)[keep], hit[keep].astype(np.float32))
    sel = keep & hit
    assert sel.sum() > 100
    want_xyz = o.astype(np.float64) + ref['t'][:, None] * d.astype(np.float64)
    assert np.abs(xyz.reshape(-1, 3)[sel] - want_xyz[sel]).max() <= XYZ_TOL
    from nerfactor_amd.mesh import TriMesh
    np.testing.assert_allclose(normal.reshape(-1, 3)[sel], TriMesh(v, f).face_normals[ref['tri'][sel]], atol=1e-6)
    raw_xyz = np.load(os.path.join(out, 'test_000', 'xyz.npy')).reshape(-1, 3)
    raw_normal = np.load(os.path.join(out, 'test_000', 'normal.npy')).reshape(-1, 3)
    lref = mc.oracle_lvis64(v, f, raw_xyz, raw_normal, hit.astype(np.float32), lights['lxyzs'].reshape(-1, 3).astype(np.float32), 0.1)
    excluded = lref['edge'] | (np.abs(lref['cos']) <= COS_MARGIN) | ~keep[:, None]
    assert excluded.mean() <= 0.02
    np.testing.assert_array_equal(lvis.reshape(-1, 32)[~excluded], lref['lvis'][~excluded])
    assert (lvis == 1).any() and (lvis.reshape(-1, 32)[hit] == 0).any()
