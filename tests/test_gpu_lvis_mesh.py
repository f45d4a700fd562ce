"""The drivers of DESIGN.md section 3.11 on the GPU, on the NeRF fitted to a unit sphere (a 24 x 24 scene, box +-1.5):
mesh_from_nerf with and without the component filter, light visibility from the march and from shadow rays against the
NeRF's own mesh side by side, and geometry_from_nerf --lvis_mesh against the same run without the flag.

Where the fitted level set has floaters was looked up on the CPU first (the fp32 oracle's fine-network density,
oracle/nerf_ref.py, on mesh_from_nerf's lattice, tests/isosurface_ref.py and tests/mesh_components_ref.py): at iso 0 the
surface is one component at res 16 .. 36 and 48; at iso 10 it has 3 components at res 24, 9 at res 36 and 42 at res 40
(18 644 of 20 048 triangles in the largest).  The filtered runs below use res 40, iso 10; the GPU evaluates the network in
bf16, so the test counts the components of the mesh it gets with the reference labelling instead of pinning 42."""
import os
from os.path import join

import numpy as np
import pytest
import torch
from PIL import Image

from tests import isosurface_ref as iso
from tests import mesh_components_ref as ref
from tests import mesh_component_cases as mcc
from tests import synth_scene
from tests.golden import golden_inputs as gi
from tests.test_gpu_render_from_nerf import fill_nerf

pytestmark = pytest.mark.gpu
BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
BBOX = '-1.5,1.5,-1.5,1.5,-1.5,1.5'


@pytest.fixture(scope='module')
def trained_nerf(tmp_path_factory, nfx_lib, cuda):
    """A checkpoint directory of the fitted NeRF, saved the way tests/test_gpu_mesh_from_nerf.py saves it."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    root = str(tmp_path_factory.mktemp('lvis_mesh'))
    data_root, _ = synth_scene.write_scene(root, imh=24, imw=24, n_train=1, n_val=1, n_test=2)
    nerf_dir = join(root, 'out_nerf', 'lr1e-4')
    over = dict(data_root=data_root, imh=24)
    nerf = get_model_class('nerf')(make_config('nerf', **over))
    fill_nerf(nerf, gi.trained_nerf_nets())
    os.makedirs(join(nerf_dir, 'checkpoints'))
    with open(nerf_dir + '.ini', 'w') as h:
        make_config('nerf', **over).write(h)
    nerf.register_trainable()
    torch.save({'net': nerf.state_dict(), 'step': 0}, join(nerf_dir, 'checkpoints', 'ckpt-1'))
    return root, nerf_dir, nerf.to(cuda)


def _read(path):
    """(vertices float32, normals float32, faces) of a PLY written with normals."""
    from nerfactor_amd import mesh
    loaded = mesh.TriMesh.load(path)
    body = open(path, 'rb').read().split(b'end_header\n')[1]
    rows = np.frombuffer(body, '<f4', loaded.vertices.shape[0] * 6).reshape(-1, 6)
    assert np.array_equal(rows[:, :3], loaded.vertices.astype(np.float32))
    return rows[:, :3], rows[:, 3:], loaded.faces


def test_mesh_from_nerf_without_filter_flags_is_unchanged(trained_nerf, tmp_path, capsys):
    from nerfactor_amd import mesh
    from nerfactor_amd.nerfactor import mesh_from_nerf
    _, nerf_dir, model = trained_nerf
    out = mesh_from_nerf.main(['--trained_nerf=' + nerf_dir, '--res=24', '--iso=0', '--scene_bbox=' + BBOX])
    log = capsys.readouterr().out
    assert out == join(nerf_dir, 'mesh_fine_res24_iso0.ply')
    assert 'components' not in log and 'triangles; lattice ' in log
    v, f, n = mesh_from_nerf.extract(model, BOX, 24, iso=0.)
    mesh.write_ply(str(tmp_path / 'want.ply'), v, f, normals=n)
    assert open(out, 'rb').read() == open(str(tmp_path / 'want.ply'), 'rb').read()
    times = {}
    mesh_from_nerf.extract(model, BOX, 24, iso=0., times=times)
    assert sorted(times) == ['isosurface', 'lattice', 'normals']


@pytest.mark.parametrize('res,iso_level', [(24, 0.), (40, 10.)])
def test_mesh_from_nerf_keep_largest_writes_a_closed_sub_mesh(trained_nerf, capsys, res, iso_level):
    from nerfactor_amd.nerfactor import mesh_from_nerf
    _, nerf_dir, model = trained_nerf
    v, f, n = mesh_from_nerf.extract(model, BOX, res, iso=iso_level)
    label = ref.labels(f, v.shape[0])
    n_components = np.unique(label[f[:, 0]]).size
    print('res %d, iso %g: %d vertices, %d triangles, %d components' % (res, iso_level, v.shape[0], f.shape[0], n_components))
    assert n_components > 1 or res == 24, "res 40, iso 10 is the run with floaters"
    want_v, want_f, want = mcc.filter_numpy(v, f, label, keep_largest=1)
    out = mesh_from_nerf.main(['--trained_nerf=' + nerf_dir, '--res=%d' % res, '--iso=%g' % iso_level, '--scene_bbox=' + BBOX,
                               '--keep_largest=1'])
    log = capsys.readouterr().out
    assert out == join(nerf_dir, 'mesh_fine_res%d_iso%g_largest1.ply' % (res, iso_level))
    assert ('%d vertices, %d triangles; %d components, 1 kept, %d triangles and %d vertices dropped, components '
            % (want_v.shape[0], want_f.shape[0], n_components, want['dropped_faces'], want['dropped_vertices'])) in log
    got_v, got_n, got_f = _read(out)
    index = want['vertex_index'].numpy()
    assert np.array_equal(got_v.view(np.uint32), v[index].view(np.uint32)), "the surviving vertices, bit for bit, in order"
    assert np.array_equal(got_f, want_f)
    assert np.array_equal(got_v[got_f].view(np.uint32), v[f[label[f[:, 0]] == want['kept'][0][0]]].view(np.uint32))
    assert iso.unpaired_edges(got_f).size == 0, "closed"
    assert np.array_equal(got_n.view(np.uint32), n[index].view(np.uint32)), "the normals of the surviving vertices"
    # extract() with a filter returns what the driver wrote, and min_faces selects by size
    found = {}
    ev, ef, en = mesh_from_nerf.extract(model, BOX, res, iso=iso_level, keep_largest=1, info=found)
    assert np.array_equal(ev, got_v) and np.array_equal(ef, got_f) and np.array_equal(en, got_n)
    assert found['n_components'] == n_components and len(found['kept']) == 1
    if n_components > 1:
        sizes = np.sort(np.unique(label[f[:, 0]], return_counts=True)[1])
        mv, mf, _ = mesh_from_nerf.extract(model, BOX, res, iso=iso_level, min_faces=int(sizes[-2]), normals=False)
        assert mf.shape[0] == sizes[sizes >= sizes[-2]].sum() and mv.shape[0] > got_v.shape[0]


@pytest.fixture(scope='module')
def sphere_mesh(trained_nerf):
    """The PLY of mesh_from_nerf --keep_largest=1 at res 40, iso 10."""
    from nerfactor_amd.nerfactor import mesh_from_nerf
    root, nerf_dir, _ = trained_nerf
    return mesh_from_nerf.main(['--trained_nerf=' + nerf_dir, '--res=40', '--iso=10', '--scene_bbox=' + BBOX, '--keep_largest=1',
                                '--out=' + join(root, 'largest.ply')])


def test_the_two_light_visibility_routes(trained_nerf, sphere_mesh, cuda):
    from nerfactor_amd import mesh
    from nerfactor_amd.brdf.renderer import gen_light_xyz
    from nerfactor_amd.nerfactor import geometry_from_nerf as G
    from nerfactor_amd.nerfactor.config import make_config
    model = trained_nerf[2]
    cfg = make_config('nerf')
    rayo, rayd, _ = gi.nerf1k_rays()
    o = torch.from_numpy(np.ascontiguousarray(rayo, dtype=np.float32)).to(cuda)
    d = torch.nn.functional.normalize(torch.from_numpy(np.ascontiguousarray(rayd, dtype=np.float32)).to(cuda), dim=1, eps=1e-12)
    inter = mesh.RayMeshIntersector(mesh.TriMesh.load(sphere_mesh), device=cuda)
    with torch.no_grad():
        occu, depth, normal = G.compute_depth_and_normal(model, o, d, cfg)
        hit = torch.nonzero(occu.clamp(0, 1) > 0)[:, 0][::8]
        surf = (o[hit] + d[hit] * depth[hit, None]).contiguous()
        nrm = normal[hit].contiguous()
        march = G.compute_light_visibility(model, surf, nrm, cfg, light_h=8)
        by_mesh = G.compute_light_visibility_mesh(inter, surf, nrm, light_h=8, eps=0.1)
        chunked = G.compute_light_visibility_mesh(inter, surf, nrm, light_h=8, eps=0.1, chunk=7)
    assert surf.shape[0] >= 32 and by_mesh.shape == march.shape == (surf.shape[0], 128)
    assert torch.equal(by_mesh, chunked)
    lxyz = gen_light_xyz(8, 16)[0].reshape(-1, 3).astype(np.float32).astype(np.float64)
    s64, n64 = surf.cpu().numpy().astype(np.float64), nrm.cpu().numpy().astype(np.float64)
    to_light = lxyz[None] - s64[:, None]
    cos = (n64[:, None] * to_light / np.linalg.norm(to_light, axis=-1, keepdims=True)).sum(-1)
    back = cos < -1e-4
    march, by_mesh = march.cpu().numpy(), by_mesh.cpu().numpy()
    assert back.sum() > 1000 and not march[back].any() and not by_mesh[back].any()
    assert np.isin(by_mesh, (0., 1.)).all() and (by_mesh == 1).any() and (by_mesh == 0).any()
    front = cos > 1e-4
    print('front-lit pairs %d: mean |march - mesh| %.4f, |diff| > 0.5 on %.4f' %
          (front.sum(), np.abs(march - by_mesh)[front].mean(), (np.abs(march - by_mesh)[front] > 0.5).mean()))


def test_geometry_from_nerf_with_lvis_mesh(trained_nerf, sphere_mesh, capsys):
    from nerfactor_amd.nerfactor import geometry_from_nerf
    root, nerf_dir, _ = trained_nerf
    base = ['--trained_nerf=' + nerf_dir, '--imh=24', '--occu_thres=0.05', '--light_h=8', '--scene_bbox=' + BBOX]
    plain = geometry_from_nerf.main(base + ['--out_root=' + join(root, 'geo_march')])
    capsys.readouterr()
    meshed = geometry_from_nerf.main(base + ['--out_root=' + join(root, 'geo_mesh'), '--lvis_mesh=' + sphere_mesh])
    assert 'light visibility from ' + sphere_mesh in capsys.readouterr().out
    assert len(plain) == len(meshed) >= 3
    mixed = 0
    for a, b in zip(plain, meshed):
        for name in ('xyz.npy', 'normal.npy', 'alpha.png', 'xyz.png', 'normal.png'):
            assert open(join(a, name), 'rb').read() == open(join(b, name), 'rb').read(), (b, name)
        lvis = np.load(join(b, 'lvis.npy'))
        assert lvis.shape == (24, 24, 128) and lvis.dtype == np.float32 and os.path.exists(join(b, 'lvis.png'))
        alpha = np.asarray(Image.open(join(b, 'alpha.png')))
        for row, a8 in zip(lvis.reshape(-1, 128), alpha.reshape(-1)):
            values = np.unique(row[row != 0])
            assert values.size <= 1, "a pixel's visibility is 0 or its alpha"
            assert a8 != 0 or values.size == 0
            mixed += int(values.size == 1 and (row == 0).any())
    assert mixed > 0, "some pixel has lit and unlit lights"


def test_surf_from_mvs_keep_largest_casts_against_the_largest_component(cuda, nfx_lib, tmp_path, capsys):
    """tests/mesh_cases.py's S1 is a sphere (320 triangles) over a ground grid (128): with --keep_largest=1 the driver writes,
    file for file, what it writes for a scan that holds the sphere alone."""
    from nerfactor_amd.data_gen.dtu_mvs import surf_from_mvs
    from nerfactor_amd.mesh import PerspCam, write_ply
    from tests import mesh_cases
    v, f = mesh_cases.scene('S1')
    sphere = f[:320]
    assert sphere.max() + 1 == 162 and f[320:].min() == 162
    outs = {}
    for name, (mv, mf, flags) in (('whole', (v, f, ['--keep_largest=1'])), ('sphere', (v[:162], sphere, []))):
        cam_dir, surf_dir, img_dir, out = (str(tmp_path / name / p) for p in ('cams', 'surf', 'scan7', 'out'))
        for p in (cam_dir, surf_dir, img_dir):
            os.makedirs(p)
        write_ply(surf_from_mvs.mesh_path_of(surf_dir, img_dir), mv, mf, binary=True)
        rng = np.random.RandomState(5)
        for i in range(2):
            cam = PerspCam(f_pix=40., im_res=(32, 40), loc=mesh_cases.CENTRE + (1300 * np.cos(2. * i), 1300 * np.sin(2. * i), -900.),
                           lookat=mesh_cases.CENTRE, up=(0, 0, -1))
            np.savetxt(join(cam_dir, 'pos_%03d.txt' % (i + 1)), cam.int_mat.dot(cam.ext_mat))
            Image.fromarray(rng.randint(0, 255, size=(32, 40, 3)).astype(np.uint8)).save(join(img_dir, 'rect_%03d_3_r5000.png' % (i + 1)))
        surf_from_mvs.main(['--cam_dir', cam_dir, '--surf_dir', surf_dir, '--img_dir', img_dir, '--outdir', out, '--h', '16',
                            '--light_h', '4', '--n_test', '2', '--n_vali', '1'] + flags)
        outs[name] = (out, capsys.readouterr().out)
    assert '2 components, 1 kept, 128 triangles and 81 vertices dropped, components ' in outs['whole'][1]
    assert ': 162 vertices, 320 triangles' in outs['whole'][1] and 'components' not in outs['sphere'][1]
    views = sorted(os.listdir(outs['sphere'][0]))
    assert sorted(os.listdir(outs['whole'][0])) == views and len(views) == 5
    compared = 0
    for view in views:
        if view == 'lights.npz':
            a, b = (np.load(join(outs[k][0], view)) for k in ('whole', 'sphere'))
            assert all(np.array_equal(a[key], b[key]) for key in ('lxyzs', 'lareas'))
            continue
        for name in ('alpha.png', 'xyz.npy', 'normal.npy', 'lvis.npy'):
            assert open(join(outs['whole'][0], view, name), 'rb').read() == open(join(outs['sphere'][0], view, name), 'rb').read(), (view, name)
            compared += 1
    assert compared == 16
    assert (np.load(join(outs['whole'][0], 'test_000', 'lvis.npy')) == 1).any()
