"""nerfactor/mesh_from_nerf.py end to end on the GPU: the driver on a saved checkpoint of the NeRF fitted to a unit sphere, its
PLY back through mesh.TriMesh.load, and rays cast against that mesh by the project's own mesh kernels — which checks the
winding contract (face normals leave the object) from the iso-surface kernel to the ray cast."""
import os
from os.path import join

import numpy as np
import pytest
import torch

from tests import synth_scene
from tests.golden import golden_inputs as gi
from tests.test_gpu_render_from_nerf import fill_nerf

pytestmark = pytest.mark.gpu
BOX = [-1.5, 1.5, -1.5, 1.5, -1.5, 1.5]
BBOX = '-1.5,1.5,-1.5,1.5,-1.5,1.5'


@pytest.fixture(scope='module')
def trained_nerf(tmp_path_factory, nfx_lib, cuda):
    """A checkpoint directory of the fitted NeRF, saved the way tests/test_gpu_occupancy.py's scene saves it."""
    from nerfactor_amd.nerfactor.config import make_config
    from nerfactor_amd.nerfactor.models import get_model_class
    root = str(tmp_path_factory.mktemp('mesh_from_nerf'))
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
    return nerf_dir, nerf.to(cuda)


def test_driver_writes_the_mesh_extract_returns_and_rays_hit_its_outside(trained_nerf, cuda, capsys):
    from nerfactor_amd import mesh
    from nerfactor_amd.nerfactor import mesh_from_nerf
    nerf_dir, model = trained_nerf
    out = mesh_from_nerf.main(['--trained_nerf=' + nerf_dir, '--res=24', '--iso=0', '--scene_bbox=' + BBOX])
    assert out == join(nerf_dir, 'mesh_fine_res24_iso0.ply') and os.path.exists(out)
    log = capsys.readouterr().out
    v, f, n = mesh_from_nerf.extract(model, BOX, 24, iso=0.)
    assert '24^3 lattice' in log and '%d vertices, %d triangles' % (v.shape[0], f.shape[0]) in log
    for step in ('lattice', 'iso-surface', 'normals'):
        assert step + ' ' in log
    loaded = mesh.TriMesh.load(out)
    assert np.array_equal(loaded.vertices.astype(np.float32), v) and np.array_equal(loaded.faces, f)
    body = open(out, 'rb').read().split(b'end_header\n')[1]
    assert np.array_equal(np.frombuffer(body, '<f4', v.shape[0] * 6).reshape(-1, 6)[:, 3:], n)
    # 64 rays from radius 3 towards the origin: every one hits, on a face whose normal looks back at it
    rng = np.random.default_rng(12)
    u = rng.normal(size=(64, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t, tri = mesh.RayMeshIntersector(loaded, device=cuda).cast(3. * u, -u)
    t, tri = t.cpu().numpy(), tri.cpu().numpy()
    assert (tri >= 0).all() and np.isfinite(t).all()
    assert 1.5 < t.min() and t.max() < 2.5, "the fitted sphere has radius 1"
    assert ((loaded.face_normals[tri] * -u).sum(1) < 0).all()


def test_driver_options(trained_nerf, tmp_path):
    from nerfactor_amd import mesh
    from nerfactor_amd.nerfactor import mesh_from_nerf
    nerf_dir, _ = trained_nerf
    out = mesh_from_nerf.main(['--trained_nerf=' + nerf_dir, '--res=16', '--iso=0', '--scene_bbox=' + BBOX, '--network=coarse',
                               '--nonormals', '--out=' + str(tmp_path / 'coarse.ply')])
    assert out == str(tmp_path / 'coarse.ply')
    head = open(out, 'rb').read().split(b'end_header')[0]
    assert b'property float nx' not in head
    assert mesh.TriMesh.load(out).faces.shape[0] > 100
