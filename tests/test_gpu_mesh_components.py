"""csrc/mesh_components.hip on the GPU: the labels equal the NumPy union-find of
tests/mesh_components_ref.py exactly on every case of tests/mesh_component_cases.py — the 70 001-vertex chains, the hub that
100 000 unions contend for, wave and block edges — under any order and rotation of the faces, on every run and whatever the
output and the workspace held before; the filter on the device equals mesh.filter_by_labels of the reference labels; and on
the analytic scene the mesh shadow rays show the point of it: 93 front-lit pairs shadowed by the floaters, none without them.
No test launches the kernel with a face index out of range."""
import numpy as np
import pytest
import torch

from tests import mesh_component_cases as mcc

pytestmark = pytest.mark.gpu
CASES = sorted(mcc.cases())


def _labels(faces, nv, cuda, **kw):
    from nerfactor_amd import ops
    return ops.mesh_components(torch.from_numpy(np.array(faces)).to(cuda), nv, **kw).cpu().numpy()


@pytest.fixture(scope='module')
def scene_on_device(nfx_lib, cuda):
    """(vertices, faces) of the scene from ops.isosurface on the device; equal to the restatement's."""
    from nerfactor_amd import ops
    origin, spacing = mcc.scene_frame()
    v, f = ops.isosurface(torch.from_numpy(np.array(mcc.scene_field())).to(cuda), 0., origin, spacing)
    rv, rf = mcc.scene_mesh()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.cpu().numpy(), rf)
    return v, f


@pytest.mark.parametrize('name', CASES)
def test_labels_equal_the_reference(name, nfx_lib, cuda, scene_on_device):
    from nerfactor_amd import ops
    faces, nv = mcc.cases()[name]
    want = mcc.reference(name)
    if name == 'j':
        got = ops.mesh_components(scene_on_device[1], nv).cpu().numpy()
    else:
        got = _labels(faces, nv, cuda)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # any order of the faces, any rotation inside a face; a second run; poisoned output and workspace
    rng = np.random.default_rng(5)
    if faces.shape[0]:
        moved = faces[rng.permutation(faces.shape[0])]
        moved = np.take_along_axis(moved, (np.arange(3)[None] + rng.integers(0, 3, size=(moved.shape[0], 1))) % 3, axis=1)
        assert np.array_equal(_labels(moved, nv, cuda), want)
    assert np.array_equal(_labels(faces, nv, cuda), want)
    for byte in (0xFF, 0x7F):
        label = torch.full((nv,), byte, dtype=torch.uint8, device=cuda).repeat_interleave(4).view(torch.int32)
        ws = torch.full((16,), byte, dtype=torch.uint8, device=cuda).view(torch.int32)
        assert label.shape == (nv,) and ws.shape == (4,)
        assert np.array_equal(_labels(faces, nv, cuda, label=label, ws=ws), want), hex(byte)
        assert int(ws[0]) == 0, "no face was skipped"


def test_nv_zero_and_the_torch_pre_check(nfx_lib, cuda):
    from nerfactor_amd import ops
    none = torch.zeros((0, 3), dtype=torch.int32, device=cuda)
    assert tuple(ops.mesh_components(none, 0).shape) == (0,)
    faces = torch.tensor(((0, 1, 2), (2, 3, 4)), dtype=torch.int32, device=cuda)
    assert ops.mesh_components(faces, 5).tolist() == [0] * 5
    # refused by the reductions in torch: the kernel is not launched with these
    with pytest.raises(nfx_lib.NfxError, match=r'0 \.\. 4, outside \[0, 4\)'):
        ops.mesh_components(faces, 4)
    bad = faces.clone()
    bad[1, 1] = -1
    with pytest.raises(nfx_lib.NfxError, match=r'-1 \.\. 4, outside \[0, 5\)'):
        ops.mesh_components(bad, 5)
    with pytest.raises(nfx_lib.NfxError, match='outside'):
        ops.mesh_components(faces, 0)
    with pytest.raises(nfx_lib.NfxError, match='contiguous'):
        ops.mesh_components(faces.t().contiguous().t(), 5)
    with pytest.raises(nfx_lib.NfxError, match='int32'):
        ops.mesh_components(faces.long(), 5)


def test_filter_on_the_device_equals_the_filter_of_the_reference_labels(nfx_lib, cuda, scene_on_device):
    from nerfactor_amd import mesh, ops
    v, f = scene_on_device
    normals = torch.nn.functional.normalize(v, dim=1)
    v1, f1, (n1,), info = ops.mesh_filter_components(v, f, keep_largest=1, attrs=(normals,))
    rv, rf, rinfo = mcc.filter_numpy(*mcc.scene_mesh(), mcc.reference('j'), keep_largest=1)
    assert v1.is_cuda and f1.is_cuda and f1.dtype == torch.int32
    assert np.array_equal(v1.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f1.cpu().numpy(), rf)
    assert np.array_equal(info['vertex_index'].cpu().numpy(), rinfo['vertex_index'].numpy())
    assert torch.equal(n1, normals[info['vertex_index']])
    assert {k: info[k] for k in info if k != 'vertex_index'} == {k: rinfo[k] for k in rinfo if k != 'vertex_index'}
    assert info['kept'] == [(0, 11304, 5654)]
    # the host convenience: the same mesh
    whole = mesh.TriMesh(*mcc.scene_mesh())
    largest = whole.filter_components(keep_largest=1, device=cuda)
    assert np.array_equal(largest.vertices.astype(np.float32), rv) and np.array_equal(largest.faces, rf)
    assert largest.filter_info['dropped_faces'] == 608
    two = whole.filter_components(min_faces=201, device=cuda)
    assert two.filter_info['kept'] == [(0, 11304, 5654), (2202, 408, 206)]
    with pytest.raises(ValueError, match='keep_largest'):
        whole.filter_components(device=cuda)


def test_shadow_rays_on_the_whole_and_on_the_filtered_mesh(nfx_lib, cuda, scene_on_device):
    """nfx_mesh_lvis against the fp32 emulation (bit for bit) and the float64 oracle of tests/mesh_cases.py, both stored by
    tests/golden/make_mesh_components_golden.py and re-checked row-wise by the CPU suite."""
    from nerfactor_amd import mesh
    xyz, normal, alpha, lxyz = mcc.scene_rows()
    whole = mesh.TriMesh(*mcc.scene_mesh())
    gold, cos = mcc.scene_golden(), mcc.scene_cos()
    shadowed = []
    for name, tri_mesh in (('whole', whole), ('largest', whole.filter_components(keep_largest=1, device=cuda))):
        got = mesh.RayMeshIntersector(tri_mesh, device=cuda).light_visibility(xyz, normal, alpha, lxyz, mcc.EPS).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), gold[name]['emu'].view(np.uint32))
        excluded = gold[name]['edge'] | (np.abs(cos) <= mcc.COS_MARGIN)
        assert excluded.mean() <= 0.02
        assert np.array_equal(got[~excluded], gold[name]['lvis'][~excluded])
        shadowed.append(int(((cos > 0) & ~excluded & (got == 0)).sum()))
    assert shadowed == [93, 0]
