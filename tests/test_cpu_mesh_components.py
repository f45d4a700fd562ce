"""Connected components of a triangle mesh without a GPU: the NumPy reference satisfies its own
definition on every case, mesh.filter_by_labels (plain torch) on CPU tensors, the analytic scene — two floaters beside a unit
sphere wrongly shadow 93 of 6080 front-lit (point, light) pairs in the float64 ray oracle, none once only the largest
component is kept — and the refusals of the C-ABI and the three drivers that are decided before a GPU is touched."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import isosurface_ref as iso
from tests import mesh_cases
from tests import mesh_component_cases as mcc
from tests import mesh_components_ref as ref

CASES = sorted(mcc.cases())


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('name', CASES)
def test_reference_labels_satisfy_the_definition(name):
    faces, nv = mcc.cases()[name]
    lab = mcc.reference(name)
    assert lab.dtype == np.int32 and lab.shape == (nv,)
    assert (lab <= np.arange(nv)).all()
    assert np.array_equal(lab[lab], lab), "a label is the label of itself"
    assert (lab[faces] == lab[faces[:, :1]]).all(), "one label per face"
    named = np.zeros(nv, dtype=bool)
    named[faces.reshape(-1)] = True
    assert np.array_equal(lab[~named], np.arange(nv)[~named])
    if name in mcc.SMALL:
        assert np.array_equal(ref.flood_fill(faces, nv), lab)


def test_reference_on_the_cases_with_a_known_answer():
    assert np.array_equal(mcc.reference('a'), np.arange(5))
    assert np.array_equal(mcc.reference('b'), (0, 0, 0, 3))
    for name in ('c_ascending', 'c_descending', 'c_shuffled', 'd', 'g'):
        assert not mcc.reference(name).any(), name
    assert np.unique(mcc.reference('e')).size == 40000
    assert np.array_equal(mcc.reference('f'), np.arange(20001) % 2)
    faces, _ = mcc.cases()['d']
    assert 1000 < int(np.nonzero(faces == 0)[0][0]) < faces.shape[0] - 1000, "the minimum sits inside the chain"


# ------------------------------------------------------------------------------------------------ filter_by_labels
def _toy():
    """Four components over 14 vertices: label 0 with 2 faces, 3 with 3 (one of them degenerate), 7 with 3, 11 with 1;
    vertices 6 and 13 are named by no face."""
    faces = np.array(((7, 8, 9), (0, 1, 2), (3, 4, 5), (9, 8, 10), (11, 12, 11), (4, 4, 5), (2, 1, 0), (3, 5, 4), (10, 7, 9)), dtype=np.int32)
    vertices = np.arange(14 * 3, dtype=np.float32).reshape(14, 3) * 0.5
    return vertices, faces, ref.labels(faces, 14)


def _filter(vertices, faces, label, **kw):
    from nerfactor_amd import mesh
    attrs = kw.pop('attrs', ())
    return mesh.filter_by_labels(torch.from_numpy(vertices.copy()), torch.from_numpy(faces.copy()), torch.from_numpy(label.copy()),
                                 attrs=attrs, **kw)


def test_filter_keeps_order_reindexes_and_gathers_attrs(nfx_lib):
    vertices, faces, label = _toy()
    assert np.array_equal(label, (0, 0, 0, 3, 3, 3, 6, 7, 7, 7, 7, 11, 11, 13))
    normals = torch.from_numpy(-vertices.copy())
    ids = torch.arange(14)[:, None]
    v, f, (n, i), info = _filter(vertices, faces, label, keep_largest=2, attrs=(normals, ids))
    keep_face = np.isin(label[faces[:, 0]], (3, 7))         # sizes 3 and 3: the two largest
    old = np.array((3, 4, 5, 7, 8, 9, 10))
    assert np.array_equal(info['vertex_index'].numpy(), old) and info['vertex_index'].dtype == torch.int64
    assert np.array_equal(v.numpy(), vertices[old]) and np.array_equal(n.numpy(), -vertices[old]) and np.array_equal(i.numpy()[:, 0], old)
    assert f.dtype == torch.int32 and np.array_equal(v.numpy()[f.numpy()], vertices[faces[keep_face]]), "the same coordinates, in order"
    assert info['n_components'] == 4 and info['n_unreferenced'] == 2
    assert info['kept'] == [(3, 3, 3), (7, 3, 4)]
    assert info['dropped_faces'] == 3 and info['dropped_vertices'] == 7


def test_filter_ties_go_to_the_smaller_label_and_the_criteria_intersect(nfx_lib):
    vertices, faces, label = _toy()
    assert _filter(vertices, faces, label, keep_largest=1)[3]['kept'] == [(3, 3, 3)]
    assert _filter(vertices, faces, label, keep_largest=3)[3]['kept'] == [(0, 2, 3), (3, 3, 3), (7, 3, 4)]
    assert _filter(vertices, faces, label, min_faces=2)[3]['kept'] == [(0, 2, 3), (3, 3, 3), (7, 3, 4)]
    assert _filter(vertices, faces, label, min_faces=3)[3]['kept'] == [(3, 3, 3), (7, 3, 4)]
    assert _filter(vertices, faces, label, keep_largest=1, min_faces=3)[3]['kept'] == [(3, 3, 3)]
    assert _filter(vertices, faces, label, keep_largest=4, min_faces=2)[3]['kept'] == [(0, 2, 3), (3, 3, 3), (7, 3, 4)]
    # the largest component fails min_faces: nothing is left, and that is not an error
    v, f, (a,), info = _filter(vertices, faces, label, keep_largest=1, min_faces=4, attrs=(torch.zeros(14, 2),))
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(a.shape) == (0, 2)
    assert info['kept'] == [] and info['dropped_faces'] == 9 and info['dropped_vertices'] == 14 and info['vertex_index'].numel() == 0
    # a mesh without faces
    v, f, _, info = _filter(vertices, faces[:0], np.arange(14, dtype=np.int32), keep_largest=1)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and info['n_components'] == 0 and info['n_unreferenced'] == 14


def test_filter_refusals(nfx_lib):
    vertices, faces, label = _toy()
    for kw in (dict(), dict(keep_largest=0, min_faces=0), dict(keep_largest=-1), dict(min_faces=-2), dict(keep_largest=1.5)):
        with pytest.raises(ValueError, match='keep_largest'):
            _filter(vertices, faces, label, **kw)
    with pytest.raises(ValueError, match='label'):
        _filter(vertices, faces, label[:-1], keep_largest=1)
    with pytest.raises(ValueError, match='attribute'):
        _filter(vertices, faces, label, keep_largest=1, attrs=(torch.zeros(13, 3),))
    with pytest.raises(ValueError, match='outside'):
        _filter(vertices, faces + 12, label, keep_largest=1)


# ------------------------------------------------------------------------------------------------ the scene
def test_scene_is_what_the_tests_pin(nfx_lib):
    v, f = mcc.scene_mesh()
    assert v.shape == (5962, 3) and f.shape == (11912, 3)
    assert iso.unpaired_edges(f).size == 0 and iso.euler_characteristic(v, f) == 6
    lab = mcc.reference('j')
    comp, faces_of = np.unique(lab[f[:, 0]], return_counts=True)
    assert comp.tolist() == [0, 2202, 5860] and faces_of.tolist() == [11304, 408, 200]
    assert [int((lab == c).sum()) for c in comp] == [5654, 206, 102]


def test_scene_largest_component_is_the_closed_sphere(nfx_lib):
    v, f = mcc.scene_mesh()
    v1, f1, info = mcc.filter_numpy(v, f, mcc.reference('j'), keep_largest=1)
    assert v1.shape == (5654, 3) and f1.shape == (11304, 3) and info['kept'] == [(0, 11304, 5654)]
    assert info['n_components'] == 3 and info['dropped_faces'] == 608 and info['dropped_vertices'] == 308
    assert iso.unpaired_edges(f1).size == 0 and iso.euler_characteristic(v1, f1) == 2
    assert np.abs(np.linalg.norm(v1, axis=1) - 1).max() < 0.02, "the unit sphere"
    assert np.array_equal(mcc.filter_numpy(v, f, mcc.reference('j'), min_faces=409)[1], f1)
    v2, f2, info2 = mcc.filter_numpy(v, f, mcc.reference('j'), min_faces=201)
    assert info2['kept'] == [(0, 11304, 5654), (2202, 408, 206)] and iso.euler_characteristic(v2, f2) == 4


def test_floaters_shadow_the_sphere_and_the_filter_removes_them(nfx_lib):
    """The float64 ray oracle on the scene (stored results, tests/golden/make_mesh_components_golden.py): of 6080 front-lit
    pairs 93 are shadowed on the whole mesh and none on its largest component; no pair is excluded."""
    gold = mcc.scene_golden()
    cos = mcc.scene_cos()
    front = cos > 0
    excluded = gold['whole']['edge'] | gold['largest']['edge'] | (np.abs(cos) <= mcc.COS_MARGIN)
    shadowed = [int((front & (gold[k]['lvis'] == 0)).sum()) for k in ('whole', 'largest')]
    print('front-lit %d, shadowed %s, excluded %d' % (front.sum(), shadowed, excluded.sum()))
    assert front.sum() == 6080 and not excluded.any()
    assert shadowed == [93, 0]
    assert np.array_equal(gold['largest']['lvis'], front.astype(np.float64))
    for k in ('whole', 'largest'):
        assert not gold[k]['lvis'][~front].any()
        assert np.array_equal(gold[k]['emu'], gold[k]['lvis'].astype(np.float32)), "fp32 emulation and float64 oracle agree off the excluded set"


def test_stored_oracle_results_are_the_oracles(nfx_lib):
    """Every twelfth surface row again, live, through mesh_cases.oracle_lvis64 and mesh_cases.emu_lvis on both meshes."""
    v, f = mcc.scene_mesh()
    xyz, normal, alpha, lxyz = mcc.scene_rows()
    v1, f1, _ = mcc.filter_numpy(v, f, mcc.reference('j'), keep_largest=1)
    gold = mcc.scene_golden()
    rows = slice(0, 96, 12)
    for k, (mv, mf) in (('whole', (v, f)), ('largest', (v1, f1))):
        ref = mesh_cases.oracle_lvis64(mv, mf, xyz[rows], normal[rows], alpha[rows], lxyz, mcc.EPS)
        assert np.array_equal(ref['lvis'], gold[k]['lvis'][rows]) and np.array_equal(ref['edge'], gold[k]['edge'][rows])
        assert np.array_equal(ref['cos'], mcc.scene_cos()[rows])
        emu, _ = mesh_cases.emu_lvis(mv, mf, xyz[rows], normal[rows], alpha[rows], lxyz, mcc.EPS)
        assert np.array_equal(emu.view(np.uint32), gold[k]['emu'][rows].view(np.uint32))
    assert (gold['whole']['lvis'][rows] != gold['largest']['lvis'][rows]).any(), "the rows recomputed include shadowed pairs"


# ------------------------------------------------------------------------------------------------ refusals before the GPU
def test_c_abi_refuses_the_limits_before_any_launch(nfx_lib):
    lib = nfx_lib.lib
    size = lib.nfx_mesh_components_workspace_bytes
    assert size(0, 0) == 16 and size(1 << 20, 1 << 21) == 16 and size((1 << 31) - 1, ((1 << 31) - 1) // 3) == 16
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 1) == 0 and size(1, ((1 << 31) + 2) // 3) == 0
    for nf, nv, faces, label, ws, wsb, word in ((1, -1, 16, 16, 16, 16, 'nv = -1'), (1, 1 << 31, 16, 16, 16, 16, 'nv = 2147483648'),
                                                (-1, 4, 16, 16, 16, 16, 'nf = -1'), (715827883, 4, 16, 16, 16, 16, '3 nf = 2147483649'),
                                                (1, 4, 16, 16, 16, 12, '12 bytes'), (1, 4, 16, 16, None, 16, 'null workspace'),
                                                (1, 4, None, 16, 16, 16, 'null pointer'), (1, 4, 16, None, 16, 16, 'null pointer'),
                                                (1, 4, 20, 16, 16, 16, 'aligned'), (1, 4, 16, 24, 16, 16, 'aligned'),
                                                (1, 4, 16, 16, 8, 16, 'aligned')):
        rc = lib.nfx_mesh_components(faces, nf, nv, label, ws, wsb, None)       # never dereferenced: refused first
        assert rc != 0 and 'nfx_mesh_components' in nfx_lib.last_error() and word in nfx_lib.last_error(), (word, nfx_lib.last_error())


def test_ops_refuse_host_tensors(nfx_lib):
    from nerfactor_amd import ops
    with pytest.raises(nfx_lib.NfxError, match='CUDA'):
        ops.mesh_components(torch.zeros((2, 3), dtype=torch.int32), 4)
    with pytest.raises(nfx_lib.NfxError, match='CUDA'):
        ops.mesh_filter_components(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), keep_largest=1)


def test_mesh_from_nerf_refuses_negative_filters_and_names_the_filtered_file(nfx_lib):
    from nerfactor_amd.nerfactor import mesh_from_nerf
    box = [-1., 1.] * 3
    assert mesh_from_nerf.check_lattice(box, 8, 0., 0, 0) == mesh_from_nerf.check_lattice(box, 8, 0.)
    for kw in (dict(keep_largest=-1), dict(min_faces=-1)):
        with pytest.raises(ValueError, match='negative'):
            mesh_from_nerf.check_lattice(box, 8, 0., **kw)
    for flag in ('--keep_largest=-1', '--min_faces=-3'):
        with pytest.raises(ValueError, match='negative'):
            mesh_from_nerf.main(['--trained_nerf=/nonexistent', '--res=8', flag])
    name = mesh_from_nerf.default_out
    assert name('d', 'fine', 24, 0.) == 'd/mesh_fine_res24_iso0.ply'
    assert name('d', 'fine', 24, 0., 1, 0) == 'd/mesh_fine_res24_iso0_largest1.ply'
    assert name('d', 'fine', 24, 0., 0, 50) == 'd/mesh_fine_res24_iso0_min50.ply'
    assert name('d', 'coarse', 128, 10., 2, 50) == 'd/mesh_coarse_res128_iso10_largest2_min50.ply'
    args = mesh_from_nerf.parse_args(['--trained_nerf=x'])
    assert args.keep_largest == 0 and args.min_faces == 0


def test_surf_from_mvs_refuses_negative_filters(nfx_lib):
    from nerfactor_amd.data_gen.dtu_mvs import surf_from_mvs
    base = ['--cam_dir=c', '--surf_dir=s', '--img_dir=i/scan1', '--outdir=o']
    args = surf_from_mvs.parse_args(base)
    assert args.keep_largest == 0 and args.min_faces == 0
    for flag in ('--keep_largest=-1', '--min_faces=-1'):
        with pytest.raises(ValueError, match='negative'):
            surf_from_mvs.main(base + [flag])


def test_geometry_from_nerf_refuses_a_bad_mesh_or_eps_before_the_gpu(nfx_lib, tmp_path):
    from nerfactor_amd import mesh
    from nerfactor_amd.nerfactor import geometry_from_nerf as g
    base = ['--trained_nerf=/nonexistent', '--out_root=' + str(tmp_path / 'out')]
    args = g.parse_args(base)
    assert args.lvis_mesh is None and args.lvis_mesh_eps == 0.1
    assert g.check_lvis_mesh(None, float('nan')) is None, "without --lvis_mesh the eps is not looked at"
    with pytest.raises(FileNotFoundError, match='lvis_mesh'):
        g.main(base + ['--lvis_mesh=' + str(tmp_path / 'missing.ply')])
    junk = tmp_path / 'junk.ply'
    junk.write_bytes(b'not a mesh at all')
    with pytest.raises(ValueError, match='cannot be read'):
        g.main(base + ['--lvis_mesh=' + str(junk)])
    good = str(tmp_path / 'good.ply')
    mesh.write_ply(good, [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    for eps in ('0', '-0.1', 'nan', 'inf'):
        with pytest.raises(ValueError, match='lvis_mesh_eps'):
            g.main(base + ['--lvis_mesh=' + good, '--lvis_mesh_eps=' + eps])
    empty = str(tmp_path / 'empty.ply')
    mesh.write_ply(empty, [[0, 0, 0]], np.zeros((0, 3), dtype=np.int32))
    with pytest.raises(ValueError, match='no triangle'):
        g.main(base + ['--lvis_mesh=' + empty])
    loaded = g.check_lvis_mesh(good, 0.1)
    assert loaded.faces.shape == (1, 3)
    assert not (tmp_path / 'out').exists()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        g.parse_args(base + ['--help'])
    helptext = ' '.join(buf.getvalue().split())
    assert 'binary' in helptext and 'unbounded' in helptext and 'level set' in helptext
