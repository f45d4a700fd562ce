"""Marching tetrahedra without a GPU: the kernels' tables against the NumPy restatement's, the
restatement's own properties (tests/isosurface_ref.py: closed, consistently oriented, the right topology, outward
winding), mesh.write_ply with normals, and the argument errors of nerfactor/mesh_from_nerf.py."""
import itertools

import numpy as np
import pytest

from tests import isosurface_ref as ref


def _grid(n, lo, hi):
    g = lo + (np.arange(n) + 0.5) / n * (hi - lo)
    return np.meshgrid(g, g, g, indexing='ij'), (g[0],) * 3, (g[1] - g[0],) * 3


def test_tables_of_the_library_equal_the_restatement(nfx_lib):
    from nerfactor_amd import ops
    tri, edge = ops.isosurface_tables()
    want_tri, want_edge = ref.tables()
    assert tri.dtype == want_tri.dtype and tri.shape == want_tri.shape and np.array_equal(tri, want_tri)
    assert edge.dtype == want_edge.dtype and edge.shape == want_edge.shape and np.array_equal(edge, want_edge)


def test_tables_follow_the_rule():
    """One triangle for 1 or 3 inside corners, two for 2, none for 0 or 4; every triangle edge a crossing edge of its tet."""
    tri, edge = ref.tables()
    for t, mask in itertools.product(range(6), range(16)):
        inside = bin(mask).count('1')
        n_tri = int((tri[t, mask, :, 0, 0] >= 0).sum())
        assert n_tri == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside]
        for r in range(n_tri):
            pairs = {tuple(int(x) for x in tri[t, mask, r, v]) for v in range(3)}
            assert len(pairs) == 3
            for a, b in pairs:
                assert a < b and ((mask >> a) & 1) != ((mask >> b) & 1)
    # six tets around the main diagonal, the 19 edges of the split in 7 classes
    classes = {(tuple(edge[t, a, b, 1:]), int(edge[t, a, b, 0])) for t in range(6) for a in range(4) for b in range(a + 1, 4)}
    assert len(classes) == 19 and {c for _, c in classes} == set(range(7))


@pytest.mark.parametrize('shape', ['sphere', 'torus'])
def test_closed_surfaces_are_closed_oriented_and_of_the_right_genus(shape):
    (x, y, z), origin, spacing = _grid(14, -1.5, 1.5)
    if shape == 'sphere':
        f, chi, volume = 1.0 - np.sqrt(x * x + y * y + z * z), 2, 4. / 3. * np.pi
    else:
        f, chi, volume = 0.35 - np.sqrt((np.sqrt(x * x + y * y) - 0.9) ** 2 + z * z), 0, 2 * np.pi ** 2 * 0.9 * 0.35 ** 2
    v, faces = ref.extract(f.astype(np.float32), 0., origin, spacing)
    assert faces.shape[0] > 1000 and faces.max() == v.shape[0] - 1
    assert ref.unpaired_edges(faces).shape[0] == 0, "every directed edge once, its reverse once"
    assert ref.euler_characteristic(v, faces) == chi
    got = ref.signed_volume(v, faces)
    assert 0.85 * volume < got < 1.02 * volume, (got, volume)      # a 14^3 lattice: the inscribed polyhedron


def test_plane_on_an_anisotropic_lattice_faces_down_the_gradient():
    spacing, origin = np.array([0.5, 1., 2.]), np.array([-3.25, -4.5, -7.])
    grad = np.array([0.7, -1.3, 0.45])
    idx = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(6), indexing='ij'), -1)
    f = ((origin + idx * spacing) @ grad + 1.234).astype(np.float32)
    v, faces = ref.extract(f, 0.25, origin, spacing)
    assert faces.shape[0] > 50
    n = ref.face_normals(v, faces)
    assert ((n @ -grad) > 0).all()
    assert np.abs(v.astype(np.float64) @ grad + 1.234 - 0.25).max() < 1e-5      # a linear field is interpolated exactly


def test_a_sphere_cut_by_the_boundary_is_open_only_there():
    (x, y, z), origin, spacing = _grid(12, -1., 1.)
    f = (1.2 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)     # radius 1.2 in a box of half-width 1
    v, faces = ref.extract(f, 0., origin, spacing)
    open_edges = ref.unpaired_edges(faces)
    assert open_edges.shape[0] > 0
    lo, hi = np.float32(origin[0]), np.float32(origin[0]) + np.float32(11) * np.float32(spacing[0])
    on_plane = (np.abs(v[:, None, :] - np.array([lo, hi], dtype=np.float32)[None, :, None]) < 1e-6)      # [nv, 2, 3]
    for a, b in open_edges:
        assert (on_plane[a] & on_plane[b]).any(), "an unpaired edge lies in one boundary plane"


def test_all_256_corner_patterns_of_one_cell():
    rng = np.random.default_rng(5)
    corners = ref.tet_corners()
    edges19 = sorted({(tuple(corners[t, a]), tuple(corners[t, b])) for t in range(6) for a in range(4) for b in range(a + 1, 4)})
    assert len(edges19) == 19
    for pattern in range(256):
        sign = np.array([1. if (pattern >> k) & 1 else -1. for k in range(8)]).reshape(2, 2, 2)      # bit 4 dx + 2 dy + dz
        f = (sign * rng.uniform(0.2, 1., (2, 2, 2))).astype(np.float32)
        v, faces = ref.extract(f, 0.)
        want = 0
        for t in range(6):
            inside = sum(int(f[tuple(corners[t, n])] > 0) for n in range(4))
            want += {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside]
        assert faces.shape[0] == want, pattern
        crossing = [(p, q) for p, q in edges19 if (f[p] > 0) != (f[q] > 0)]
        assert v.shape[0] == len(crossing), pattern
        # vertex k lies on crossing edge k (ascending owner, class) and on no other: one vertex per edge, none shared
        for k, (p, q) in enumerate(sorted(crossing, key=lambda e: (e[0], ref.CLASS_OFFSETS.index(tuple(np.subtract(e[1], e[0])))))):
            t = float(np.float32(0. - f[p]) / np.float32(f[q] - f[p]))
            assert 0. < t < 1.
            assert np.allclose(v[k], np.array(p) + t * np.subtract(q, p), atol=1e-6), (pattern, k)
        assert np.unique(v, axis=0).shape[0] == v.shape[0], pattern
        if faces.size:
            assert set(np.unique(faces)) == set(range(v.shape[0])), pattern


def test_corners_exactly_at_iso_are_outside_and_give_no_nan():
    rng = np.random.default_rng(6)
    f = rng.integers(-2, 3, (6, 5, 7)).astype(np.float32)
    v, faces = ref.extract(f, 1.)
    assert faces.shape[0] > 0 and np.isfinite(v).all()
    at_iso = np.argwhere(f == 1.)
    assert at_iso.shape[0] > 10
    # a corner at iso is outside: an edge to an inside neighbour has its vertex exactly on that corner (t = 0 or 1)
    on_lattice = (v == np.round(v)).all(1)
    assert on_lattice.any() and set(map(tuple, v[on_lattice].astype(int))) <= set(map(tuple, at_iso))


# ------------------------------------------------------------------------------------------------ write_ply
def _write_ply_as_it_stood(path, vertices, faces, binary=True):
    """mesh.write_ply before it learnt normals, verbatim."""
    v = np.asarray(vertices, dtype='<f4').reshape(-1, 3)
    f = np.asarray(faces, dtype='<i4').reshape(-1, 3)
    head = ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % ('binary_little_endian' if binary else 'ascii', v.shape[0], f.shape[0]))
    with open(path, 'wb') as h:
        h.write(head.encode('ascii'))
        if binary:
            h.write(v.tobytes())
            rec = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('v', '<i4', 3)]))
            rec['n'], rec['v'] = 3, f
            h.write(rec.tobytes())
        else:
            for row in v:
                h.write(('%r %r %r\n' % tuple(float(x) for x in row)).encode('ascii'))
            for row in f:
                h.write(('3 %d %d %d\n' % tuple(int(x) for x in row)).encode('ascii'))


@pytest.mark.parametrize('binary', [True, False])
def test_write_ply_with_and_without_normals(tmp_path, binary):
    from nerfactor_amd import mesh
    rng = np.random.default_rng(7)
    v = rng.normal(size=(11, 3)).astype(np.float32)
    f = rng.integers(0, 11, (17, 3)).astype(np.int32)
    n = rng.normal(size=(11, 3)).astype(np.float32)
    mesh.write_ply(str(tmp_path / 'new.ply'), v, f, binary=binary)
    _write_ply_as_it_stood(str(tmp_path / 'old.ply'), v, f, binary=binary)
    assert (tmp_path / 'new.ply').read_bytes() == (tmp_path / 'old.ply').read_bytes()
    mesh.write_ply(str(tmp_path / 'n.ply'), v, f, binary=binary, normals=n)
    head = (tmp_path / 'n.ply').read_bytes().split(b'end_header')[0].decode()
    assert head.index('property float z') < head.index('property float nx') < head.index('property float ny') \
        < head.index('property float nz') < head.index('element face')
    v2, f2 = mesh.read_ply(str(tmp_path / 'n.ply'))
    assert np.array_equal(v2.astype(np.float32), v) and np.array_equal(f2, f)
    if binary:
        body = (tmp_path / 'n.ply').read_bytes().split(b'end_header\n')[1]
        assert np.array_equal(np.frombuffer(body, '<f4', 11 * 6).reshape(11, 6)[:, 3:], n)
    with pytest.raises(ValueError, match='10 normals for 11 vertices'):
        mesh.write_ply(str(tmp_path / 'bad.ply'), v, f, normals=n[:10])


# ------------------------------------------------------------------------------------------------ the driver's refusals
@pytest.mark.parametrize('flags,match', [
    (['--res=1'], 'res = 1'),
    (['--res=1291'], r'res\^3 = 2151685171'),
    (['--iso=nan'], 'iso = nan'),
    (['--iso=inf'], 'iso = inf'),
    (['--scene_bbox=0,1,0,1'], 'got 4 numbers'),
    (['--scene_bbox=0,1,1,0,0,1'], 'min < max'),
    (['--scene_bbox=0,1,a,b,0,1'], 'x_min,x_max'),
])
def test_driver_refuses_bad_arguments_before_anything_else(nfx_lib, flags, match):
    from nerfactor_amd.nerfactor import mesh_from_nerf
    with pytest.raises(ValueError, match=match):
        mesh_from_nerf.main(['--trained_nerf=/nonexistent'] + flags)


def test_driver_flags(nfx_lib):
    from nerfactor_amd.nerfactor import mesh_from_nerf
    args = mesh_from_nerf.parse_args(['--trained_nerf=x'])
    assert (args.res, args.iso, args.network, args.nonormals, args.out, args.scene_bbox) == (256, 10., 'fine', False, None, None)
    assert mesh_from_nerf.default_out('x', 'fine', 256, 10.) == 'x/mesh_fine_res256_iso10.ply'
    assert mesh_from_nerf.default_out('x', 'coarse', 24, 0.5) == 'x/mesh_coarse_res24_iso0.5.ply'
    with pytest.raises(SystemExit):
        mesh_from_nerf.parse_args(['--trained_nerf=x', '--network=medium'])
    with pytest.raises(SystemExit):
        mesh_from_nerf.parse_args(['--res=8'])
    origin, spacing = mesh_from_nerf.lattice_frame([-1.5, 1.5, 0., 1., 2., 4.], 4)
    assert origin == [-1.125, 0.125, 2.25] and spacing == [0.75, 0.25, 0.5]
