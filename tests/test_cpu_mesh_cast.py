"""The mesh ray cast without a GPU: the host-side BVH builder (reached through the loaded library, and once more as a plain
C++ program under the address and undefined-behaviour sanitizers), the fp32 emulation of csrc/mesh_cast.hip against the
float64 oracle (tests/mesh_cases.py), the PLY reader, the projection-matrix decomposition and the camera."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_cases as mc
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_mvs_cams.npz')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _leafs(scene):
    return (1, 4, mc.scene(scene)[1].shape[0])


# ---------------------------------------------------------------------------------------------- builder
@pytest.mark.parametrize('scene', mc.SCENES)
def test_builder_invariants(nfx_lib, scene):
    from nerfactor_amd import ops
    v, f = mc.scene(scene)
    nf = f.shape[0]
    for max_leaf in _leafs(scene):
        blob = ops.mesh_bvh_build(v, f, max_leaf)
        assert blob.ctypes.data % 16 == 0 and blob.size == nfx_lib.lib.nfx_mesh_bvh_bytes(nf, max_leaf)
        assert np.array_equal(blob, ops.mesh_bvh_build(v.copy(), f.copy(), max_leaf))            # two builds, identical bytes
        B = mc.parse_blob(blob)
        nn = B['n_nodes']
        assert B['magic'] == 0x4856424e and B['n_tris'] == nf and B['max_leaf'] == min(max_leaf, nf)
        if max_leaf >= nf:
            assert nn == 1 and B['first'][0] == 0                                                # one leaf with every triangle
        assert B['skip'][nn] == nn and B['first'][nn] == nf                                      # the sentinel
        skip, first = B['skip'][:nn], B['first'][:nn]
        sub = np.where(B['first'] < 0, -B['first'] - 1, B['first'])
        assert (skip > np.arange(nn)).all() and (skip <= nn).all()
        # every triangle in exactly one leaf, leaves contiguous and in order; the reordered triangles are the mesh's
        assert sorted(B['orig'].tolist()) == list(range(nf))
        np.testing.assert_array_equal(B['tris'], v[f[B['orig']]])
        covered = 0
        for i in np.nonzero(first >= 0)[0]:
            assert first[i] == covered and 1 <= sub[skip[i]] - first[i] <= max_leaf
            covered = sub[skip[i]]
        assert covered == nf

        def subtree(i):
            """(end of the subtree of node i, lo, hi of everything below) — depth-first: the first child is i + 1, the second
            child the first child's skip link, and the subtree ends at the node's own skip link."""
            if first[i] >= 0:
                tri = B['tris'][first[i]:sub[skip[i]]].reshape(-1, 3)
                lo, hi = tri.min(0), tri.max(0)
                assert (B['lo'][i] < lo).all() and (B['hi'][i] > hi).all()                        # padded outward
                return i + 1, B['lo'][i], B['hi'][i]
            assert sub[i] == sub[i + 1]
            end_l, lo_l, hi_l = subtree(i + 1)
            assert end_l == skip[i + 1]
            end_r, lo_r, hi_r = subtree(end_l)
            assert end_r == skip[end_l] == skip[i]
            assert (B['lo'][i] <= np.minimum(lo_l, lo_r)).all() and (B['hi'][i] >= np.maximum(hi_l, hi_r)).all()
            return end_r, B['lo'][i], B['hi'][i]
        assert subtree(0)[0] == nn


def test_builder_and_entry_points_reject_bad_input(nfx_lib):
    from nerfactor_amd import ops
    v, f = mc.scene('S4')
    bad_v = v.copy()
    bad_v[2, 1] = np.inf
    with pytest.raises(nfx_lib.NfxError, match='non-finite'):
        ops.mesh_bvh_build(bad_v, f, 4)
    bad_f = f.copy()
    bad_f[3, 2] = v.shape[0]
    with pytest.raises(nfx_lib.NfxError, match='names vertex'):
        ops.mesh_bvh_build(v, bad_f, 4)
    with pytest.raises(nfx_lib.NfxError):
        ops.mesh_bvh_build(v, f, 0)
    assert nfx_lib.lib.nfx_mesh_bvh_bytes(0, 4) == 0
    # the cast entry points check the host header against the blob's size before anything is launched (no GPU touched here)
    blob = ops.mesh_bvh_build(v, f, 4)
    for damage in ('magic', 'nodes', 'size', 'align'):
        header, size, ptr = blob[:32].copy(), blob.size, blob.ctypes.data
        if damage == 'magic':
            header[0] ^= 1
        elif damage == 'nodes':
            header[8:12].view(np.int32)[0] += 1
        elif damage == 'size':
            size -= 48
        else:
            ptr += 4
        rc = nfx_lib.lib.nfx_mesh_cast(ptr, size, header.ctypes.data, None, None, 0, None, None, None)
        assert rc != 0 and 'nfx_mesh_cast' in nfx_lib.last_error(), damage
        rc = nfx_lib.lib.nfx_mesh_lvis(ptr, size, header.ctypes.data, None, None, None, 0, None, 1, 0.1, None, None)
        assert rc != 0 and 'nfx_mesh_lvis' in nfx_lib.last_error(), damage
    assert nfx_lib.lib.nfx_mesh_cast(blob.ctypes.data, blob.size, blob[:32].ctypes.data, None, None, 0, None, None, None) == 0


def test_builder_under_address_and_ub_sanitizers(tmp_path):
    """mesh_bvh.cpp alone as plain C++ (it includes no HIP header) with a stand-alone main, S1-S4, max_leaf 1 / 4 / nf."""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, 'nerfactor_amd', 'csrc')
    assert 'hip' not in ''.join(l for l in open(os.path.join(src, 'mesh_bvh.cpp')) if l.startswith('#include')).lower()
    exe = str(tmp_path / 'mesh_bvh_san')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I' + src,
                    os.path.join(src, 'mesh_bvh.cpp'), os.path.join(ROOT, 'tests', 'mesh_bvh_sanitizer_main.cpp'), '-o', exe], check=True)
    paths = []
    for s in mc.SCENES:
        v, f = mc.scene(s)
        paths.append(str(tmp_path / (s + '.mesh')))
        with open(paths[-1], 'wb') as h:
            np.array((v.shape[0], f.shape[0]), dtype=np.int64).tofile(h)
            v.tofile(h)
            f.tofile(h)
    res = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert res.returncode == 0 and 'MESH_BVH_SANITIZER_OK' in res.stdout, res.stdout + res.stderr


# ---------------------------------------------------------------------------------------------- emulation and oracle
@pytest.mark.parametrize('scene', mc.SCENES)
def test_emulated_tree_walk_is_the_emulated_brute_force(nfx_lib, scene):
    from nerfactor_amd import ops
    v, f = mc.scene(scene)
    o, d = mc.rays(1280)
    want_t, want_tri = mc.emu_cast_brute(v, f, o, d)
    for max_leaf in _leafs(scene):
        t, tri, visited, _ = mc.emu_cast_tree(ops.mesh_bvh_build(v, f, max_leaf), o, d)
        np.testing.assert_array_equal(tri, want_tri)
        np.testing.assert_array_equal(_bits(t), _bits(want_t))
        assert visited.max() <= mc.parse_blob(ops.mesh_bvh_build(v, f, max_leaf))['n_nodes']
    if scene == 'S1':      # the shadow rays' early-exit walk decides what the brute force decides
        xyz, normal, alpha = mc.surface_rows('S1')
        so, sd = mc.shadow_rays32(xyz[alpha != 0][::3], mc.light_xyz(4), mc.LVIS_EPS)
        hit, _, _ = mc.emu_cast_tree(ops.mesh_bvh_build(v, f, 4), so.reshape(-1, 3), sd.reshape(-1, 3), any_hit=True)
        np.testing.assert_array_equal(hit, mc.emu_cast_brute(v, f, so.reshape(-1, 3), sd.reshape(-1, 3), any_hit=True))
        assert hit.any() and not hit.all()


@pytest.mark.parametrize('scene', mc.SCENES)
def test_emulation_against_the_float64_oracle(scene):
    v, f = mc.scene(scene)
    o, d = mc.rays(1280)
    t, tri = mc.emu_cast_brute(v, f, o, d)
    ref = mc.oracle64(v, f, o, d)
    assert ref['edge'].mean() <= 0.01
    np.testing.assert_array_equal(tri[~ref['edge']], ref['tri'][~ref['edge']])
    assert (tri >= 0).any() and (tri < 0).any()
    if scene == 'S2':
        nf = f.shape[0]
        assert (tri == mc.DUP).any() and not np.isin(tri, (nf - 3, nf - 2)).any()     # tie to the smaller index; zero area never hit


def test_emulation_is_watertight():
    v, f = mc.scene('S1')
    o, d = mc.watertight_rays()
    t, tri = mc.emu_cast_brute(v, f, o, d)
    assert (tri >= 0).sum() == o.shape[0] == 642           # 0 misses allowed
    # a target that faces the camera is reached on the sphere itself (a silhouette target may be passed by a rounding and the
    # ray then ends on the far side or on the ground: still a hit)
    target = (o + d).astype(np.float64)
    facing = ((target - mc.CENTRE) * (mc.CAM - target)).sum(1) > 0.05 * 300 * np.linalg.norm(mc.CAM - target, axis=1)
    assert facing.sum() > 200 and (tri[facing] < 320).all()
    np.testing.assert_allclose(t[facing], 1, atol=1e-5)          # d = target - origin: the hit is the target


# ---------------------------------------------------------------------------------------------- PLY
def test_ply_round_trips_and_rejections(tmp_path):
    from nerfactor_amd.mesh import TriMesh, read_ply, write_ply
    v, f = mc.scene('S4')
    for binary in (True, False):
        p = str(tmp_path / ('m%d.ply' % binary))
        write_ply(p, v, f, binary=binary)
        rv, rf = read_ply(p)
        np.testing.assert_array_equal(rv.astype(np.float32), v)
        np.testing.assert_array_equal(rf, f)
        assert rf.dtype == np.int32
    # double coordinates, extra vertex properties, uint indices under the other name, binary
    p = str(tmp_path / 'extra.ply')
    dt = np.dtype([('x', '<f8'), ('nx', '<f4'), ('y', '<f8'), ('z', '<f8'), ('red', 'u1')])
    rec = np.zeros(v.shape[0], dtype=dt)
    rec['x'], rec['y'], rec['z'], rec['nx'], rec['red'] = v[:, 0], v[:, 1], v[:, 2], 7, 200
    frec = np.zeros(f.shape[0], dtype=np.dtype([('n', 'u1'), ('v', '<u4', 3)]))
    frec['n'], frec['v'] = 3, f
    with open(p, 'wb') as h:
        h.write(("ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex %d\nproperty double x\nproperty float nx\n"
                 "property double y\nproperty double z\nproperty uchar red\nelement face %d\nproperty list uchar uint vertex_index\n"
                 "end_header\n" % (v.shape[0], f.shape[0])).encode())
        h.write(rec.tobytes() + frec.tobytes())
    rv, rf = read_ply(p)
    np.testing.assert_array_equal(rv, v.astype(np.float64))
    np.testing.assert_array_equal(rf, f)
    # ... and as ASCII
    p = str(tmp_path / 'extra_ascii.ply')
    with open(p, 'w') as h:
        h.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0 9\n1 0 0.5 9\n0 2 0 9\n3 0 1 2\n")
    rv, rf = read_ply(p)
    np.testing.assert_array_equal(rv, [[0, 0, 0], [1, 0, 0.5], [0, 2, 0]])
    np.testing.assert_array_equal(rf, [[0, 1, 2]])
    # a quad raises, in both encodings; so do big-endian files and files that are not PLY
    q = str(tmp_path / 'quad.ply')
    with open(q, 'w') as h:
        h.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match='triangles'):
        read_ply(q)
    qb = str(tmp_path / 'quadb.ply')
    with open(qb, 'wb') as h:
        h.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                b"element face 1\nproperty list uchar int vertex_indices\nend_header\n")
        h.write(np.zeros(12, '<f4').tobytes() + b'\x04' + np.arange(4, dtype='<i4').tobytes())
    with pytest.raises(ValueError, match='triangles'):
        read_ply(qb)
    with open(q, 'w') as h:
        h.write("ply\nformat binary_big_endian 1.0\nend_header\n")
    with pytest.raises(ValueError, match='not supported'):
        read_ply(q)
    # face normals: normalize(cross(v1 - v0, v2 - v0)), trimesh's definition
    m = TriMesh(*mc.scene('S2'))
    tri = m.vertices[m.faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(n, axis=1)
    ok = length > 0
    assert (~ok).sum() == 1 and (m.face_normals[~ok] == 0).all()
    np.testing.assert_allclose(m.face_normals[ok], n[ok] / length[ok, None], rtol=0, atol=1e-15)
    sphere = m.face_normals[:320]
    centre_to_face = tri[:320].mean(1) - mc.CENTRE
    assert ((sphere * centre_to_face).sum(1) > 0).all()          # outward


# ---------------------------------------------------------------------------------------------- camera
def test_decompose_projection():
    from nerfactor_amd.mesh import decompose_projection
    rng = np.random.RandomState(0)
    for k in range(8):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        R = q * np.sign(np.linalg.det(q))
        K = np.array([[2800. + 50 * k, 0.3 * k, 800.], [0, 2850. - 20 * k, 600.], [0, 0, 1.]])
        t = rng.normal(size=3) * 500
        P = K.dot(np.hstack((R, t[:, None]))) * (1. if k % 2 == 0 else 3.7)
        K2, R2, t2 = decompose_projection(P)
        np.testing.assert_allclose(K2.dot(np.hstack((R2, t2[:, None]))), P, rtol=0, atol=1e-12 * np.abs(P).max())
        assert (np.tril(K2, -1) == 0).all() and (np.diag(K2) > 0).all()
        assert abs(np.linalg.det(R2) - 1) < 1e-12
        np.testing.assert_allclose(R2.dot(R2.T), np.eye(3), atol=1e-12)
        np.testing.assert_allclose(K2 / K2[2, 2], K, rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(R2, R, atol=1e-10)
    with pytest.raises(ValueError):
        decompose_projection(np.eye(3))


def test_perspcam_and_camera_path_against_the_reference():
    from nerfactor_amd.data_gen.dtu_mvs import surf_from_mvs
    from nerfactor_amd.mesh import PerspCam, sph2cart
    g = np.load(GOLD)
    for k in ('a', 'b'):
        cam = PerspCam()
        cam.int_mat = g['ext_%s_K' % k]
        cam.ext_mat = g['ext_%s_Rt' % k]
        assert (cam.im_h, cam.im_w) == (8, 10)
        np.testing.assert_allclose(cam.loc, g['ext_%s_loc' % k], rtol=0, atol=1e-9)
        rays = cam.gen_rays()
        assert rays.shape == (8, 10, 1, 3)
        np.testing.assert_allclose(rays, g['ext_%s_rays' % k], rtol=0, atol=1e-12)
        np.testing.assert_allclose(cam.ext_mat, g['ext_%s_Rt' % k], rtol=0, atol=1e-9)          # setter and getter are inverses
        cam = PerspCam(f_pix=float(g['look_%s_f' % k]), im_res=tuple(g['look_%s_hw' % k]), loc=g['look_%s_loc' % k],
                       lookat=g['look_%s_lookat' % k], up=g['look_%s_up' % k])
        np.testing.assert_allclose(cam.gen_rays(), g['look_%s_rays' % k], rtol=0, atol=1e-12)
    lats, lngs = surf_from_mvs.test_cam_path(float(g['test_cam_dist']), 6)
    locs = np.array([sph2cart((float(g['test_cam_dist']), lat, lng)) + g['test_center'] for lat, lng in zip(lats, lngs)])
    np.testing.assert_allclose(locs, g['test_locs'], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(surf_from_mvs.vali_indices(49, 2), np.arange(49)[:-1:24])
    assert surf_from_mvs.mesh_path_of('/d/surf/', '/i/scan65/') == '/d/surf/surf065_l3_surf_11_trim_8.ply'
