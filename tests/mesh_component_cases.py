"""The meshes of the component-labelling tests (tests/test_cpu_mesh_components.py, tests/test_gpu_mesh_components.py), seeded,
and the analytic scene that shows what floaters do to light visibility.

  a   nv = 5, no face                                  b   one triangle in nv = 4: vertex 3 is named by no face
  c   the strip (i, i+1, i+2) over 70 001 vertices — one path-shaped component — with the faces ascending, descending and
      shuffled                                         d   the same strip with the vertex ids permuted: the minimum sits mid-chain
  e   40 000 disjoint triangles with permuted ids      f   two interleaved strips (i, i+2, i+4): the labels alternate 0, 1
  g   spokes (hub, 2i, 2i+1), i < 50 000, hub = nv - 1: everything meets at one heavily contended vertex, every label is 0
  h   a random mesh with every face three times, plus (a, a, a) and (a, a, b) faces
  i   nv in {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} with nv // 2 random faces: many components, wave and block edges
  j   the scene: on the 32^3 lattice over [-1.6, 1.6]^3 (spacing 0.1) the float32 field
      max(1 - |p|, 0.2 - |p - (0, 0, 1.3)|, 0.15 - |p - (1.25, 0.3, 0.2)|) at iso 0 — a unit sphere and two small blobs beside
      it, extracted by tests/isosurface_ref.py: 5962 vertices, 11 912 triangles, three closed components."""
import functools

import numpy as np

STRIP_NV = 70001
I_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
SCENE_BOX = [-1.6, 1.6] * 3
SCENE_RES = 32
BLOBS = (((0., 0., 0.), 1.), ((0., 0., 1.3), .2), ((1.25, .3, .2), .15))
LIGHT_H = 8
EPS = 0.1
COS_MARGIN = 4 * 1.27e-7  # tests/test_gpu_mesh_cast.py's: a pair with |normal . dir| <= this may fall on either side in fp32


def _strip(nv, step=1):
    i = np.arange(nv - 2 * step, dtype=np.int32)
    return np.stack((i, i + step, i + 2 * step), 1)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (faces int32 [nf, 3], nv)}; read-only arrays."""
    rng = np.random.default_rng(20)
    out = {'a': (np.zeros((0, 3), dtype=np.int32), 5), 'b': (np.array(((2, 0, 1),), dtype=np.int32), 4)}
    strip = _strip(STRIP_NV)
    out['c_ascending'] = (strip, STRIP_NV)
    out['c_descending'] = (strip[::-1].copy(), STRIP_NV)
    out['c_shuffled'] = (strip[rng.permutation(strip.shape[0])], STRIP_NV)
    out['d'] = (rng.permutation(STRIP_NV).astype(np.int32)[strip], STRIP_NV)
    out['e'] = (rng.permutation(120000).astype(np.int32).reshape(-1, 3), 120000)
    out['f'] = (_strip(20001, 2)[rng.permutation(20001 - 4)], 20001)
    i = np.arange(50000, dtype=np.int32)
    out['g'] = (np.stack((np.full_like(i, 100000), 2 * i, 2 * i + 1), 1), 100001)
    base = rng.integers(0, 3000, size=(900, 3)).astype(np.int32)
    a, b = rng.integers(0, 3000, size=(2, 200)).astype(np.int32)
    out['h'] = (np.concatenate((base, np.stack((a, a, a), 1), base, np.stack((a, a, b), 1), base))[rng.permutation(3100)], 3000)
    for nv in I_SIZES:
        out['i_%d' % nv] = (rng.integers(0, nv, size=(nv // 2, 3)).astype(np.int32), nv)
    out['j'] = (scene_mesh()[1], scene_mesh()[0].shape[0])
    for f, _ in out.values():
        f.setflags(write=False)
    return out


SMALL = ('a', 'b', 'h') + tuple('i_%d' % nv for nv in I_SIZES)     # the cases the flood fill also labels


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference labels of a case, computed once."""
    from tests import mesh_components_ref
    faces, nv = cases()[name]
    lab = mesh_components_ref.labels(faces, nv)
    lab.setflags(write=False)
    return lab


# ------------------------------------------------------------------------------------------------ the scene (case j)
def scene_frame():
    """(origin, spacing) of the scene's lattice: mesh_from_nerf.lattice_frame of the box at 32 points per axis."""
    from nerfactor_amd.nerfactor import mesh_from_nerf
    return mesh_from_nerf.lattice_frame(SCENE_BOX, SCENE_RES)


@functools.lru_cache(maxsize=None)
def scene_field():
    """float32 [32, 32, 32]: the field on the lattice points origin + idx * spacing (float32, multiply then add)."""
    origin, spacing = (np.asarray(x, dtype=np.float32) for x in scene_frame())
    idx = np.stack(np.meshgrid(*(np.arange(SCENE_RES, dtype=np.float32),) * 3, indexing='ij'), -1)
    p = origin + idx * spacing
    assert p.dtype == np.float32
    field = None
    for centre, radius in BLOBS:
        q = p - np.asarray(centre, dtype=np.float32)
        f = np.float32(radius) - np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])
        field = f if field is None else np.maximum(field, f)
    assert field.dtype == np.float32
    field.setflags(write=False)
    return field


@functools.lru_cache(maxsize=None)
def scene_mesh():
    """(vertices float32 [nv, 3], faces int32 [nf, 3]) of the scene by the NumPy restatement of the iso-surface rules."""
    from tests import isosurface_ref
    origin, spacing = scene_frame()
    v, f = isosurface_ref.extract(scene_field(), 0., origin, spacing)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def scene_rows():
    """(xyz, normal, alpha, lxyz) float32: 96 seeded points on the unit sphere with their outward normals, and the
    2 x 8 x 16 lights of gen_light_xyz(8, 16)."""
    from nerfactor_amd.brdf.renderer import gen_light_xyz
    u = np.random.default_rng(3).normal(size=(96, 3))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    lxyz, _ = gen_light_xyz(LIGHT_H, 2 * LIGHT_H)
    return u, u.copy(), np.ones(96, dtype=np.float32), np.asarray(lxyz).reshape(-1, 3).astype(np.float32)


def scene_digest():
    """SHA-256 (hex) of the scene's mesh, surface rows and lights: what the stored oracle results belong to."""
    import hashlib
    h = hashlib.sha256()
    for a in scene_mesh() + scene_rows():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def scene_golden():
    """{whole|largest: dict(emu float32, lvis float64, edge bool [96, 128])}: mesh_cases.emu_lvis and mesh_cases.oracle_lvis64
    on the scene against the whole mesh and its largest component, as tests/golden/make_mesh_components_golden.py stored them
    (each takes every ray against every triangle in NumPy: too slow to repeat in every test)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_components_scene.npz'))
    assert z['inputs'].tobytes().hex() == scene_digest(), "the scene changed: run tests/golden/make_mesh_components_golden.py"
    return {k: {'emu': z[k + '_emu'], 'lvis': z[k + '_lvis'].astype(np.float64), 'edge': z[k + '_edge']} for k in ('whole', 'largest')}


def scene_cos():
    """float64 [96, 128]: normal . dir of every (row, light) pair, as mesh_cases.oracle_lvis64 forms it."""
    xyz, normal, _, lxyz = scene_rows()
    p, q = xyz.astype(np.float64)[:, None, :], lxyz.astype(np.float64)[None, :, :]
    d = (q - p) / np.linalg.norm(q - p, axis=-1, keepdims=True)
    return (normal.astype(np.float64)[:, None, :] * d).sum(-1)


def filter_numpy(vertices, faces, label, keep_largest=0, min_faces=0):
    """(vertices', faces', info) of mesh.filter_by_labels on NumPy arrays through CPU tensors."""
    import torch
    from nerfactor_amd import mesh
    v, f, _, info = mesh.filter_by_labels(torch.from_numpy(np.array(vertices)), torch.from_numpy(np.array(faces)),
                                          torch.from_numpy(np.array(label)), keep_largest, min_faces)
    return v.numpy(), f.numpy(), info
