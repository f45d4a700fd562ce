"""Marching tetrahedra on a scalar lattice, restated in NumPy from the rules of include/nfx.h — not
from the kernel: the tables by the geometric rule (floating-point midpoints on the unit cube), the vertices in fp32 in the
stated operation order, vertices and triangles in the stated order.  The yardstick of csrc/isosurface.hip."""
import itertools

import numpy as np

CLASS_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))     # lexicographic: tet 0..5


def tet_corners():
    """int [6, 4, 3]: corner n of tet t as an offset from the cell's lowest lattice point."""
    c = np.zeros((6, 4, 3), dtype=np.int64)
    for t, (p0, p1, _) in enumerate(PERMS):
        c[t, 1, p0] = 1
        c[t, 2, p0] = c[t, 2, p1] = 1
        c[t, 3] = 1
    return c


def tables():
    """(tri int8 [6, 16, 2, 3, 2], edge int8 [6, 4, 4, 4]) in the layout of nfx_isosurface_tables."""
    corners = tet_corners()
    tri = np.full((6, 16, 2, 3, 2), -1, dtype=np.int8)
    edge = np.full((6, 4, 4, 4), -1, dtype=np.int8)
    for t in range(6):
        for a in range(4):
            for b in range(a + 1, 4):
                d = tuple(int(x) for x in corners[t, b] - corners[t, a])
                edge[t, a, b] = (CLASS_OFFSETS.index(d),) + tuple(corners[t, a])
        for mask in range(16):
            inside = [n for n in range(4) if (mask >> n) & 1]
            outside = [n for n in range(4) if not (mask >> n) & 1]
            if len(inside) in (1, 3):
                lone, rest = (inside[0], outside) if len(inside) == 1 else (outside[0], inside)
                triangles = [[(lone, r) for r in rest]]
            elif len(inside) == 2:
                (i, j), (k, l) = inside, outside
                q = [(i, k), (i, l), (j, l), (j, k)]
                triangles = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                continue
            towards = corners[t, outside].mean(0) - corners[t, inside].mean(0)
            for r, verts in enumerate(triangles):
                mid = [(corners[t, a] + corners[t, b]) / 2. for a, b in verts]
                if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), towards) < 0:
                    verts = [verts[0], verts[2], verts[1]]
                tri[t, mask, r] = [(min(a, b), max(a, b)) for a, b in verts]
    return tri, edge


_TABLES = None


def extract(field, iso, origin=(0., 0., 0.), spacing=(1., 1., 1.)):
    """(vertices float32 [nv, 3], faces int32 [nf, 3]) of float32 field[nx, ny, nz]."""
    global _TABLES
    if _TABLES is None:
        _TABLES = tables()
    tri, edge = _TABLES
    corners = tet_corners()
    f = np.ascontiguousarray(field, dtype=np.float32)
    nx, ny, nz = f.shape
    assert min(f.shape) >= 2
    iso = np.float32(iso)
    origin, spacing = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        inside = f > iso
    # ---- vertices: ascending (owner's flat index, class)
    cross = np.zeros((nx, ny, nz, 7), dtype=bool)
    for cl, (dx, dy, dz) in enumerate(CLASS_OFFSETS):
        cross[:nx - dx, :ny - dy, :nz - dz, cl] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    cross = cross.reshape(-1, 7)
    owner, cl = np.nonzero(cross)
    vid = np.full(cross.shape, -1, dtype=np.int32)
    vid[owner, cl] = np.arange(owner.size, dtype=np.int32)
    idx = np.stack(np.unravel_index(owner, (nx, ny, nz)), 1)
    far = idx + np.asarray(CLASS_OFFSETS)[cl]
    fp, fq = f[tuple(idx.T)], f[tuple(far.T)]
    with np.errstate(all='ignore'):
        t = (iso - fp) / (fq - fp)
        p = origin + idx.astype(np.float32) * spacing
        q = origin + far.astype(np.float32) * spacing
        vertices = p + t[:, None] * (q - p)
    assert vertices.dtype == np.float32
    # ---- triangles: ascending (cell's flat index, tet, triangle)
    pattern = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)       # bit 4 dx + 2 dy + dz
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        pattern |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << (4 * dx + 2 * dy + dz)
    ci, cj, ck = np.nonzero((pattern != 0) & (pattern != 255))         # row-major: ascending flat index
    base = np.stack((ci, cj, ck), 1)
    pat = pattern[ci, cj, ck]
    faces = np.full((base.shape[0], 6, 2, 3), -1, dtype=np.int32)
    for tet in range(6):
        cid = 4 * corners[tet, :, 0] + 2 * corners[tet, :, 1] + corners[tet, :, 2]
        m4 = sum(((pat >> cid[n]) & 1) << n for n in range(4))
        for r in range(2):
            for v in range(3):
                a, b = tri[tet, m4, r, v, 0].astype(np.int64), tri[tet, m4, r, v, 1].astype(np.int64)
                have = a >= 0
                e = edge[tet, np.where(have, a, 0), np.where(have, b, 1)].astype(np.int64)
                own = base + e[:, 1:]
                flat = (own[:, 0] * ny + own[:, 1]) * nz + own[:, 2]
                faces[:, tet, r, v] = np.where(have, vid[flat, e[:, 0]], -1)
    keep = faces[..., 0] >= 0
    faces = faces[keep]
    assert faces.size == 0 or faces.min() >= 0
    return vertices.reshape(-1, 3), np.ascontiguousarray(faces.reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ mesh properties
def directed_edges(faces):
    """int64 [3 nf, 2]: the directed edges (v0, v1), (v1, v2), (v2, v0) of every triangle."""
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))


def unpaired_edges(faces):
    """The directed edges that do not occur exactly once with their reverse exactly once (empty for a closed, consistently
    oriented manifold mesh)."""
    e = directed_edges(faces)
    n = int(e.max()) + 1 if e.size else 1
    key, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    uniq, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    pos = np.clip(np.searchsorted(uniq, rev), 0, max(uniq.size - 1, 0))
    reverse = np.where(uniq[pos] == rev, count[pos], 0) if uniq.size else np.zeros(0, dtype=np.int64)
    bad = (count[inv.reshape(-1)] != 1) | (reverse != 1)
    return e[bad]


def euler_characteristic(vertices, faces):
    e = np.sort(directed_edges(faces), 1)
    return int(np.asarray(vertices).shape[0] - np.unique(e, axis=0).shape[0] + np.asarray(faces).shape[0])


def signed_volume(vertices, faces):
    """Positive when the normals (v1 - v0) x (v2 - v0) of a closed mesh point outwards."""
    t = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum('ij,ij->i', t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.)


def face_normals(vertices, faces):
    t = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
