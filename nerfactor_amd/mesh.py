"""mesh — triangle meshes, rays against them on the GPU, and the perspective camera that makes the rays: what
data_gen/dtu_mvs/surf_from_mvs.py takes from trimesh (load, face_normals, ray.ray_pyembree.RayMeshIntersector), OpenCV
(decomposeProjectionMatrix) and xiuminglib (camera.PerspCam, geometry.sph.sph2cart) in the reference.  The mesh, the tree
build (ops.mesh_bvh_build, host code of libnfx) and the camera are host-side NumPy; every ray is cast by the two kernels of
csrc/mesh_cast.hip (ops.mesh_cast, ops.mesh_lvis), which have no CPU path.  Connected components: the labels come from
csrc/mesh_components.hip (ops.mesh_components); filter_by_labels, which selects and re-indexes, is plain torch."""
import numpy as np

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply(path):
    """(vertices float64 [nv, 3], faces int32 [nf, 3]) of a PLY file: `ascii` or `binary_little_endian`; float or double x, y, z
    (other vertex properties are skipped); faces as `list uchar int|uint vertex_indices|vertex_index`, triangles only.
    Anything else raises ValueError."""
    with open(path, 'rb') as h:
        data = h.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    body = data[data.index(b'\n', end) + 1:]
    fmt, elements = None, []       # elements: [name, count, [(kind, name, types...)]]
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == 'property':
            if tok[1] == 'list':
                elements[-1][2].append(('list', tok[4], tok[2], tok[3]))
            else:
                elements[-1][2].append(('scalar', tok[2], tok[1]))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError("%s: PLY format %r is not supported (ascii, binary_little_endian)" % (path, fmt))
    vertices = faces = None
    ascii_lines = body.decode('ascii', 'replace').splitlines() if fmt == 'ascii' else None
    pos = 0
    for name, count, props in elements:
        if any(p[0] == 'list' for p in props):
            if name != 'face':
                raise ValueError("%s: a list property outside the face element (%s)" % (path, name))
            if len(props) != 1 or props[0][1] not in ('vertex_indices', 'vertex_index') or _PLY_TYPES.get(props[0][2]) != 'u1' \
                    or _PLY_TYPES.get(props[0][3]) not in ('i4', 'u4'):
                raise ValueError("%s: faces must be `property list uchar int|uint vertex_indices`" % path)
            if fmt == 'ascii':
                rows = [ascii_lines[pos + i].split() for i in range(count)]
                pos += count
                if any(len(r) != 4 or r[0] != '3' for r in rows):
                    raise ValueError("%s: only triangles are supported" % path)
                faces = np.array([r[1:] for r in rows], dtype=np.int64).reshape(-1, 3)
            else:
                rec = np.frombuffer(body, dtype=np.dtype([('n', 'u1'), ('v', '<' + _PLY_TYPES[props[0][3]], 3)]), count=count, offset=pos) \
                    if count * 13 <= len(body) - pos else None
                if rec is None or (rec['n'] != 3).any():
                    raise ValueError("%s: only triangles are supported" % path)
                pos += count * 13
                faces = rec['v'].astype(np.int64)
        else:
            dt = np.dtype([(p[1], '<' + _PLY_TYPES[p[2]]) for p in props])
            if fmt == 'ascii':
                rows = np.array([ascii_lines[pos + i].split() for i in range(count)], dtype=np.float64).reshape(count, len(props))
                pos += count
                cols = {p[1]: rows[:, k] for k, p in enumerate(props)}
            else:
                rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                cols = {p[1]: rec[p[1]] for p in props}
            if name == 'vertex':
                if not all(k in cols for k in 'xyz') or any(_PLY_TYPES[p[2]] not in ('f4', 'f8') for p in props if p[1] in 'xyz'):
                    raise ValueError("%s: the vertex element needs float or double x, y, z" % path)
                vertices = np.stack([cols['x'], cols['y'], cols['z']], axis=1).astype(np.float64)
    if vertices is None or faces is None:
        raise ValueError("%s: no vertex or no face element" % path)
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (path, vertices.shape[0]))
    return vertices, faces.astype(np.int32)


def write_ply(path, vertices, faces, binary=True, normals=None):
    """The triangle mesh as a PLY file with float x, y, z and `list uchar int vertex_indices` faces; with `normals` [nv, 3]
    also float nx, ny, nz per vertex."""
    v = np.asarray(vertices, dtype='<f4').reshape(-1, 3)
    f = np.asarray(faces, dtype='<i4').reshape(-1, 3)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        n = np.asarray(normals, dtype='<f4').reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("write_ply: %d normals for %d vertices" % (n.shape[0], v.shape[0]))
        v = np.ascontiguousarray(np.concatenate((v, n), 1))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    head = ("ply\nformat %s 1.0\nelement vertex %d\n%s"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % ('binary_little_endian' if binary else 'ascii', v.shape[0], props, f.shape[0]))
    with open(path, 'wb') as h:
        h.write(head.encode('ascii'))
        if binary:
            h.write(v.tobytes())
            rec = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('v', '<i4', 3)]))
            rec['n'], rec['v'] = 3, f
            h.write(rec.tobytes())
        else:
            for row in v:
                h.write((' '.join('%r' % float(x) for x in row) + '\n').encode('ascii'))
            for row in f:
                h.write(('3 %d %d %d\n' % tuple(int(x) for x in row)).encode('ascii'))


def check_filter(keep_largest, min_faces):
    """(K, M) as ints of a component filter; a negative number, or no criterion at all, is refused."""
    try:
        k, m = int(keep_largest), int(min_faces)
        exact = k == keep_largest and m == min_faces
    except (TypeError, ValueError):
        exact = False
    if not exact or k < 0 or m < 0:
        raise ValueError("component filter: keep_largest = %r and min_faces = %r must be integers >= 0" % (keep_largest, min_faces))
    if k == 0 and m == 0:
        raise ValueError("component filter: keep_largest = 0 and min_faces = 0 keep every component: give one of them")
    return k, m


def filter_by_labels(vertices, faces, label, keep_largest=0, min_faces=0, attrs=()):
    """(vertices', faces', attrs', info): the mesh without the components that fail the filter.  Pure torch on the tensors'
    own device (CPU tensors work).  vertices [nv, 3], faces integer [nf, 3], label integer [nv] with label[v] = the smallest
    vertex index of v's component (ops.mesh_components), attrs: per-vertex tensors [nv, k].

    A face belongs to the component of its first vertex; a component's size is its number of faces, duplicate and degenerate
    faces included.  keep_largest = K >= 1 keeps the K components with the most faces (equal sizes: the smaller label first),
    min_faces = M >= 1 those with at least M faces; with both a component must pass both; with neither the call is refused.
    A vertex survives if and only if a surviving face names it, so vertices that no face names are always dropped.  Surviving
    vertices and faces keep their relative order; the faces are re-indexed, the attrs gathered with the same index.  A filter
    that keeps nothing returns (0, 3) shapes.
    info: n_components (with at least one face), n_unreferenced (vertices that no face names), kept = [(label, faces,
    vertices)] in ascending label order, dropped_faces, dropped_vertices, vertex_index (int64 tensor: the old index of every
    surviving vertex).
    Vertices are not welded: a triangle soup (every triangle with three vertices of its own) has one component per triangle."""
    import torch
    k, m = check_filter(keep_largest, min_faces)
    if vertices.dim() != 2 or faces.dim() != 2 or faces.shape[1] != 3 or label.dim() != 1 or label.shape[0] != vertices.shape[0]:
        raise ValueError("filter_by_labels: vertices [nv, 3], faces [nf, 3] and label [nv] are expected, got %s, %s and %s"
                         % (tuple(vertices.shape), tuple(faces.shape), tuple(label.shape)))
    attrs = tuple(attrs)
    for a in attrs:
        if a.shape[0] != vertices.shape[0]:
            raise ValueError("filter_by_labels: an attribute of %d rows for %d vertices" % (a.shape[0], vertices.shape[0]))
    nv, nf = vertices.shape[0], faces.shape[0]
    if nf and (int(faces.min()) < 0 or int(faces.max()) >= nv):
        raise ValueError("filter_by_labels: a face names a vertex outside [0, %d)" % nv)
    idx = faces.long()
    face_label = label.long()[idx[:, 0]]
    comp, sizes = torch.unique(face_label, return_counts=True)          # ascending labels
    keep = torch.ones_like(comp, dtype=torch.bool)
    if m:
        keep &= sizes >= m
    if k:
        top = torch.zeros_like(keep)
        top[torch.sort(sizes, descending=True, stable=True).indices[:k]] = True    # stable: equal sizes in label order
        keep &= top
    keep_face = keep[torch.searchsorted(comp, face_label)]
    idx = idx[keep_face]
    referenced = torch.zeros(nv, dtype=torch.bool, device=faces.device)
    referenced[faces.long().reshape(-1)] = True
    keep_vertex = torch.zeros(nv, dtype=torch.bool, device=faces.device)
    keep_vertex[idx.reshape(-1)] = True
    vertex_index = keep_vertex.nonzero()[:, 0]
    new_index = torch.cumsum(keep_vertex, 0) - 1
    kept_label, kept_vertices = torch.unique(label.long()[vertex_index], return_counts=True)
    info = {'n_components': int(comp.numel()), 'n_unreferenced': nv - int(referenced.sum()),
            'kept': list(zip(kept_label.tolist(), sizes[keep].tolist(), kept_vertices.tolist())),
            'dropped_faces': nf - int(idx.shape[0]), 'dropped_vertices': nv - int(vertex_index.numel()),
            'vertex_index': vertex_index}
    return vertices[vertex_index], new_index[idx].to(faces.dtype), tuple(a[vertex_index] for a in attrs), info


def filter_clause(info, seconds=None):
    """The drivers' log clause of a component filter."""
    text = "%d components, %d kept, %d triangles and %d vertices dropped" % (info['n_components'], len(info['kept']),
                                                                             info['dropped_faces'], info['dropped_vertices'])
    return text if seconds is None else text + ", components %.3f s" % seconds


class TriMesh:
    """vertices [nv, 3] float64 and faces [nf, 3] int32 with trimesh's face normals; the kernels see the vertices as float32."""

    def __init__(self, vertices, faces):
        self.vertices = np.array(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.array(faces, dtype=np.int32).reshape(-1, 3)
        self._normals = None
        self._bvh = {}

    @classmethod
    def load(cls, path):
        return cls(*read_ply(path))

    @property
    def face_normals(self):
        """[nf, 3]: normalize(cross(v1 - v0, v2 - v0)); zeros for a zero-area face."""
        if self._normals is None:
            tri = self.vertices[self.faces]
            n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            length = np.linalg.norm(n, axis=1, keepdims=True)
            self._normals = np.divide(n, length, out=np.zeros_like(n), where=length > 0)
        return self._normals

    def filter_components(self, keep_largest=0, min_faces=0, device=None):
        """A new TriMesh without the components that fail the filter (filter_by_labels' rules; its info as `.filter_info`):
        the faces are uploaded, labelled on the GPU (ops.mesh_components) and the labels downloaded.  Vertices are not welded
        first: a PLY stored as a triangle soup has one component per triangle."""
        import torch
        from . import ops
        check_filter(keep_largest, min_faces)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("labelling components needs an MI355X: libnfx has no CPU path")
            from . import dist as nfx_dist
            device = nfx_dist.local_device()
        label = ops.mesh_components(torch.from_numpy(self.faces).to(device).contiguous(), self.vertices.shape[0]).cpu()
        v, f, _, info = filter_by_labels(torch.from_numpy(self.vertices), torch.from_numpy(self.faces), label, keep_largest, min_faces)
        out = TriMesh(v.numpy(), f.numpy())
        out.filter_info = info
        return out

    def bvh(self, max_leaf=4, device=None):
        """(blob on the device, its 32-byte header on the host); built and uploaded once per (max_leaf, device)."""
        import torch
        from . import ops
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("casting rays needs an MI355X: libnfx has no CPU path")
            from . import dist as nfx_dist
            device = nfx_dist.local_device()
        key = (int(max_leaf), str(torch.device(device)))
        if key not in self._bvh:
            host = ops.mesh_bvh_build(self.vertices.astype(np.float32), self.faces, max_leaf)
            self._bvh[key] = (torch.from_numpy(host).to(device), host[:32].copy())
        return self._bvh[key]


class RayMeshIntersector:
    """trimesh.ray.ray_pyembree.RayMeshIntersector as far as the driver uses it, on nfx_mesh_cast / nfx_mesh_lvis."""

    def __init__(self, mesh, max_leaf=4, device=None):
        self.mesh, self.max_leaf, self.device = mesh, max_leaf, device

    def _dev(self, a, blob):
        import torch
        if isinstance(a, torch.Tensor):
            return a.to(device=blob.device, dtype=torch.float32)
        return torch.as_tensor(np.array(a, dtype=np.float32), device=blob.device)

    def cast(self, origins, dirs):
        """(t [n] float32, tri [n] int32) device tensors: the closest hit per ray; +inf and -1 for a miss."""
        from . import ops
        blob, header = self.mesh.bvh(self.max_leaf, self.device)
        return ops.mesh_cast(blob, header, self._dev(origins, blob).reshape(-1, 3), self._dev(dirs, blob).reshape(-1, 3))

    def intersects_location(self, origins, dirs, multiple_hits=False):
        """(locs [m, 3], ray_ind [m], tri_ind [m]) NumPy arrays of the m rays that hit, first hit only; locs = o + t d in float32."""
        if multiple_hits:
            raise NotImplementedError("multiple_hits=True")
        blob, _ = self.mesh.bvh(self.max_leaf, self.device)
        o, d = self._dev(origins, blob).reshape(-1, 3), self._dev(dirs, blob).reshape(-1, 3)
        t, tri = self.cast(o, d)
        hit = tri >= 0
        locs = o[hit] + t[hit][:, None] * d[hit]
        return locs.cpu().numpy(), hit.nonzero()[:, 0].cpu().numpy(), tri[hit].cpu().numpy().astype(np.int64)

    def light_visibility(self, xyz, normal, alpha, lxyz, eps, out=None):
        """[n, L] device tensor: alpha where light l is in front of row i's surface and unoccluded, else 0."""
        from . import ops
        blob, header = self.mesh.bvh(self.max_leaf, self.device)
        return ops.mesh_lvis(blob, header, self._dev(xyz, blob).reshape(-1, 3), self._dev(normal, blob).reshape(-1, 3),
                             self._dev(alpha, blob).reshape(-1), self._dev(lxyz, blob).reshape(-1, 3), eps, out=out)


def sph2cart(r_lat_lng):
    """(r, latitude, longitude) -> (x, y, z), xiuminglib's lat-lng convention: z = r sin(lat), x = r cos(lat) cos(lng)."""
    p = np.asarray(r_lat_lng, dtype=np.float64)
    r, lat, lng = p[..., 0], p[..., 1], p[..., 2]
    return np.stack((r * np.cos(lat) * np.cos(lng), r * np.cos(lat) * np.sin(lng), r * np.sin(lat)), axis=-1)


def decompose_projection(P):
    """P [3, 4] -> (K, R, t) with K [R | t] = P, K upper triangular with a positive diagonal and det R = +1: the RQ
    decomposition of P[:, :3] (scipy.linalg.rq) with the signs moved between the factors.  For a projection matrix with
    positive focal lengths and det P[:, :3] > 0 — DTU's are — this is what cv2.decomposeProjectionMatrix returns as camera
    and rotation matrix; for det P[:, :3] < 0 the whole of P is negated first (the same projection)."""
    from scipy.linalg import rq
    P = np.asarray(P, dtype=np.float64)
    if P.shape != (3, 4):
        raise ValueError("a 3 x 4 projection matrix is expected, got %s" % (P.shape,))
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    K, R = rq(P[:, :3])
    sign = np.diag(np.where(np.diag(K) < 0, -1., 1.))
    K, R = K.dot(sign), sign.dot(R)
    return K, R, np.linalg.solve(K, P[:, 3])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class PerspCam:
    """The parts of xiuminglib.camera.PerspCam that surf_from_mvs.py uses: a computer-vision camera (+x right, +y down, +z the
    viewing direction) given by loc / lookat / up or by its 3 x 4 object-to-camera matrix, one focal length in pixels, and
    the principal point at the image centre."""

    def __init__(self, f_pix=533.33, im_res=(256, 256), loc=(1, 1, 1), lookat=(0, 0, 0), up=(0, 1, 0)):
        self.f_pix = float(f_pix)
        self.im_h, self.im_w = int(im_res[0]), int(im_res[1])
        self.loc, self.lookat, self.up = np.array(loc, dtype=float), np.array(lookat, dtype=float), np.array(up, dtype=float)

    @property
    def int_mat(self):
        return np.array([[self.f_pix, 0, self.im_w / 2], [0, self.f_pix, self.im_h / 2], [0, 0, 1]])

    @int_mat.setter
    def int_mat(self, mat):
        mat = np.array(mat, dtype=float)
        assert mat.shape == (3, 3) and mat[1, 0] == 0 and mat[0, 1] == 0 and all(mat[2, :] == [0, 0, 1]), "not a skew-free K"
        assert mat[0, 0] == mat[1, 1], "X and Y focal lengths are different"
        w, h = mat[0, 2] * 2, mat[1, 2] * 2
        assert w == int(w) and h == int(h), "the principal point is not at the centre of an integer-sized image"
        self.f_pix, self.im_w, self.im_h = float(mat[0, 0]), int(w), int(h)

    @property
    def ext_mat(self):
        cvz = self.lookat - self.loc
        assert np.linalg.norm(cvz) > 0, "Camera location and look-at coincide"
        cvx = np.cross(cvz, self.up)
        cvy = np.cross(cvz, cvx)
        rot_obj2cv = np.linalg.inv(np.vstack((_unit(cvx), _unit(cvy), _unit(cvz))).T)
        return rot_obj2cv.dot(np.hstack((np.eye(3), -self.loc.reshape(3, 1))))

    @ext_mat.setter
    def ext_mat(self, o2c):
        o2c = np.array(o2c, dtype=float)
        assert o2c.shape == (3, 4), "a 3 x 4 object-to-camera matrix is expected"
        rot = o2c[:, :3]
        assert np.allclose(rot.dot(rot.T), np.eye(3), atol=1e-6) and abs(np.linalg.det(rot) - 1) < 1e-6, \
            "The R part of object-to-camera is not a valid rotation matrix"
        c2o = np.linalg.inv(np.vstack((o2c, [0, 0, 0, 1])))
        at = lambda p: (c2o.dot(np.append(p, 1.)))[:3] / (c2o.dot(np.append(p, 1.)))[3]
        self.loc = at([0, 0, 0])
        self.lookat = at([0, 0, 1])
        self.up = at([0, -1, 0]) - self.loc

    def gen_rays(self):
        """[H, W, 1, 3] unit ray directions through the pixel centres (one sample per pixel); the origin is `loc`."""
        v, h = np.meshgrid(np.arange(self.im_h), np.arange(self.im_w), indexing='ij')
        hs, vs = (h.ravel() + 0.5), (v.ravel() + 0.5)
        zs = np.ones(hs.shape, dtype=float)
        pts = np.vstack((zs * (hs - self.im_w / 2) / self.f_pix, zs * (vs - self.im_h / 2) / self.f_pix, zs, zs))
        c2o = np.linalg.inv(np.vstack((self.ext_mat, [0, 0, 0, 1])))
        pts_o = c2o.dot(pts)
        xyz = (pts_o[:3] / pts_o[3]).T.reshape(self.im_h, self.im_w, 3)
        return _unit(xyz - self.loc)[:, :, None, :]
