"""Scenes, rays and the two oracles of the mesh ray-cast tests (tests/test_cpu_mesh_cast.py, tests/test_gpu_mesh_cast.py).

Scenes are at DTU scale (coordinates of several hundred, camera 1400 away), so fp32 rounding is visible:
  S1  a twice-subdivided icosphere of radius 300 centred at (50, -30, 600) over an 8 x 8-quad ground grid, 1600 wide, at
      z = 930 (+z is down, as in DTU): 320 + 128 = 448 triangles, real cast shadows and real misses
  S2  S1 plus a zero-area triangle (a repeated vertex), an exact duplicate of a sphere triangle (equal t: the smaller index
      wins) and a far-away sliver
  S3  one triangle;  S4  five triangles (not a multiple of max_leaf = 4)
Rays: a 32 x 40 look-at view from (400, 200, -700) with seeded sub-pixel jitter, directions NOT normalised.

Oracle (a), `oracle64`: float64 Moeller-Trumbore over all triangles, smallest t > 0, the smaller index at equal t, both
faces.  It also flags EDGE rays: a ray that crosses the plane of some triangle in front of it within 1e-5 (barycentric) of
that triangle's boundary, |min(u, v, w)| < 1e-5 — where a different rounding may legitimately pick the neighbour or miss.

Oracle (b), `emu_*`: a NumPy float32 emulation of csrc/mesh_cast.hip in the operation order written down there (every
intermediate is float32, no fused multiply-add, IEEE division and square root; the fp64 fallback where an edge function is
exactly 0).  `emu_cast_brute` tests every triangle; `emu_cast_tree` walks the builder's blob with the kernel's stackless
loop and its box test.  The GPU must equal (b) bit for bit; (b) must equal (a) off the edge rays."""
import functools

import numpy as np

F32 = np.float32
CAM = np.array((400., 200., -700.))
CENTRE = np.array((50., -30., 600.))
EDGE_TOL = 1e-5
LVIS_EPS = 0.1           # the driver's default --lvis_eps
LVIS_RADIUS = 1e5        # ... and --lvis_radius
DUP = 41                 # the sphere triangle that S2 holds twice (three rays of the view hit it)


# ------------------------------------------------------------------------------------------------ scenes
def icosphere(subdiv, radius, centre):
    p = (1 + 5 ** .5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, dtype=np.float64), np.array(f, dtype=np.int32)


def ground(nq=8, width=1600., z=930., centre=(50., -30.)):
    g = np.linspace(-width / 2, width / 2, nq + 1)
    xs, ys = np.meshgrid(g + centre[0], g + centre[1], indexing='ij')
    v = np.stack((xs.ravel(), ys.ravel(), np.full(xs.size, z)), axis=1)
    f = []
    for i in range(nq):
        for j in range(nq):
            a, b, c, d = i * (nq + 1) + j, (i + 1) * (nq + 1) + j, (i + 1) * (nq + 1) + j + 1, i * (nq + 1) + j + 1
            f += [(a, c, b), (a, d, c)]      # normals towards -z, the camera's side
    return v, np.array(f, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(vertices float32 [nv, 3], faces int32 [nf, 3]); read-only arrays."""
    sv, sf = icosphere(2, 300., CENTRE)
    gv, gf = ground()
    v = np.vstack((sv, gv))
    f = np.vstack((sf, gf + sv.shape[0]))
    if name == 'S2':
        n = v.shape[0]
        extra = np.array(((60., -20., 100.), (60., -20., 100.), (90., 10., 120.),          # zero area: a repeated vertex
                          (5000., 5000., 5000.), (5000.001, 5000., 5000.), (5400., 5001., 5000.)))   # a far sliver
        v = np.vstack((v, extra))
        f = np.vstack((f, [(n, n + 1, n + 2)], sf[DUP:DUP + 1], [(n + 3, n + 4, n + 5)]))    # ... and a duplicate of triangle DUP
    elif name == 'S3':
        v, f = np.array(((-200., -250., 640.), (330., -100., 560.), (20., 290., 700.))), np.array(((0, 1, 2),))
    elif name == 'S4':
        v = np.array(((-300., -300., 600.), (300., -300., 600.), (300., 300., 640.), (-300., 300., 640.), (50., -30., 380.),
                      (50., -30., 900.)))
        f = np.array(((0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (0, 1, 5)))
    elif name != 'S1':
        raise KeyError(name)
    v, f = v.astype(F32), f.astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


SCENES = ('S1', 'S2', 'S3', 'S4')
RAY_COUNTS = (1280, 1, 63, 65)


@functools.lru_cache(maxsize=None)
def view_rays(h=32, w=40, seed=0):
    """(rayo, rayd) float32 [h * w, 3]: the look-at view with sub-pixel jitter; directions are not unit vectors."""
    rng = np.random.RandomState(seed)
    z = (CENTRE - CAM) / np.linalg.norm(CENTRE - CAM)
    x = np.cross(z, (0., 0., -1.))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    f = h / 2 / np.tan(np.radians(32.))
    vs, hs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    jit = rng.uniform(-0.5, 0.5, size=(2, h, w))
    px, py = hs + 0.5 + jit[0] - w / 2, vs + 0.5 + jit[1] - h / 2
    d = px[..., None] * x + py[..., None] * y + f * z
    rayd = d.reshape(-1, 3).astype(F32)
    rayo = np.tile(CAM, (h * w, 1)).astype(F32)
    rayo.setflags(write=False)
    rayd.setflags(write=False)
    return rayo, rayd


def rays(n):
    """the first n rays of a fixed permutation of the view (all 1280 in image order for n = 1280)"""
    o, d = view_rays()
    if n == o.shape[0]:
        return o, d
    idx = np.random.RandomState(1).permutation(o.shape[0])[:n]
    return o[idx], d[idx]


def light_xyz(light_h):
    """[2 light_h^2, 3] float32 light positions as the driver makes them for S1: the reference's gen_light_xyz at LVIS_RADIUS,
    moved to the mesh centre, z flipped."""
    from nerfactor_amd.brdf.renderer import gen_light_xyz
    lxyz, _ = gen_light_xyz(light_h, 2 * light_h, envmap_radius=LVIS_RADIUS)
    lxyz = np.array(lxyz, dtype=np.float64) + scene('S1')[0].astype(np.float64).mean(axis=0)
    lxyz[:, :, 2] = -lxyz[:, :, 2]
    return lxyz.reshape(-1, 3).astype(F32)


# ------------------------------------------------------------------------------------------------ oracle (a): float64
def oracle64(vertices, faces, rayo, rayd, chunk=4096):
    """dict(t [n] float64 (+inf), tri [n] (-1), edge [n] bool) of float64 rays against all triangles."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    o_all, d_all = np.asarray(rayo, dtype=np.float64).reshape(-1, 3), np.asarray(rayd, dtype=np.float64).reshape(-1, 3)
    n = o_all.shape[0]
    out_t, out_tri, out_edge = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool)
    with np.errstate(all='ignore'):
        for lo in range(0, n, chunk):
            o, d = o_all[lo:lo + chunk, None, :], d_all[lo:lo + chunk, None, :]
            p = np.cross(d, e2[None])
            det = (e1[None] * p).sum(-1)
            s = o - v0[None]
            u = (s * p).sum(-1) / det
            q = np.cross(s, e1[None])
            v = (d * q).sum(-1) / det
            t = (e2[None] * q).sum(-1) / det
            front = (det != 0) & (t > 0)
            m = np.minimum(np.minimum(u, v), 1 - u - v)
            hit = front & (m >= 0)
            tt = np.where(hit, t, np.inf)
            best = tt.argmin(axis=1)
            bt = tt[np.arange(tt.shape[0]), best]
            out_t[lo:lo + chunk] = bt
            out_tri[lo:lo + chunk] = np.where(np.isfinite(bt), best, -1)
            out_edge[lo:lo + chunk] = (front & (np.abs(m) < EDGE_TOL)).any(axis=1)
    return {'t': out_t, 'tri': out_tri, 'edge': out_edge}


# ------------------------------------------------------------------------------------------------ oracle (b): fp32 emulation
def _pick(k, a0, a1, a2):
    return np.where(k == 0, a0, np.where(k == 1, a1, a2))


def ray_setup32(rayo, rayd):
    """The per-ray constants of mesh_cast.hip's Ray, float32 [n] each."""
    o, d = np.asarray(rayo, dtype=F32).reshape(-1, 3), np.asarray(rayd, dtype=F32).reshape(-1, 3)
    with np.errstate(all='ignore'):
        ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
        ad = np.abs(d)
        kz = np.zeros(o.shape[0], dtype=np.int64)
        m = ad[:, 0].copy()
        sel = ad[:, 1] > m
        kz[sel], m[sel] = 1, ad[sel, 1]
        kz[ad[:, 2] > m] = 2
        kx = np.where(kz == 2, 0, kz + 1)
        ky = np.where(kx == 2, 0, kx + 1)
        dz = _pick(kz, d[:, 0], d[:, 1], d[:, 2])
        kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
        one = F32(1)
        return {'o': o, 'ok': ok, 'kx': kx, 'ky': ky, 'kz': kz, 'sx': _pick(kx, d[:, 0], d[:, 1], d[:, 2]) / dz,
                'sy': _pick(ky, d[:, 0], d[:, 1], d[:, 2]) / dz, 'sz': one / dz, 'inv': one / d}


def tri_t32(R, p0, p1, p2, sel=None, extra_axis=False):
    """t float32 of Ray::hit (not > 0 for a miss).  R: ray_setup32; p0, p1, p2 [..., 3] float32 broadcastable against the
    rays (`sel`: a subset of the rays; extra_axis: rays [n, 1] against triangles [1, m])."""
    def r(key):
        a = R[key] if sel is None else R[key][sel]
        return a[:, None] if extra_axis else a
    o = R['o'] if sel is None else R['o'][sel]
    if extra_axis:
        o = o[:, None, :]
    kx, ky, kz, sx, sy, sz = r('kx'), r('ky'), r('kz'), r('sx'), r('sy'), r('sz')
    with np.errstate(all='ignore'):
        a, b, c = p0 - o, p1 - o, p2 - o
        assert a.dtype == F32
        az, bz, cz = _pick(kz, a[..., 0], a[..., 1], a[..., 2]), _pick(kz, b[..., 0], b[..., 1], b[..., 2]), _pick(kz, c[..., 0], c[..., 1], c[..., 2])
        ax, ay = _pick(kx, a[..., 0], a[..., 1], a[..., 2]) - sx * az, _pick(ky, a[..., 0], a[..., 1], a[..., 2]) - sy * az
        bx, by = _pick(kx, b[..., 0], b[..., 1], b[..., 2]) - sx * bz, _pick(ky, b[..., 0], b[..., 1], b[..., 2]) - sy * bz
        cx, cy = _pick(kx, c[..., 0], c[..., 1], c[..., 2]) - sx * cz, _pick(ky, c[..., 0], c[..., 1], c[..., 2]) - sy * cz
        u, v, w = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        z = (u == 0) | (v == 0) | (w == 0)
        if z.any():
            D = np.float64
            u = np.where(z, (cx.astype(D) * by.astype(D) - cy.astype(D) * bx.astype(D)).astype(F32), u)
            v = np.where(z, (ax.astype(D) * cy.astype(D) - ay.astype(D) * cx.astype(D)).astype(F32), v)
            w = np.where(z, (bx.astype(D) * ay.astype(D) - by.astype(D) * ax.astype(D)).astype(F32), w)
        mixed = ((u < 0) | (v < 0) | (w < 0)) & ((u > 0) | (v > 0) | (w > 0))
        det = (u + v) + w
        tt = (u * (sz * az) + v * (sz * bz)) + w * (sz * cz)
        t = tt / det
        assert t.dtype == F32
        return np.where(mixed | (det == 0), F32(-1), t)


def emu_cast_brute(vertices, faces, rayo, rayd, any_hit=False, chunk=4096):
    """(t float32 [n], tri int32 [n]) of the emulated triangle test over ALL triangles; any_hit: bool [n] instead."""
    tri = np.asarray(vertices, dtype=F32)[np.asarray(faces)]
    R = ray_setup32(rayo, rayd)
    n = R['o'].shape[0]
    out_t, out_tri = np.full(n, np.inf, dtype=F32), np.full(n, -1, dtype=np.int32)
    for lo in range(0, n, chunk):
        sel = slice(lo, min(lo + chunk, n))
        t = tri_t32(R, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], sel=sel, extra_axis=True)
        tt = np.where((t > 0) & R['ok'][sel, None], t, F32(np.inf))
        best = tt.argmin(axis=1)
        bt = tt[np.arange(tt.shape[0]), best]
        out_t[sel] = bt
        out_tri[sel] = np.where(bt < np.inf, best, -1)
    return (out_tri >= 0) if any_hit else (out_t, out_tri)


def parse_blob(blob):
    """The builder's blob -> dict(header fields, lo/hi [n_nodes + 1, 3], skip, first [n_nodes + 1], tris [nf, 3, 3], orig [nf])."""
    raw = np.ascontiguousarray(blob, dtype=np.uint8)
    head = raw[:32].view(np.int32)
    out = {'magic': int(raw[:4].view(np.uint32)[0]), 'version': int(head[1]), 'n_nodes': int(head[2]), 'n_tris': int(head[3]),
           'max_leaf': int(head[4])}
    nn, nt = out['n_nodes'], out['n_tris']
    assert raw.size == 32 + (nn + 1) * 32 + nt * 48, (raw.size, nn, nt)
    nodes = raw[32:32 + (nn + 1) * 32]
    nf32, ni32 = nodes.view(F32).reshape(nn + 1, 8), nodes.view(np.int32).reshape(nn + 1, 8)
    tris = raw[32 + (nn + 1) * 32:]
    tf32, ti32 = tris.view(F32).reshape(nt, 12), tris.view(np.int32).reshape(nt, 12)
    out.update(lo=nf32[:, 0:3], hi=nf32[:, 4:7], skip=ni32[:, 3], first=ni32[:, 7], tris=tf32.reshape(nt, 3, 4)[:, :, :3], orig=ti32[:, 3])
    return out


def emu_cast_tree(blob, rayo, rayd, any_hit=False):
    """The kernel's stackless walk over the blob, all rays in lockstep: (t, tri, nodes visited [n], triangles tested [n]);
    any_hit: (hit bool [n], nodes, triangles)."""
    B = parse_blob(blob)
    nn, nt = B['n_nodes'], B['n_tris']
    R = ray_setup32(rayo, rayd)
    o, inv = R['o'], R['inv']
    n = o.shape[0]
    best_t, best_tri = np.full(n, np.inf, dtype=F32), np.full(n, -1, dtype=np.int32)
    node = np.where(R['ok'], 0, nn)
    visited, tested = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    slack = F32(1.0 / 262144.0)
    sub_first = np.where(B['first'] < 0, -B['first'] - 1, B['first'])
    with np.errstate(all='ignore'):
        for _ in range(nn):
            act = np.nonzero(node < nn)[0]
            if act.size == 0:
                break
            nd = node[act]
            visited[act] += 1
            lo, hi = B['lo'][nd] - o[act], B['hi'][nd] - o[act]
            dmax = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
            s = (slack * dmax)[:, None]
            a, b = (lo - s) * inv[act], (hi + s) * inv[act]
            tn = np.fmax(np.fmax(np.fmin(a[:, 0], b[:, 0]), np.fmin(a[:, 1], b[:, 1])), np.fmax(np.fmin(a[:, 2], b[:, 2]), F32(0)))
            tf = np.fmin(np.fmin(np.fmax(a[:, 0], b[:, 0]), np.fmax(a[:, 1], b[:, 1])), np.fmax(a[:, 2], b[:, 2]))
            go = (tn <= tf) & (tn <= best_t[act])
            skip = np.clip(B['skip'][nd], nd + 1, nn)
            inner = B['first'][nd] < 0
            nxt = np.where(go & inner, nd + 1, skip)
            leaf = go & ~inner
            if leaf.any():
                li = act[leaf]
                first, end = np.clip(B['first'][nd[leaf]], 0, nt), np.clip(sub_first[skip[leaf]], 0, nt)
                for k in range(int((end - first).max())):
                    on = first + k < end
                    if any_hit:
                        on &= best_tri[li] < 0
                    rr, ti = li[on], (first + k)[on]
                    tested[rr] += 1
                    t = tri_t32(R, B['tris'][ti, 0], B['tris'][ti, 1], B['tris'][ti, 2], sel=rr)
                    orig = B['orig'][ti]
                    better = (t > 0) & ((t < best_t[rr]) | ((t == best_t[rr]) & (orig < best_tri[rr])))
                    best_t[rr[better]], best_tri[rr[better]] = t[better], orig[better]
                if any_hit:
                    nxt[leaf] = np.where(best_tri[li] >= 0, nn, nxt[leaf])
            node[act] = nxt
    if any_hit:
        return best_tri >= 0, visited, tested
    return best_t, best_tri, visited, tested


def shadow_rays32(xyz, lxyz, eps):
    """(origin, dir) float32 [n, L, 3] in the kernel's operation order."""
    p, q = np.asarray(xyz, dtype=F32)[:, None, :], np.asarray(lxyz, dtype=F32)[None, :, :]
    with np.errstate(all='ignore'):
        e = q - p
        length = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        d = e / length[..., None]
        return p + F32(eps) * d, d


def emu_lvis(vertices, faces, xyz, normal, alpha, lxyz, eps):
    """lvis float32 [n, L] of the emulated kernel (brute force over the triangles), and cos [n, L] float32."""
    o, d = shadow_rays32(xyz, lxyz, eps)
    nrm, alpha = np.asarray(normal, dtype=F32)[:, None, :], np.asarray(alpha, dtype=F32)
    with np.errstate(all='ignore'):
        cos = (nrm[..., 0] * d[..., 0] + nrm[..., 1] * d[..., 1]) + nrm[..., 2] * d[..., 2]
        cast = (alpha[:, None] != 0) & (cos > 0)
    vis = np.zeros(cos.shape, dtype=F32)
    hit = emu_cast_brute(vertices, faces, o[cast], d[cast], any_hit=True, chunk=8192)
    vis[cast] = np.where(hit, F32(0), np.broadcast_to(alpha[:, None], cos.shape)[cast])
    return vis, cos


def oracle_lvis64(vertices, faces, xyz, normal, alpha, lxyz, eps):
    """dict(lvis, cos, edge [n, L]) in float64 from the same float32 inputs."""
    p, q = np.asarray(xyz, dtype=np.float64)[:, None, :], np.asarray(lxyz, dtype=np.float64)[None, :, :]
    with np.errstate(all='ignore'):
        d = (q - p) / np.linalg.norm(q - p, axis=-1, keepdims=True)
        o = p + float(eps) * d
        cos = (np.asarray(normal, dtype=np.float64)[:, None, :] * d).sum(-1)
    alpha = np.asarray(alpha, dtype=np.float64)
    cast = (alpha[:, None] != 0) & (cos > 0)
    res = oracle64(vertices, faces, o[cast], d[cast])
    vis, edge = np.zeros(cos.shape), np.zeros(cos.shape, dtype=bool)
    vis[cast] = np.where(res['tri'] >= 0, 0., np.broadcast_to(alpha[:, None], cos.shape)[cast])
    edge[cast] = res['edge']
    return {'lvis': vis, 'cos': cos, 'edge': edge}


@functools.lru_cache(maxsize=None)
def surface_rows(scene_name='S1'):
    """(xyz, normal, alpha) float32 of the 1280-ray view on a scene, as the driver makes them from the emulated cast: xyz = o + t d
    in float32 (0 for a miss), the hit face's normal ((0, 1, 0) for a miss), alpha 1 / 0."""
    from nerfactor_amd.mesh import TriMesh
    v, f = scene(scene_name)
    o, d = view_rays()
    t, tri = emu_cast_brute(v, f, o, d)
    hit = tri >= 0
    xyz = np.zeros((o.shape[0], 3), dtype=F32)
    xyz[hit] = o[hit] + t[hit][:, None] * d[hit]
    normal = np.tile(np.array((0, 1, 0), dtype=F32), (o.shape[0], 1))
    normal[hit] = TriMesh(v, f).face_normals[tri[hit]].astype(F32)
    return xyz, normal, hit.astype(F32)


@functools.lru_cache(maxsize=None)
def watertight_rays():
    """(rayo, rayd) float32: from the view's camera exactly at every vertex and every edge midpoint of S1's sphere, targets and
    directions made from the float32 vertex values (d = target - origin in float32)."""
    sv, sf = icosphere(2, 300., CENTRE)
    v = sv.astype(F32)
    edges = np.unique(np.sort(np.vstack((sf[:, [0, 1]], sf[:, [1, 2]], sf[:, [2, 0]])), axis=1), axis=0)
    targets = np.vstack((v, (v[edges[:, 0]] + v[edges[:, 1]]) * F32(0.5)))
    assert targets.dtype == F32 and targets.shape[0] == 162 + 480
    rayo = np.tile(CAM, (targets.shape[0], 1)).astype(F32)
    return rayo, targets - rayo
