#!/usr/bin/env python
"""Times the mesh ray cast at the size of one DTU view, on the GPU:

  build    nfx_mesh_bvh_build (host) of a procedurally displaced icosphere, 8 subdivisions = 1.31 M triangles, over a 64 x 64-quad
           ground grid, max_leaf 4;
  cast     one nfx_mesh_cast launch of a 256 x 320 camera view;
  lvis     one nfx_mesh_lvis launch of that view's surface points against 512 lights (shadow rays = the (point, light)
           pairs with alpha != 0 and normal . dir > 0, the ones that walk the tree).

Every launch is warmed up; a timed region is `inner` launches between two device events around a synchronised stretch, sized
to about a third of a second; `--reps` regions, median and spread (max - min) / median, per launch.  The mean number of nodes
visited and triangles tested per ray comes from the CPU emulation of the walk (tests/mesh_cases.py) on a sample of the
rays.  No threshold is asserted: nothing earlier exists to compare with.  One JSON line; --out FILE also writes it there.

    python scripts/bench_mesh_cast.py [--subdiv 8] [--reps 5] [--out profiles/mesh_cast/bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def region_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed(fn, reps):
    for _ in range(3):
        fn()
    inner = max(1, int(300. / max(region_ms(fn, 2), 1e-3)))
    ms = sorted(region_ms(fn, inner) for _ in range(reps))
    med = ms[len(ms) // 2]
    return {'ms_per_launch': med, 'spread': (ms[-1] - ms[0]) / med, 'launches_per_region': inner, 'regions': reps}


def displaced_icosphere(subdiv, radius, centre):
    """Vectorised subdivision of the unit icosahedron, then a smooth radial displacement of a few percent."""
    from tests import mesh_cases as mc
    v, f = mc.icosphere(0, 1., (0., 0., 0.))
    for _ in range(subdiv):
        e = np.sort(np.vstack((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1) + v.shape[0]
        ab, bc, ca = m[0], m[1], m[2]
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.vstack((np.stack((a, ab, ca), 1), np.stack((b, bc, ab), 1), np.stack((c, ca, bc), 1), np.stack((ab, bc, ca), 1))).astype(np.int32)
        v = np.vstack((v, mid))
    bump = 1 + 0.04 * np.sin(9 * v[:, 0]) * np.sin(7 * v[:, 1] + 1) + 0.02 * np.sin(23 * v[:, 2] + 2 * v[:, 0])
    return v * (radius * bump)[:, None] + np.asarray(centre), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subdiv', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=512, help="rays of each kind walked by the CPU emulation")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mesh_cast.py measures on an MI355X: no GPU is visible")
    from nerfactor_amd import build
    build.build()
    from nerfactor_amd import ops
    from nerfactor_amd.mesh import PerspCam, TriMesh
    from tests import mesh_cases as mc
    dev = torch.device('cuda', 0)
    sv, sf = displaced_icosphere(args.subdiv, 300., mc.CENTRE)
    gv, gf = mc.ground(nq=64)
    mesh = TriMesh(np.vstack((sv, gv)), np.vstack((sf, gf + sv.shape[0])))
    v32 = mesh.vertices.astype(np.float32)
    t0 = time.perf_counter()
    host = ops.mesh_bvh_build(v32, mesh.faces, 4)
    build_ms = (time.perf_counter() - t0) * 1e3
    blob, header = torch.from_numpy(host).to(dev), host[:32].copy()
    result = {'triangles': int(mesh.faces.shape[0]), 'nodes': mc.parse_blob(host)['n_nodes'], 'blob_bytes': int(host.size), 'max_leaf': 4,
              'bvh_build_ms': build_ms, 'device': torch.cuda.get_device_name(0)}

    cam = PerspCam(f_pix=256 / 2 / np.tan(np.radians(20.)), im_res=(256, 320), loc=mc.CAM, lookat=mc.CENTRE, up=(0, 0, -1))
    d = cam.gen_rays().reshape(-1, 3).astype(np.float32)
    o = np.tile(mc.CAM, (d.shape[0], 1)).astype(np.float32)
    od, dd = torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev)
    result['cast'] = timed(lambda: ops.mesh_cast(blob, header, od, dd), args.reps)
    result['cast']['rays'] = int(d.shape[0])
    result['cast']['rays_per_s'] = d.shape[0] / (result['cast']['ms_per_launch'] * 1e-3)
    t, tri = ops.mesh_cast(blob, header, od, dd)
    hit = tri >= 0
    result['cast']['hit_fraction'] = float(hit.float().mean())

    xyz = torch.where(hit[:, None], od + t[:, None] * dd, torch.zeros_like(od))
    normal = torch.zeros_like(od)
    normal[:, 1] = 1
    normal[hit] = torch.as_tensor(mesh.face_normals.astype(np.float32), device=dev)[tri[hit].long()]
    alpha = hit.float()
    lxyz = torch.as_tensor(mc.light_xyz(16), device=dev)
    out = torch.empty((d.shape[0], lxyz.shape[0]), device=dev)
    result['lvis'] = timed(lambda: ops.mesh_lvis(blob, header, xyz, normal, alpha, lxyz, mc.LVIS_EPS, out=out), args.reps)
    ldir = torch.nn.functional.normalize(lxyz[None] - xyz[:, None], dim=2)
    walked = ((normal[:, None] * ldir).sum(2) > 0) & hit[:, None]
    result['lvis'].update(rows=int(d.shape[0]), lights=int(lxyz.shape[0]), pairs=int(walked.numel()), shadow_rays=int(walked.sum()),
                          visible_fraction_of_shadow_rays=float((out[walked] > 0).float().mean()))
    result['lvis']['shadow_rays_per_s'] = result['lvis']['shadow_rays'] / (result['lvis']['ms_per_launch'] * 1e-3)
    result['lvis']['pairs_per_s'] = result['lvis']['pairs'] / (result['lvis']['ms_per_launch'] * 1e-3)

    # what a ray costs: the CPU emulation of the same walk on a sample
    rng = np.random.RandomState(0)
    pick = rng.choice(d.shape[0], args.sample, replace=False)
    et, etri, visited, tested = mc.emu_cast_tree(host, o[pick], d[pick])
    result['cast'].update(sample=int(args.sample), nodes_per_ray=float(visited.mean()), triangles_per_ray=float(tested.mean()),
                          sample_equals_gpu=bool(np.array_equal(etri, tri.cpu().numpy()[pick])
                                                 and np.array_equal(et.view(np.int32), t.cpu().numpy()[pick].view(np.int32))))
    rows, lights = np.nonzero(walked.cpu().numpy())
    sel = rng.choice(rows.size, min(args.sample, rows.size), replace=False)
    so, sd = mc.shadow_rays32(xyz.cpu().numpy()[rows[sel]], lxyz.cpu().numpy(), mc.LVIS_EPS)
    k = np.arange(sel.size)
    ehit, visited, tested = mc.emu_cast_tree(host, so[k, lights[sel]], sd[k, lights[sel]], any_hit=True)
    got = out.cpu().numpy()[rows[sel], lights[sel]]
    nrm, sdir = normal.cpu().numpy()[rows[sel]], sd[k, lights[sel]]
    front = (nrm[:, 0] * sdir[:, 0] + nrm[:, 1] * sdir[:, 1]) + nrm[:, 2] * sdir[:, 2] > 0      # the kernel's own fp32 cosine
    result['lvis'].update(sample=int(sel.size), nodes_per_ray=float(visited.mean()), triangles_per_ray=float(tested.mean()),
                          sample_equals_gpu=bool(np.array_equal(front & ~ehit, got > 0)))
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as h:
            h.write(line + '\n')


if __name__ == '__main__':
    main()
