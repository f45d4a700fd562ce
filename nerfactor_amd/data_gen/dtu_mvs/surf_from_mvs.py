"""From a DTU scan (projection matrices, a surface mesh, images) to the directory that `dataset = mvs_shape` reads, with the
reference's flags and output layout (data_gen/dtu_mvs/surf_from_mvs.py):

    python -m nerfactor_amd.data_gen.dtu_mvs.surf_from_mvs --cam_dir <dir> --surf_dir <dir> --img_dir <dir>/scanN --outdir <mvs_root> \\
        [--h 256] [--light_h 16] [--n_vali 2] [--n_test 120] [--lvis_eps 0.1] [--lvis_radius 1e5] [--nolvis] [--debug] [--overwrite]
        [--keep_largest K] [--min_faces M]

    <outdir>/lights.npz                          lxyzs [h, 2h, 3] around the mesh centre with z flipped, lareas [h, 2h]
    <outdir>/{train,val}_###/                    metadata.json (id, imh, imw, cam_loc), rgba.png, alpha.png, xyz.{npy,png},
                                                 normal.{npy,png}, lvis.{npy,png}
    <outdir>/test_###/                           the same without rgba.png, plus nn.png (the nearest training view's image)

Cameras are `pos_???.txt` (3 x 4 projection matrices), images `*_3_*.png` (the most diffuse lighting), the mesh
<surf_dir>/<basename(surf_dir)><scan number, 3 digits>_l3_surf_11_trim_8.ply.  Every `n_imgs // n_vali`-th view but the last is a
validation view; the test cameras sweep latitude and longitude at 1.5 x the mean camera distance, looking at the mesh centre with
-z up, and reuse the LAST training camera's intrinsics — all as in the reference.

One deliberate difference: the reference ships with its gen_lvis calls commented out although its own dataset needs lvis.npy;
this driver writes it unless --nolvis is given.  The reference's lvis.mp4 and debug video are not written.

Camera rays and one shadow ray per (surface point, light) are cast on the GPU (mesh.RayMeshIntersector: nfx_mesh_cast,
nfx_mesh_lvis with the rays made in the kernel); the [pixels, lights] visibility of a view is the only large allocation.
--keep_largest K / --min_faces M (opt-in): the scan's connected components are labelled on the GPU (TriMesh.filter_components)
and only the K with the most triangles / those with at least M triangles are cast against; vertices are not welded first."""
import argparse
import glob
import json
import os
import shutil
import sys
import time
from os.path import basename, isdir, join

import numpy as np

from ...brdf.renderer import gen_light_xyz
from ...mesh import PerspCam, RayMeshIntersector, TriMesh, decompose_projection, filter_clause, sph2cart
from ...nerfactor.util.light import resize_antialias


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cam_dir', required=True, help="directory of pos_???.txt projection matrices")
    ap.add_argument('--surf_dir', required=True, help="directory of the surface meshes")
    ap.add_argument('--img_dir', required=True, help="directory of the scan's images, named scan<N>")
    ap.add_argument('--outdir', required=True, help="output directory (the mvs_root of the configs)")
    ap.add_argument('--h', type=int, default=256, help="output image height")
    ap.add_argument('--light_h', type=int, default=16, help="light probe height")
    ap.add_argument('--n_vali', type=int, default=2, help="number of validation views")
    ap.add_argument('--n_test', type=int, default=120, help="number of test views")
    ap.add_argument('--lvis_eps', type=float, default=1e-1, help="offset of a shadow ray's origin along its direction")
    ap.add_argument('--lvis_radius', type=float, default=1e5, help="radius of the light sphere")
    ap.add_argument('--lvis_chunk', type=int, default=1 << 16, help="pixels per light-visibility launch")
    ap.add_argument('--keep_largest', type=int, default=0, help="keep only the K connected components of the scan with the most triangles")
    ap.add_argument('--min_faces', type=int, default=0, help="keep only the connected components of the scan with at least M triangles")
    ap.add_argument('--nolvis', action='store_true', help="skip light visibility (what the reference does as shipped)")
    ap.add_argument('--debug', action='store_true', help="first four views only")
    ap.add_argument('--overwrite', action='store_true', help="whether to remove output folder if it already exists")
    return ap.parse_args(argv)


def _read_img(path):
    from PIL import Image
    arr = np.array(Image.open(path))
    if arr.ndim == 2:
        arr = np.dstack([arr] * 3)
    return arr.astype(np.float32) / np.iinfo(arr.dtype).max


def _write_png(arr_0to1, path):
    from PIL import Image
    Image.fromarray((np.clip(arr_0to1, 0, 1) * 255 + .5).astype(np.uint8)).save(path)


def mesh_path_of(surf_dir, img_dir):
    """<surf_dir>/<basename(surf_dir)><scan number>_l3_surf_11_trim_8.ply (surf_from_mvs.py:61-64)."""
    surf_dir, scene = surf_dir.rstrip('/'), basename(img_dir.rstrip('/'))
    return join(surf_dir, basename(surf_dir) + '%03d' % int(scene.lstrip('scan')) + '_l3_surf_11_trim_8.ply')


def vali_indices(n_imgs, n_vali):
    return np.arange(n_imgs)[:-1:(n_imgs // n_vali)]


def test_cam_path(cam_dist, n_test):
    """(lats, lngs) [n_test] of the test cameras (surf_from_mvs.py:167-171)."""
    lngs = np.linspace(-0.25 * np.pi, 0.5 * np.pi, n_test // 2)
    lngs = np.hstack((lngs, np.linspace(0.5 * np.pi, -0.25 * np.pi, n_test - len(lngs))))
    return np.linspace(-0.25 * np.pi, 0, n_test), lngs


def camera_from_projection(P, factor, im_hw):
    """The reference's camera of a projection matrix at the output size (surf_from_mvs.py:109-121): one focal length, the mean
    of K's two, scaled by the resize; the principal point at the image centre."""
    K, R, t = decompose_projection(P)
    K = K / K[2, 2]
    f = (K[0, 0] + K[1, 1]) / 2 / factor
    cam = PerspCam()
    cam.int_mat = np.array([[f, 0, im_hw[1] / 2], [0, f, im_hw[0] / 2], [0, 0, 1]])
    cam.ext_mat = np.hstack((R, t.reshape(3, 1)))
    return cam


def process_view(cam, mesh, inter, lxyz, args, outdir):
    """Casts the view and writes its buffers; returns (alpha, xyz, normal) [H, W(, 3)]."""
    import torch
    os.makedirs(outdir, exist_ok=True)
    ray_dirs = cam.gen_rays()
    h, w = ray_dirs.shape[:2]
    dirs = ray_dirs.reshape(-1, 3)
    origs = np.tile(cam.loc, (dirs.shape[0], 1))
    locs, ray_ind, tri_ind = inter.intersects_location(origs, dirs, multiple_hits=False)
    with open(join(outdir, 'metadata.json'), 'w') as fh:
        json.dump({'id': basename(outdir), 'imh': h, 'imw': w, 'cam_loc': np.asarray(cam.loc).tolist()}, fh, indent=4, sort_keys=True)
    alpha = np.zeros(h * w, dtype=np.float32)            # 0 background, 1 foreground
    alpha[ray_ind] = 1
    xyz = np.zeros((h * w, 3), dtype=np.float32)         # background (0, 0, 0)
    xyz[ray_ind] = locs
    normal = np.zeros((h * w, 3), dtype=np.float32)      # background (0, 1, 0)
    normal[:, 1] = 1
    normal[ray_ind] = mesh.face_normals[tri_ind]
    _write_png(alpha.reshape(h, w), join(outdir, 'alpha.png'))
    np.save(join(outdir, 'xyz.npy'), xyz.reshape(h, w, 3))
    span = float(xyz.max() - xyz.min())
    _write_png((xyz.reshape(h, w, 3) - xyz.min()) / (span if span > 0 else 1.), join(outdir, 'xyz.png'))
    np.save(join(outdir, 'normal.npy'), normal.reshape(h, w, 3))
    _write_png((normal.reshape(h, w, 3) + 1) / 2, join(outdir, 'normal.png'))
    if not args.nolvis:
        device = mesh.bvh(inter.max_leaf, inter.device)[0].device
        lvis = torch.empty((h * w, lxyz.shape[0]), dtype=torch.float32, device=device)
        for lo in range(0, h * w, args.lvis_chunk):
            hi = min(lo + args.lvis_chunk, h * w)
            inter.light_visibility(xyz[lo:hi], normal[lo:hi], alpha[lo:hi], lxyz, args.lvis_eps, out=lvis[lo:hi])
        lvis = lvis.cpu().numpy().reshape(h, w, -1)
        np.save(join(outdir, 'lvis.npy'), lvis)
        _write_png(lvis.mean(axis=2), join(outdir, 'lvis.png'))
    return alpha.reshape(h, w), xyz.reshape(h, w, 3), normal.reshape(h, w, 3)


def main(argv=None):
    args = parse_args(argv)
    if args.keep_largest < 0 or args.min_faces < 0:
        raise ValueError("surf_from_mvs: keep_largest = %d and min_faces = %d must not be negative" % (args.keep_largest, args.min_faces))
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("surf_from_mvs casts every ray on the GPU and needs an MI355X: libnfx has no CPU path")
    if args.overwrite and isdir(args.outdir):
        shutil.rmtree(args.outdir)
    os.makedirs(args.outdir, exist_ok=True)

    cam_paths = sorted(glob.glob(join(args.cam_dir, 'pos_???.txt')))
    img_paths = sorted(glob.glob(join(args.img_dir, '*_3_*.png')))       # the most diffuse lighting
    assert img_paths, "No image globbed"
    cam_paths = cam_paths[:len(img_paths)]                               # in case only the first 49 cameras have images
    if args.debug:
        img_paths, cam_paths = img_paths[:4], cam_paths[:4]
    n_imgs = len(img_paths)
    assert len(cam_paths) == n_imgs, "Mismatch between numbers of images (%d) and poses (%d)" % (n_imgs, len(cam_paths))
    ind_vali = vali_indices(n_imgs, args.n_vali)

    mesh = TriMesh.load(mesh_path_of(args.surf_dir, args.img_dir))
    if args.keep_largest or args.min_faces:      # before the BVH is built
        t0 = time.perf_counter()
        mesh = mesh.filter_components(args.keep_largest, args.min_faces)
        print("[surf_from_mvs] %s: %d vertices, %d triangles" % (filter_clause(mesh.filter_info, time.perf_counter() - t0),
                                                               mesh.vertices.shape[0], mesh.faces.shape[0]), flush=True)
    inter = RayMeshIntersector(mesh)

    # DTU scenes are roughly 1000x bigger than normalised NeRF scenes and not centred at the origin, and their z axis is flipped
    lxyzs, lareas = gen_light_xyz(args.light_h, 2 * args.light_h, envmap_radius=args.lvis_radius)
    mesh_center = np.mean(mesh.vertices, axis=0)
    lxyzs = lxyzs + mesh_center
    lxyzs[:, :, 2] = -lxyzs[:, :, 2]
    np.savez(join(args.outdir, 'lights.npz'), lxyzs=lxyzs, lareas=lareas)
    lxyz = lxyzs.reshape(-1, 3).astype(np.float32)

    imgs, cams = [], []
    factor = None
    train_i = vali_i = 0
    for i, (img_path, cam_path) in enumerate(zip(img_paths, cam_paths)):
        img = _read_img(img_path)
        if factor is None:
            factor = float(img.shape[0]) / args.h
        else:
            assert float(img.shape[0]) / args.h == factor, "Images are of varying sizes"
        img = resize_antialias(img, new_h=args.h)
        if img.shape[2] == 3:
            img = np.dstack((img, np.ones_like(img)[:, :, :1]))          # an all-one alpha
        imgs.append(img)
        cam = camera_from_projection(np.loadtxt(cam_path), factor, img.shape[:2])
        cams.append(cam)
        if i in ind_vali:
            view_name, vali_i = 'val_%03d' % vali_i, vali_i + 1
        else:
            view_name, train_i = 'train_%03d' % train_i, train_i + 1
        outdir = join(args.outdir, view_name)
        process_view(cam, mesh, inter, lxyz, args, outdir)
        _write_png(img, join(outdir, 'rgba.png'))
        print("[surf_from_mvs] %s" % view_name, flush=True)

    # ------ test views
    cam_locs = [x.loc for x in cams]
    cam_dist = 1.5 * np.mean([np.linalg.norm(x - mesh_center) for x in cam_locs])
    lats, lngs = test_cam_path(cam_dist, args.n_test)
    if args.debug:
        lats, lngs = lats[:4], lngs[:4]
    cam = cams[-1]                                                      # its intrinsics stay: the reference reuses the object
    for i, (lat, lng) in enumerate(zip(lats, lngs)):
        cam.loc = sph2cart((cam_dist, lat, lng)) + mesh_center
        cam.lookat = mesh_center
        cam.up = np.array((0., 0., -1.))
        outdir = join(args.outdir, 'test_%03d' % i)
        process_view(cam, mesh, inter, lxyz, args, outdir)
        nn = imgs[int(np.argmin([np.linalg.norm(cam.loc - x) for x in cam_locs]))]
        _write_png(nn, join(outdir, 'nn.png'))
        print("[surf_from_mvs] test_%03d" % i, flush=True)
    return args.outdir


if __name__ == '__main__':
    main(sys.argv[1:])
