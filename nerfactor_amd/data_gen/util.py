"""From posed photographs to the directory that `dataset = nerf` reads: the pose normalisation of the original NeRF code and
the writer of the reference's data_gen/util.py (gen_data, recenter_poses, spherify_poses, poses_avg), restated.

    <outroot>/transforms_{train,val,test}.json     camera_angle_x and one {file_path, rotation, transform_matrix} per frame
    <outroot>/{train,val}_###/                     rgba.png, metadata.json
    <outroot>/test_###/                            nn.png (the nearest input view's image), metadata.json: the 120 poses of a
                                                   circle around the scene at the cameras' mean height

metadata.json: cam_angle_x, cam_transform_mat (16 comma-separated numbers, camera to world), imh, imw, original_path, envmap,
envmap_inten, scene, spp.  Poses are [N, 3, 5]: camera-to-world [R | t] and a last column (H, W, focal length).

Number formats follow the reference, because the written matrices are compared with its own to 1e-5: the poses arrive as
float32, recentring gives float32 again, everything after it is float64."""
import json
import os
from os.path import join

import numpy as np

N_TEST_POSES = 120


def _unit(v):
    return v / np.linalg.norm(v)


def _frame(z, up, pos):
    """[3, 4] camera-to-world with the z axis along z and the y axis as close to up as an orthonormal frame allows."""
    z = _unit(z)
    x = _unit(np.cross(up, z))
    return np.stack([x, _unit(np.cross(z, x)), z, pos], 1)


def _homogeneous(p):
    """[N, 3, 4] -> [N, 4, 4]."""
    bottom = np.broadcast_to(np.array([0, 0, 0, 1.]), (p.shape[0], 1, 4))
    return np.concatenate((p, bottom), 1)


def poses_avg(poses):
    """[3, 5]: the mean position, the summed viewing and up directions made a frame, and the first pose's (H, W, f)."""
    c2w = _frame(poses[:, :3, 2].sum(0), poses[:, :3, 1].sum(0), poses[:, :3, 3].mean(0))
    return np.concatenate([c2w, poses[0, :3, -1:]], 1)


def recenter_poses(poses):
    """The poses in the frame of their average; dtype and last column kept."""
    out = poses.copy()
    avg = _homogeneous(poses_avg(poses)[None, :3, :4])[0]
    out[:, :3, :4] = (np.linalg.inv(avg) @ _homogeneous(poses[:, :3, :4]))[:, :3, :4]
    return out


def spherify_poses(poses, n_test=N_TEST_POSES):
    """(poses [N, 3, 5], test poses [n_test, 3, 5]): the poses moved so that the point closest to all optical axes is the
    origin and the mean camera direction from it is +z, scaled to a root-mean-square distance of 1; the test poses on the
    circle of that radius at the cameras' mean height, looking outwards along their position (the camera's z axis), -z up."""
    d = poses[:, :3, 2:3]
    o = poses[:, :3, 3:4]
    # least squares: the point p minimising sum |(I - d d^T)(p - o)|^2
    a = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    b = -a @ o
    centre = np.squeeze(-np.linalg.inv((np.transpose(a, [0, 2, 1]) @ a).mean(0)) @ b.mean(0))
    z = _unit((poses[:, :3, 3] - centre).mean(0))
    x = _unit(np.cross([.1, .2, .3], z))
    y = _unit(np.cross(z, x))
    c2w = np.stack([x, y, z, centre], 1)
    moved = np.linalg.inv(_homogeneous(c2w[None])) @ _homogeneous(poses[:, :3, :4])
    rad = np.sqrt(np.mean(np.sum(np.square(moved[:, :3, 3]), -1)))
    sc = 1. / rad
    moved[:, :3, 3] *= sc
    rad *= sc
    zh = np.mean(moved[:, :3, 3], 0)[2]
    circle = np.sqrt(rad ** 2 - zh ** 2)
    test = []
    for th in np.linspace(0., 2. * np.pi, n_test):
        origin = np.array([circle * np.cos(th), circle * np.sin(th), zh])
        v2 = _unit(origin)
        v0 = _unit(np.cross(v2, np.array([0, 0, -1.])))
        v1 = _unit(np.cross(v2, v0))
        test.append(np.stack([v0, v1, v2, origin], 1))
    test = np.stack(test, 0)
    hwf = poses[0, :3, -1:]
    test = np.concatenate([test, np.broadcast_to(hwf, test[:, :3, -1:].shape)], -1)
    moved = np.concatenate([moved[:, :3, :4], np.broadcast_to(hwf, moved[:, :3, -1:].shape)], -1)
    return moved, test


def vali_indices(n_imgs, n_vali):
    """The reference's split, quirk included: every (n_imgs // n_vali)-th view, the last view never: 7 views and n_vali = 2
    give (0, 3), but 11 views and n_vali = 3 give the four views (0, 3, 6, 9)."""
    return np.arange(n_imgs)[:-1:(n_imgs // n_vali)]


def quantize_uint8(arr_0to1):
    """The reference writer's quantisation: clipped to [0, 1], times 255 in the array's own float type, truncated."""
    return (np.clip(arr_0to1, 0, 1) * 255).astype(np.uint8)


def _write_png(img, path):
    from PIL import Image
    if img.dtype != np.uint8:
        img = quantize_uint8(img)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img).save(path)


def _write_json(obj, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as h:
        json.dump(obj, h, indent=4, sort_keys=True)


def _c2w44(pose):
    return np.vstack((pose[:3, :4], np.array([0, 0, 0, 1]).reshape(1, 4)))


def gen_data(poses, imgs, img_paths, n_vali, outroot):
    """poses float32 [N, 3, 5]; imgs [N, H, W, 4], uint8 (written as they are) or float in [0, 1] (quantised by truncation);
    img_paths: the N source paths for `original_path`.  Writes the directory of the module's docstring and returns
    {'ind_train', 'ind_vali', 'nn': nearest input view of every test pose, 'cam_angle_x'}."""
    poses, test_poses = spherify_poses(recenter_poses(poses))      # cameras on a unit sphere
    n_imgs = imgs.shape[0]
    ind_vali = vali_indices(n_imgs, n_vali)
    ind_train = np.array([i for i in range(n_imgs) if i not in ind_vali])
    imh, imw = int(imgs.shape[1]), int(imgs.shape[2])
    cam_angle_x = float(np.arctan2(imw / 2, poses[0, -1, -1]) * 2)

    def view_meta(c2w, original_path):
        return {'cam_angle_x': cam_angle_x, 'cam_transform_mat': ','.join(str(x) for x in c2w.ravel()), 'envmap': '',
                'envmap_inten': 0, 'imh': imh, 'imw': imw, 'scene': '', 'spp': 0, 'original_path': original_path}

    for mode, ind in (('train', ind_train), ('val', ind_vali)):
        frames = []
        for vi, i in enumerate(ind):
            folder = '%s_%03d' % (mode, vi)
            _write_png(imgs[i], join(outroot, folder, 'rgba.png'))
            c2w = _c2w44(poses[i])
            frames.append({'file_path': './%s/rgba' % folder, 'rotation': 0, 'transform_matrix': c2w.tolist()})
            _write_json(view_meta(c2w, img_paths[i]), join(outroot, folder, 'metadata.json'))
        _write_json({'camera_angle_x': cam_angle_x, 'frames': frames}, join(outroot, 'transforms_%s.json' % mode))

    frames, nn = [], []
    for i in range(test_poses.shape[0]):
        folder = 'test_%03d' % i
        c2w = _c2w44(test_poses[i])
        frames.append({'file_path': '', 'rotation': 0, 'transform_matrix': c2w.tolist()})
        nn.append(int(np.argmin(np.linalg.norm(test_poses[i][:, 3] - poses[:, :, 3], axis=1))))
        _write_png(imgs[nn[-1]], join(outroot, folder, 'nn.png'))
        _write_json(view_meta(c2w, ''), join(outroot, folder, 'metadata.json'))
    _write_json({'camera_angle_x': cam_angle_x, 'frames': frames}, join(outroot, 'transforms_test.json'))
    return {'ind_train': ind_train, 'ind_vali': ind_vali, 'nn': nn, 'cam_angle_x': cam_angle_x}


# ------------------------------------------------------------------------------------------------ reading and resizing
def read_image(path):
    """An image file as a uint8 / uint16 array [H, W(, C)], turned as its EXIF orientation says."""
    from PIL import Image, ImageOps
    with Image.open(path) as img:
        img.load()
        img = ImageOps.exif_transpose(img)
        return np.array(img)


def sortglob(directory, ext, ignore_case=False):
    """The files of `directory` with the extension `ext`, sorted by path."""
    want = '.' + ext.lower() if ignore_case else '.' + ext
    names = [n for n in os.listdir(directory) if (os.path.splitext(n)[1].lower() if ignore_case else os.path.splitext(n)[1]) == want]
    return sorted(join(directory, n) for n in names)


def load_and_resize(img_paths, h, device):
    """The images at height h with an all-one alpha appended to three channels: uint8 [N, h, w, 4] from the kernel
    (device = 'cuda': nfx_resize_antialias writes the PNG's bytes itself) or float32 from the host filter (device = 'cpu').
    -> (imgs, factor = original height / h).  Images of another size than the first are refused."""
    if device not in ('cuda', 'cpu'):
        raise ValueError("device must be 'cuda' or 'cpu', got %r" % (device,))
    raw = []
    for path in img_paths:
        arr = read_image(path)
        if arr.dtype not in (np.uint8, np.uint16):
            raise TypeError("%s: %s pixels (uint8 or uint16)" % (path, arr.dtype))
        if arr.ndim == 2:
            arr = arr[:, :, None]
        if raw and arr.shape != raw[0].shape:
            raise ValueError("Images are of varying sizes: %s is %s, %s is %s" % (img_paths[0], raw[0].shape, path, arr.shape))
        raw.append(arr)
    factor = float(raw[0].shape[0]) / h
    if device == 'cuda':
        import torch

        from .. import ops
        out = []
        for arr in raw:                         # one image at a time on the device: a 12 MP photograph is 36 MB
            x = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
            out.append(ops.resize_antialias(x, new_h=h, out_uint8=True).cpu().numpy())
        imgs = np.stack(out, 0)
        one = 255
    else:
        from ..nerfactor.util.light import resize_antialias
        imgs = np.stack([resize_antialias(arr.astype(np.float32) / np.float32(np.iinfo(arr.dtype).max), new_h=h) for arr in raw], 0)
        one = 1
    if imgs.shape[3] == 3:
        imgs = np.concatenate((imgs, np.full_like(imgs[..., :1], one)), -1)
    return imgs, factor
