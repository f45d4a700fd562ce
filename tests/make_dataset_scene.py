"""The small capture of the make_dataset tests and of tests/golden/make_reference_real_golden.py: 7 cameras on a hemisphere
around the origin in LLFF's poses_bounds.npy, and 48 x 64 photographs of uniform-random uint8 noise.

Noise, not flat or smooth pictures: the reference's writer truncates v * 255, so a region whose exact value sits on an integer
level lands on either side of it by the last bit of float32, and two correct filters would differ by one level over whole
regions.  On noise that happens to about one value in 10^4.

The fixture keeps the JPEG files' bytes (key jpeg_<i>), so that a test decodes the very files the reference read; write()
puts them, or freshly encoded ones, on disk together with poses_bounds.npy, and helpers read a written dataset back."""
import glob
import io
import json
import os
from os.path import basename, dirname, join

import numpy as np

N_VIEWS, IM_H, IM_W, FOCAL = 7, 48, 64, 60.
OUT_H, N_VALI, BOUND_FACTOR = 12, 2, .75
GOLDEN = join(dirname(os.path.abspath(__file__)), 'golden', 'reference_real.npz')


def poses_bounds():
    """float64 [7, 17]: cameras at radius 4 on two rings of the upper hemisphere, looking at the origin, world z up.  LLFF's
    rotation columns are (down, right, backwards)."""
    rows = []
    for i in range(N_VIEWS):
        lng = 2. * np.pi * i / N_VIEWS + 0.1
        lat = np.deg2rad(25. + 20. * (i % 3))
        p = 4. * np.array([np.cos(lat) * np.cos(lng), np.cos(lat) * np.sin(lng), np.sin(lat)])
        back = p / np.linalg.norm(p)
        right = np.cross([0., 0., 1.], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        pose = np.stack([-up, right, back, p, [IM_H, IM_W, FOCAL]], 1)
        rows.append(np.concatenate([pose.ravel(), [2.5 + 0.1 * i, 6. + 0.2 * i]]))
    return np.array(rows)


def noise_images():
    rng = np.random.default_rng(20211)
    return rng.integers(0, 256, (N_VIEWS, IM_H, IM_W, 3), dtype=np.int64).astype(np.uint8)


def encode_jpegs():
    """The 7 files' bytes, encoded with PIL (quality 95)."""
    from PIL import Image
    out = []
    for img in noise_images():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format='JPEG', quality=95)
        out.append(buf.getvalue())
    return out


def write(scene_dir, jpegs=None, ext='jpg'):
    """<scene_dir>/poses_bounds.npy and images/img_<i>.<ext>; jpegs: the files' bytes (default: the fixture's)."""
    if jpegs is None:
        with np.load(GOLDEN) as z:
            jpegs = [z['jpeg_%d' % i].tobytes() for i in range(N_VIEWS)]
    os.makedirs(join(scene_dir, 'images'), exist_ok=True)
    np.save(join(scene_dir, 'poses_bounds.npy'), poses_bounds())
    for i, data in enumerate(jpegs):
        with open(join(scene_dir, 'images', 'img_%d.%s' % (i, ext)), 'wb') as h:
            h.write(data)
    return scene_dir


def read_dataset(outroot):
    """(jsons {path relative to outroot: parsed JSON}, pngs {relative path: array}) of a written dataset directory."""
    from PIL import Image
    jsons, pngs = {}, {}
    for path in sorted(glob.glob(join(outroot, '*.json')) + glob.glob(join(outroot, '*', '*.json'))):
        with open(path) as h:
            jsons[os.path.relpath(path, outroot)] = json.load(h)
    for path in sorted(glob.glob(join(outroot, '*', '*.png'))):
        pngs[os.path.relpath(path, outroot)] = np.array(Image.open(path))
    return jsons, pngs


def load_golden():
    """(jsons, pngs) as read_dataset gives them, from the fixture."""
    with np.load(GOLDEN) as z:
        jsons = json.loads(str(z['jsons']))
        names = json.loads(str(z['png_names']))
        pngs = {n: z['pngs'][i] for i, n in enumerate(names)}
    return jsons, pngs


def matrix_of(meta):
    return np.array([float(x) for x in meta['cam_transform_mat'].split(',')]).reshape(4, 4)


def compare_jsons(got, want):
    """Largest |difference| over every camera matrix and angle of the two directories; everything else must be equal
    (original_path by its file name)."""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    worst = 0.
    for name in want:
        g, w = got[name], want[name]
        assert sorted(g) == sorted(w), name
        if name.startswith('transforms_'):
            worst = max(worst, abs(g['camera_angle_x'] - w['camera_angle_x']))
            assert len(g['frames']) == len(w['frames']), name
            for fg, fw in zip(g['frames'], w['frames']):
                assert (fg['file_path'], fg['rotation']) == (fw['file_path'], fw['rotation']), name
                worst = max(worst, float(np.abs(np.array(fg['transform_matrix']) - np.array(fw['transform_matrix'])).max()))
            continue
        worst = max(worst, abs(g['cam_angle_x'] - w['cam_angle_x']), float(np.abs(matrix_of(g) - matrix_of(w)).max()))
        for k in w:
            if k == 'original_path':
                assert basename(g[k]) == basename(w[k]), (name, g[k], w[k])
            elif k not in ('cam_angle_x', 'cam_transform_mat'):
                assert g[k] == w[k], (name, k, g[k], w[k])
    return worst


def compare_pngs(got, want):
    """(largest |level difference|, fraction of values that differ) over every PNG of the two directories."""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    worst, differ, total = 0, 0, 0
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype == np.uint8, name
        d = np.abs(got[name].astype(np.int32) - want[name].astype(np.int32))
        worst, differ, total = max(worst, int(d.max())), differ + int((d != 0).sum()), total + d.size
    return worst, differ / total
