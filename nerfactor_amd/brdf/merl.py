"""brdf.merl — the coordinates of the MERL table that the BRDF prior is looked at through (reference: brdf/merl/merl.py,
third_party/nielsen2015on/coordinateFunctions.py).  Host-side float64 NumPy.  Reading MERL `.binary` files is out of scope."""
import numpy as np

BRDFSHAPE = (180, 90, 90)   # (phi_d, theta_h, theta_d); theta_h is sampled non-linearly


def merl_to_rusink(ind):
    """MERL cube indices [..., 3] -> Rusinkiewicz angles (phi_d, theta_h, theta_d) in radians."""
    c = np.array(np.reshape(ind, (-1, 3)), dtype=float)
    c[:, 0] = c[:, 0] / (BRDFSHAPE[0] - 1) * np.pi
    c[:, 1] = np.square((c[:, 1] + 0.105) / BRDFSHAPE[1]) * (np.pi / 2)
    c[:, 2] = c[:, 2] / (BRDFSHAPE[2] - 1) * (np.pi / 2)
    return c


def characteristic_slice_rusink():
    """[90, 90, 3] Rusinkiewicz coordinates of the characteristic slice (phi_d index 90 of the cube), rotated so that
    theta_d runs up and theta_h to the right (merl.py:90-96)."""
    th, td = np.meshgrid(np.arange(BRDFSHAPE[1]), np.arange(BRDFSHAPE[2]), indexing='ij')
    ind = np.stack((np.full_like(th, BRDFSHAPE[0] // 2), th, td), axis=-1)
    rusink = merl_to_rusink(ind).reshape(BRDFSHAPE[1], BRDFSHAPE[2], 3)
    return np.rot90(rusink, axes=(0, 1))


def characteristic_slice_as_img(cslice, clip_percentile=80):
    """A slice of reflectances -> uint8 image: clipped at a percentile, scaled to [0, 1], gamma 2.2 (merl.py:98-104)."""
    maxv = np.percentile(cslice, clip_percentile)
    u8 = (np.clip(cslice, 0, maxv) / maxv * 255).astype(np.uint8)
    table = np.array([((x / 255) ** (1 / 2.2)) * 255 for x in np.arange(0, 256)]).astype(np.uint8)
    return table[u8]


def _rotate(vector, axis, angle):
    c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
    axis = np.reshape(np.asarray(axis, dtype=float), (-1, 3))
    return vector * c + axis * np.dot(vector, axis.T) * (1 - c) + np.cross(axis, vector) * s


def directions_to_rusink(a, b):
    """Two unit directions [N, 3] in the local frame -> (phi_d, theta_h, theta_d) [N, 3] (coordinateFunctions.py:117-129)."""
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    a, b = unit(np.reshape(a, (-1, 3))), unit(np.reshape(b, (-1, 3)))
    h = unit((a + b) / 2)
    theta_h = np.arccos(h[:, 2])
    phi_h = np.arctan2(h[:, 1], h[:, 0])
    diff = _rotate(_rotate(b, (0, 0, 1), -phi_h), (0, 1, 0), -theta_h)
    theta_d = np.arccos(diff[:, 2])
    phi_d = np.mod(np.arctan2(diff[:, 1], diff[:, 0]), np.pi)
    return np.column_stack((phi_d, theta_h, theta_d))


def dir2rusink(ldir, vdir):
    """ldir [H, W, L, 3], vdir [H, W, 3], local frames -> [H, W, L, 3]; the tooling's argument order (view, light) (merl.py:106-117)."""
    v = np.broadcast_to(vdir[:, :, None, :], ldir.shape)
    return directions_to_rusink(v.reshape(-1, 3), ldir.reshape(-1, 3)).reshape(ldir.shape)
