"""brdf.merl — measured MERL BRDFs (reference: brdf/merl/merl.py, third_party/nielsen2015on/{coordinateFunctions,
merlFunctions}.py): the coordinates of the 180 x 90 x 90 table, reading and writing `.binary` files, and class MERL with
the reference's surface.  Everything about the table itself is host-side float64 NumPy; the two things the reference does
per query — the nearest-neighbour lookup (a SciPy k-d tree there) and the render of a material on a sphere — run on the GPU
(ops.merl_query, ops.merl_sphere_fwd) and have no CPU path."""
import os

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


MERL_SCALE = (1.00 / 1500, 1.15 / 1500, 1.66 / 1500)   # the colour scaling of the files (merlFunctions.py:20)
LUM_WEIGHTS = (0.2126, 0.7152, 0.0722)                 # xiuminglib.img.rgb2lum


def rgb2lum(rgb):
    """[..., 3] -> [...] relative luminance, the statement of xiuminglib.img.rgb2lum."""
    rgb = np.asarray(rgb)
    return LUM_WEIGHTS[0] * rgb[..., 0] + LUM_WEIGHTS[1] * rgb[..., 1] + LUM_WEIGHTS[2] * rgb[..., 2]


def read_merl_binary(path):
    """A MERL `.binary` file -> (phi_d, theta_h, theta_d, 3) float64 (merlFunctions.py:readMERLBRDF): three int32 dims
    (theta_h, theta_d, phi_d on disk), then float64 values in Fortran order; colour-scaled, negatives set to -1.  A file whose
    length does not match its dims raises ValueError."""
    with open(path, 'rb') as h:
        dims = np.fromfile(h, np.int32, 3)
        if dims.size != 3 or (dims <= 0).any():
            raise ValueError("%s: not a MERL .binary file (dims %s)" % (path, dims.tolist()))
        vals = np.fromfile(h, np.float64, -1)
    want = int(np.prod(dims.astype(np.int64))) * 3
    size = os.path.getsize(path)
    if vals.size != want or size != 12 + 8 * want:
        raise ValueError("%s: dims %s need %d values (%d bytes) but the file holds %d values (%d bytes)"
                         % (path, dims.tolist(), want, 12 + 8 * want, vals.size, size))
    cube = np.swapaxes(np.reshape(vals, (dims[2], dims[1], dims[0], 3), 'F'), 1, 2)
    cube *= MERL_SCALE
    cube[cube < 0] = -1
    return cube


def write_merl_binary(path, cube, tone_map=True):
    """The inverse of read_merl_binary (merlFunctions.py:saveMERLBRDF): cube (phi_d, theta_h, theta_d, 3) -> `.binary`;
    tone_map divides by the colour scaling that the reader multiplies with."""
    cube = np.array(cube, dtype=np.float64)
    if cube.ndim != 4 or cube.shape[3] != 3:
        raise ValueError("a (phi_d, theta_h, theta_d, 3) cube is expected, got shape %s" % (cube.shape,))
    if tone_map:
        cube /= MERL_SCALE
    vec = np.reshape(np.swapaxes(cube, 1, 2), (-1), 'F')
    with open(path, 'wb') as h:
        np.array([cube.shape[2], cube.shape[1], cube.shape[0]]).astype(np.int32).tofile(h)
        vec.astype(np.float64).tofile(h)


class MERL:
    """A measured BRDF (reference: brdf/merl/merl.py:MERL).  MERL() is a Lambertian cube of ones."""

    def __init__(self, path=None):
        if path is None:
            cube_rgb = np.ones(BRDFSHAPE + (3,), dtype=float)
            name = 'lambertian'
        else:
            cube_rgb = read_merl_binary(path)
            if cube_rgb.shape != BRDFSHAPE + (3,):
                raise ValueError("%s: a %s table is expected, got %s" % (path, BRDFSHAPE, cube_rgb.shape[:3]))
            name = self.parse_name(path)
        self._cube_rgb = cube_rgb
        self.name = name
        self.flat_rusink = merl_to_rusink(np.reshape(np.indices(BRDFSHAPE), (3, -1)).T)
        self.cube_rusink = np.reshape(self.flat_rusink, BRDFSHAPE + (3,))
        self._tables = {}

    @property
    def cube_rgb(self):
        return self._cube_rgb

    @cube_rgb.setter
    def cube_rgb(self, x):
        correct_shape = self._cube_rgb.shape
        assert x.shape == correct_shape, "Reflectance must be stored in a cube of shape %s" % (correct_shape,)
        self._cube_rgb = x
        self._tables = {}

    @property
    def flat_rgb(self):
        return np.reshape(self.cube_rgb, (-1, 3))

    @property
    def valid(self):
        """[180 * 90 * 90] bool: all three channels > 0."""
        return (self.flat_rgb > 0).all(axis=1)

    @property
    def tbl(self):
        """[n_valid, 6]: (phi_d, theta_h, theta_d, r, g, b) of the valid entries, in cube order."""
        return np.hstack((self.flat_rusink, self.flat_rgb))[self.valid, :]

    @staticmethod
    def parse_name(path):
        return os.path.basename(path)[:-len('.binary')]

    def get_characterstic_slice(self):
        """[90, 90, 3]: the characteristic slice (phi_d = 90 degrees), theta_d up and theta_h to the right."""
        return np.rot90(self.cube_rgb[self.cube_rgb.shape[0] // 2, :, :], axes=(0, 1))

    get_characteristic_slice = get_characterstic_slice

    def get_characterstic_slice_rusink(self):
        return np.rot90(self.cube_rusink[self.cube_rusink.shape[0] // 2, :, :, :], axes=(0, 1))

    get_characteristic_slice_rusink = get_characterstic_slice_rusink

    characteristic_slice_as_img = staticmethod(characteristic_slice_as_img)
    dir2rusink = staticmethod(dir2rusink)

    def packed_table(self, achromatic=False):
        """float32 [180 * 90 * 90, 4] host array: rgb (the luminance three times when achromatic) plus one pad float; every invalid
        entry is -1 in all four lanes.  A table without a valid entry raises."""
        rgb = self.flat_rgb
        if achromatic:
            rgb = np.tile(rgb2lum(rgb)[:, None], (1, 3))
        rgb32 = rgb.astype(np.float32)
        valid = self.valid & (rgb32 > 0).all(axis=1)      # (a reflectance below 1.4e-45 is no float32: the entry counts as a hole)
        if not valid.any():
            raise ValueError("MERL material %r has no valid entry (all three channels > 0): nothing can be looked up" % self.name)
        packed = np.full((rgb.shape[0], 4), -1, dtype=np.float32)
        packed[valid, :3] = rgb32[valid]
        packed[valid, 3] = 0
        return packed

    def device_table(self, device, achromatic=False):
        """packed_table on `device`, built once per (device, achromatic)."""
        import torch
        key = (str(torch.device(device)), bool(achromatic))
        if key not in self._tables:
            self._tables[key] = torch.as_tensor(self.packed_table(achromatic), device=device).contiguous()
        return self._tables[key]

    def query(self, qrusink, achromatic=False):
        """Nearest valid entry's rgb for Rusinkiewicz coordinates [N, 3]: a NumPy array in gives a NumPy array out, a CUDA
        tensor a CUDA tensor.  Runs on the GPU (nfx_merl_query); there is no CPU path."""
        import torch
        from .. import ops
        if isinstance(qrusink, torch.Tensor):
            return ops.merl_query(self.device_table(qrusink.device, achromatic), qrusink.float().reshape(-1, 3))
        if not torch.cuda.is_available():
            raise RuntimeError("MERL.query needs an MI355X: libnfx has no CPU path")
        from .. import dist as nfx_dist
        device = nfx_dist.local_device()
        q = torch.as_tensor(np.ascontiguousarray(np.reshape(qrusink, (-1, 3))), dtype=torch.float32, device=device)
        return ops.merl_query(self.device_table(device, achromatic), q).cpu().numpy()

    def render_sphere(self, renderer, achromatic=False, white_bg=True, device=None):
        """[ims, ims, 3] device tensor: this material on the sphere of `renderer` (brdf.renderer.SphereRenderer) in one fused launch
        (nfx_merl_sphere_fwd: angles, lookup, cosine weighting and the sum over lights in the kernel)."""
        import torch
        from .. import ops
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("MERL.render_sphere needs an MI355X: libnfx has no CPU path")
            from .. import dist as nfx_dist
            device = nfx_dist.local_device()
        scene = renderer.device_scene(device)
        fg_rgb = ops.merl_sphere_fwd(scene['xyz'], scene['normal'], renderer.cam_loc, self.device_table(device, achromatic),
                                     scene['lxyz'], scene['lweight'])
        return renderer.assemble(fg_rgb[None], white_bg=white_bg)[0]
