"""brdf.renderer — light-sphere geometry (reference: brdf/renderer.py:184-219).  Host-side NumPy
(float64), evaluated once per model; the per-ray work happens in libnfx."""
import numpy as np


def gen_light_xyz(envmap_h, envmap_w, envmap_radius=1e2):
    """Positions of the pixels of a latitude-longitude environment map on a sphere of radius
    `envmap_radius`, plus the solid angle each pixel subtends (sums to 4*pi).

    Latitudes run from just below +pi/2 (top row) to just above -pi/2, longitudes from just below
    +pi (first column) to just above -pi: the polar / seam samples are excluded by shrinking the
    grid by one step of an (h+2) x (w+2) grid."""
    lat_step = np.pi / (envmap_h + 2)
    lng_step = 2 * np.pi / (envmap_w + 2)
    lat = np.linspace(np.pi / 2 - lat_step, -np.pi / 2 + lat_step, envmap_h)
    lng = np.linspace(np.pi - lng_step, -np.pi + lng_step, envmap_w)
    lng, lat = np.meshgrid(lng, lat)
    xyz = envmap_radius * np.stack(
        (np.cos(lat) * np.cos(lng), np.cos(lat) * np.sin(lng), np.sin(lat)), axis=-1)
    sin_colat = np.sin(np.pi / 2 - lat)
    areas = 4 * np.pi * sin_colat / np.sum(sin_colat)
    if np.any(areas == 0):
        raise ValueError("There shouldn't be light pixel that doesn't contribute")
    return xyz, areas


def load_light(envmap, envmap_inten=1., envmap_h=None):
    """The light probe a sphere is rendered under, [h, 2h, 3] float64 (reference: brdf/renderer.py:222-249).

    'white' and 'point' are the reference's arrays exactly ('point': a 4 x 4 block of ones addressed from the END of
    both axes, as the reference's negative indices do).  Anything else is a path read by util/light.read_probe and, when
    `envmap_h` is given, resized by util/light.resize_antialias.  The reference resizes with OpenCV; a file probe of
    another size is therefore NOT pinned to the reference's pixels."""
    if envmap == 'white':
        h = 16 if envmap_h is None else int(envmap_h)
        light = np.ones((h, 2 * h, 3), dtype=float)
    elif envmap == 'point':
        h = 16 if envmap_h is None else int(envmap_h)
        light = np.zeros((h, 2 * h, 3), dtype=float)
        i = -light.shape[0] // 4
        j = -int(light.shape[1] * 7 / 8)
        d = 2
        light[(i - d):(i + d), (j - d):(j + d), :] = 1
    else:
        from ..nerfactor.util import light as lightutil
        light = np.asarray(lightutil.read_probe(envmap), dtype=float)
        if envmap_h is not None and light.shape[0] != int(envmap_h):
            light = np.asarray(lightutil.resize_antialias(light, new_h=int(envmap_h)), dtype=float)
    return envmap_inten * light


def gen_world2local(normal):
    """[..., 3, 3] rotations whose rows are tangent, binormal and normal (xiuminglib geometry/normal.py:45-78)."""
    z = np.array((0, 0, 1), dtype=float)
    t = np.cross(normal, z)
    if (t == 0).all(axis=-1).any():
        raise ValueError("Found (0, 0, 0) tangents: a normal is colinear with (0, 0, 1), or (0, 0, 0)")
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    b = np.cross(normal, t)
    return np.stack((t, b, normal), axis=normal.ndim - 1)


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class SphereRenderer:
    """A sphere of a given BRDF under a light probe, direct illumination only, the probe sampled as a light stage
    (reference: brdf/renderer.py:23-181, float64 NumPy).  The sphere (radius 0.4) sits at the origin, the camera at
    (0, 0, -10) looks at it with +Y up; `ims` x `ims` pixels of sps x sps samples each, spp = sps^2.

    Attributes as in the reference, on the [ims sps, ims sps] sample grid: xyz, is_fg, normal, ldir / vdir (local frame),
    lcos, lvis, lcontrib = lvis light lcos area, lxyz, lareas, cam_loc."""

    def __init__(self, envmap, envmap_inten=1., envmap_h=None, ims=128, spp=1):
        self.ims = int(ims)
        self.sps = self._spp2sps(spp)
        self.cam_loc, self.xyz, self.is_fg = self._gen_scene()
        self.normal = _normalize(self.xyz + 1e-12)   # the eps keeps (0, 0, 0) and (0, 0, +/-1) away
        self.world2local = gen_world2local(self.normal)
        self.light = load_light(envmap, envmap_inten=envmap_inten, envmap_h=envmap_h)
        self.lxyz, self.lareas = gen_light_xyz(*self.light.shape[:2])
        self.ldir = self.gen_light_dir(local=True)
        self.vdir = self.gen_view_dir(local=True)
        self.lcos = self.ldir[..., 2]             # local frame: the normal is +Z
        self.lvis = np.logical_and(self.is_fg[:, :, None], self.lcos > 0).astype(float)
        self.lcontrib = self.calc_light_contrib(self.light)

    @staticmethod
    def _spp2sps(spp):
        sps = np.sqrt(spp)
        if sps != int(sps):
            raise ValueError("`spp` must be a square integer")
        return int(sps)

    def _gen_scene(self, sphere_radius=0.4, cam_dist=10.):
        res = self.ims * self.sps
        sample_w = 1 / (self.sps + 1)
        x = np.linspace(sample_w, self.ims - sample_w, res, endpoint=True)
        x /= self.ims
        xx, yy = np.meshgrid(x, x)
        dist = np.linalg.norm(np.dstack((xx, yy)) - 0.5, axis=2)
        is_fg = dist <= sphere_radius
        height = np.sqrt(np.where(is_fg, sphere_radius ** 2 - np.square(dist), 0))
        depth = cam_dist - height
        # perspective back-projection (xiuminglib camera.py:451-502): a 24 mm high sensor on `res` pixels, the focal
        # length chosen so that the sphere's radius projects onto 0.4 of the image — of a plane through the ORIGIN,
        # which is why the back-projected radii are close to, but not exactly, 0.4
        mm_per_pix = 24 / res
        sensor_h_active = res * mm_per_pix
        f_mm = cam_dist * (sensor_h_active / 2 / 0.5 * sphere_radius) / sphere_radius
        f_pix = float(f_mm) / mm_per_pix
        v_is, h_is = np.where(is_fg)
        hs = (h_is + 0.5) / res * res
        vs = (v_is + 0.5) / res * res
        zs = depth[is_fg]
        xs = zs * (hs - res / 2) / f_pix
        ys = zs * (vs - res / 2) / f_pix
        # camera (x right, y down, z forward) to object space: looking along +Z from -Z with +Y up flips x and y
        xyz = np.zeros((res, res, 3), dtype=float)
        xyz[is_fg] = np.stack((-xs, -ys, zs - cam_dist), axis=1)
        return np.array((0., 0., -cam_dist)), xyz, is_fg

    def gen_view_dir(self, local=False):
        vdir = self.cam_loc[None, None, :] - self.xyz
        if local:
            vdir = np.einsum('ijkl,ijl->ijk', self.world2local, vdir)
        return _normalize(vdir)

    def gen_light_dir(self, local=False):
        ldir = self.lxyz.reshape(-1, 3)[None, None, :, :] - self.xyz[:, :, None, :]
        if local:
            ldir = np.einsum('ijkl,ijnl->ijnk', self.world2local, ldir)
        return _normalize(ldir)

    def calc_light_contrib(self, light):
        light = np.reshape(light, (-1, 3))
        return self.lvis[:, :, :, None] * light[None, None] * self.lcos[:, :, :, None] * self.lareas.reshape(-1)[None, None, :, None]

    def render(self, brdf, white_bg=True):
        """brdf [H, W, L, 3] (or [H, W, L, 1]) -> [ims, ims, 3]: sum over lights, background, mean over a pixel's samples."""
        render = np.sum(brdf * self.lcontrib, axis=2)
        render[~self.is_fg] = 1. if white_bg else 0.
        s = self.sps
        return render.reshape(self.ims, s, self.ims, s, 3).sum(axis=(1, 3)) / (s ** 2)

    def device_scene(self, device):
        """What the fused sphere kernels (nfx_brdf_sphere_fwd, nfx_merl_sphere_fwd) take of this scene, as float32 tensors on
        `device`, built once per device: the foreground samples' xyz and normal, lxyz, lweight = light * area, the
        foreground mask 'fg' over the flattened sample grid, and 'renderer' (this object)."""
        import torch
        scenes = self.__dict__.setdefault('_device_scenes', {})
        key = str(device)
        if key not in scenes:
            dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device).contiguous()
            fg = self.is_fg.reshape(-1)
            lweight = self.light.reshape(-1, 3) * self.lareas.reshape(-1, 1)
            scenes[key] = {
                'renderer': self, 'fg': torch.as_tensor(fg, device=device), 'xyz': dev(self.xyz.reshape(-1, 3)[fg]),
                'normal': dev(self.normal.reshape(-1, 3)[fg]), 'lxyz': dev(self.lxyz.reshape(-1, 3)), 'lweight': dev(lweight)}
        return scenes[key]

    def assemble(self, fg_rgb, white_bg=True):
        """fg_rgb [B, n_fg, 3] device tensor of the foreground samples -> [B, ims, ims, 3]: background, mean over a pixel's samples."""
        import torch
        res = self.ims * self.sps
        fg = self.device_scene(fg_rgb.device)['fg']
        img = torch.full((fg_rgb.shape[0], res * res, 3), 1. if white_bg else 0., device=fg_rgb.device)
        img[:, fg] = fg_rgb
        return img.reshape(fg_rgb.shape[0], self.ims, self.sps, self.ims, self.sps, 3).sum(dim=(2, 4)) / float(self.sps ** 2)
