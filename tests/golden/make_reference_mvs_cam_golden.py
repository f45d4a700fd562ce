"""Generates tests/golden/reference_mvs_cams.npz from the REFERENCE's own camera code.

    python tests/golden/make_reference_mvs_cam_golden.py        (build container only: needs the reference checkout)

third_party/xiuminglib's camera.PerspCam and geometry.sph.sph2cart are imported from the reference unmodified, the way
make_reference_merl_golden.py does (absl from tests/golden/tf_shim; OpenCV is not installed and not needed by these two, an
empty stand-in module satisfies the import).  Stored, all float64:
  ext_<k>_{K,Rt}, look_<k>_{f,hw,loc,lookat,up}    the inputs of two cameras set through int_mat / ext_mat (the way
                                                   data_gen/dtu_mvs/surf_from_mvs.py sets its training cameras) and of two set
                                                   through loc / lookat / up (its test cameras), 8 x 10 pixels
  <cam>_loc, <cam>_rays                            PerspCam.loc and PerspCam.gen_rays() [8, 10, 1, 3] of each
  test_cam_dist, test_center, test_locs            the driver's test-camera positions (surf_from_mvs.py:167-183) for n_test = 6
tests/test_cpu_mesh_cast.py holds nerfactor_amd.mesh.PerspCam / sph2cart and the driver's camera path to these."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('NERFACTOR_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(HERE, 'tf_shim'), REF, os.path.join(REF, 'nerfactor'), REPO]
sys.modules.setdefault('cv2', types.ModuleType('cv2'))

from third_party.xiuminglib import xiuminglib as xm  # noqa: E402


def _rot(axis, deg):
    axis = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    a = np.radians(deg)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * k.dot(k)


def main():
    out = {}
    ext = {'a': (_rot((1, 2, 3), 40.), np.array((30., -700., 1200.)), 12.5), 'b': (_rot((-2, 0.5, 1), 155.), np.array((-400., 90., 800.)), 9.)}
    for k, (R, t, f) in ext.items():
        K = np.array([[f, 0, 5.], [0, f, 4.], [0, 0, 1]])
        Rt = np.hstack((R, t.reshape(3, 1)))
        cam = xm.camera.PerspCam()
        cam.int_mat = K
        cam.ext_mat = Rt
        out['ext_%s_K' % k], out['ext_%s_Rt' % k] = K, Rt
        out['ext_%s_loc' % k], out['ext_%s_rays' % k] = np.array(cam.loc, dtype=float), cam.gen_rays()
    look = {'a': (11., (400., 200., -700.), (50., -30., 600.), (0., 0., -1.)), 'b': (7.25, (-900., 40., 100.), (10., 20., 630.), (0., 1., 0.))}
    for k, (f, loc, lookat, up) in look.items():
        cam = xm.camera.PerspCam(f_pix=f, im_res=(8, 10), loc=loc, lookat=lookat, up=up)
        out['look_%s_f' % k], out['look_%s_hw' % k] = np.float64(f), np.array((8, 10))
        out['look_%s_loc' % k], out['look_%s_lookat' % k], out['look_%s_up' % k] = (np.array(x, dtype=float) for x in (loc, lookat, up))
        out['look_%s_rays' % k] = cam.gen_rays()
    # the driver's test-camera path
    n_test, cam_dist, center = 6, 1.5 * 1432.1, np.array((50., -30., 600.))
    lngs = np.linspace(-0.25 * np.pi, 0.5 * np.pi, n_test // 2)
    lngs = np.hstack((lngs, np.linspace(0.5 * np.pi, -0.25 * np.pi, n_test - len(lngs))))
    lats = np.linspace(-0.25 * np.pi, 0, n_test)
    locs = []
    for lat, lng in zip(lats, lngs):
        cam_loc = xm.geometry.sph.sph2cart((cam_dist, lat, lng), convention='lat-lng')
        locs.append(cam_loc + center)
    out['test_cam_dist'], out['test_center'], out['test_locs'] = np.float64(cam_dist), center, np.array(locs)
    path = os.path.join(HERE, 'reference_mvs_cams.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes', {k: np.shape(v) for k, v in out.items()})
    assert os.path.getsize(path) <= 1 << 16


if __name__ == '__main__':
    main()
