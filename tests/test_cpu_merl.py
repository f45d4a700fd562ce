"""brdf.merl.MERL on the host (no GPU): the `.binary` reader and writer, the table, the packed device table's layout, the
data set split of data_gen.merl.make_dataset, and the conditions that tests/test_gpu_merl.py rests on — all against
tests/golden/reference_merl.npz, which the reference's unmodified MERL / readMERLBRDF / saveMERLBRDF / make_dataset.main
produced for tests/merl_cases.synthetic_cube(0) (tests/golden/make_reference_merl_golden.py)."""
import os
from os.path import join

import numpy as np
import pytest

from nerfactor_amd.brdf import merl
from tests import merl_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(join(HERE, 'golden', 'reference_merl.npz'))
SPHERE = np.load(join(HERE, 'golden', 'reference_sphere.npz'))
STRIDE = 997


@pytest.fixture(scope='module')
def material(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('merl') / 'synth0.binary')
    merl.write_merl_binary(path, mc.synthetic_cube(0))
    return merl.MERL(path)


def test_reader_against_the_references_on_a_tiny_file(tmp_path):
    path = str(tmp_path / 'tiny.binary')
    with open(path, 'wb') as h:
        h.write(GOLD['tiny_bytes'].tobytes())
    cube = merl.read_merl_binary(path)
    assert cube.dtype == np.float64 and cube.shape == (3, 5, 4, 3)       # dims 5 x 4 x 3 on disk are (theta_h, theta_d, phi_d)
    assert np.array_equal(cube, GOLD['tiny_cube'])
    assert (cube == -1).sum() == 1
    # a file is not a table of the product's shape: the class refuses it, the reader does not
    with pytest.raises(ValueError, match='180'):
        merl.MERL(path)


def test_write_then_read_round_trip_bit_for_bit(tmp_path):
    """The writer divides by the colour scaling and the reader multiplies by it, each one IEEE operation per value: what comes
    back is ((cube / scale) * scale) bit for bit, -1 stays -1, and without tone mapping the file holds the cube's own bits in the
    reference's layout (int32 dims theta_h, theta_d, phi_d; float64 values in Fortran order over the swapped axes)."""
    cube = mc.synthetic_cube(3)
    path = str(tmp_path / 'm.binary')
    merl.write_merl_binary(path, cube)
    assert os.path.getsize(path) == 12 + 8 * cube.size
    back = merl.read_merl_binary(path)
    scale = np.array(merl.MERL_SCALE)
    want = (cube / scale) * scale
    want[want < 0] = -1
    assert back.dtype == np.float64 and np.array_equal(back, want)
    assert np.array_equal(back == -1, cube == -1) and np.allclose(back, cube, rtol=4.5e-16, atol=0)
    raw = str(tmp_path / 'raw.binary')
    merl.write_merl_binary(raw, cube, tone_map=False)
    assert np.array_equal(np.fromfile(raw, np.int32, 3), (90, 90, 180))
    vals = np.fromfile(raw, np.float64, offset=12)
    assert np.array_equal(np.swapaxes(np.reshape(vals, (180, 90, 90, 3), 'F'), 1, 2), cube)
    # a second trip through writer and reader changes nothing any more on values that are exact under the scaling
    exact = np.where(cube < 0, -1., 1.) * np.array((1.00, 1.15, 1.66)) / 1500
    merl.write_merl_binary(path, exact)
    once = merl.read_merl_binary(path)
    merl.write_merl_binary(path, once)
    assert np.array_equal(merl.read_merl_binary(path), once)


def test_a_truncated_file_raises_with_both_numbers(tmp_path):
    path = str(tmp_path / 'short.binary')
    merl.write_merl_binary(path, mc.synthetic_cube(1))
    whole = open(path, 'rb').read()
    for cut in (8, 12345, len(whole) - 12):
        with open(path, 'wb') as h:
            h.write(whole[:len(whole) - cut])
        with pytest.raises(ValueError) as e:
            merl.read_merl_binary(path)
        assert str(180 * 90 * 90 * 3) in str(e.value) and str((len(whole) - cut - 12) // 8) in str(e.value)
    with open(path, 'wb') as h:
        h.write(whole + b'\0' * 8)
    with pytest.raises(ValueError):
        merl.read_merl_binary(path)


def test_table_counts_split_and_luminance_against_the_reference(material):
    from nerfactor_amd.data_gen.merl import make_dataset
    assert material.name == 'synth0'
    tbl = material.tbl
    assert tbl.shape == (int(GOLD['tbl_n']), 6) and np.array_equal(tbl[::STRIDE], GOLD['tbl_rows'])
    assert (tbl[:, 3:] > 0).all()
    train_rusink, train_refl, vali_rusink, vali_refl = make_dataset.split_material(material, 0.01)
    assert train_rusink.shape == (int(GOLD['ds_train_n']), 3) and vali_rusink.shape == (int(GOLD['ds_vali_n']), 3)
    assert train_refl.shape == (train_rusink.shape[0], 1) and vali_refl.shape == (vali_rusink.shape[0], 1)
    for got, key in ((train_rusink, 'ds_train_rusink'), (train_refl, 'ds_train_refl'), (vali_rusink, 'ds_vali_rusink'),
                     (vali_refl, 'ds_vali_refl')):
        assert got.dtype == np.float32 and np.array_equal(got[::STRIDE], GOLD[key]), key
    # every 100th valid row is a validation row, the others train, in table order
    assert np.array_equal(vali_rusink, tbl[::100, :3].astype(np.float32))
    lum = 0.2126 * tbl[:, 3] + 0.7152 * tbl[:, 4] + 0.0722 * tbl[:, 5]
    assert np.array_equal(vali_refl[:, 0], lum[::100].astype(np.float32))


def test_test_coordinates_against_the_reference():
    from nerfactor_amd.brdf.renderer import SphereRenderer
    from nerfactor_amd.data_gen.merl import make_dataset
    r = SphereRenderer('point', envmap_inten=40., envmap_h=16, ims=16, spp=1)
    coords = make_dataset.test_coordinates(r)
    assert coords.dtype == np.float32 and coords.shape == (int(GOLD['ds_test_n']), 3)
    assert np.array_equal(coords[:8100], merl.MERL().get_characterstic_slice_rusink().reshape(-1, 3).astype(np.float32))
    assert np.abs(coords[::STRIDE] - GOLD['ds_test_rusink']).max() <= 2.4e-7      # one float32 ulp of pi


def test_the_lambertian_default():
    m = merl.MERL()
    assert m.name == 'lambertian' and m.cube_rgb.shape == (180, 90, 90, 3) and np.all(m.cube_rgb == 1.)
    assert m.flat_rgb.shape == (mc.N_CELLS, 3) and m.tbl.shape == (mc.N_CELLS, 6)
    assert m.cube_rusink.shape == (180, 90, 90, 3) and m.flat_rusink.shape == (mc.N_CELLS, 3)
    assert np.array_equal(m.flat_rusink, mc.grid_rusink(np.arange(mc.N_CELLS)))
    assert np.array_equal(m.get_characterstic_slice_rusink(), merl.characteristic_slice_rusink())
    assert m.get_characteristic_slice().shape == (90, 90, 3)
    assert merl.MERL.parse_name('/some/where/blue-metallic-paint.binary') == 'blue-metallic-paint'
    with pytest.raises(AssertionError):
        m.cube_rgb = np.ones((4, 4, 4, 3))
    m.cube_rgb = mc.synthetic_cube(2)
    assert m.tbl.shape[0] == int((mc.synthetic_cube(2) > 0).all(-1).sum())


def test_packed_table_layout_and_the_minus_one_convention(material):
    packed = material.packed_table()
    assert packed.dtype == np.float32 and packed.shape == (1458000, 4) and packed.flags['C_CONTIGUOUS']
    valid = (material.flat_rgb > 0).all(1)
    assert np.all(packed[~valid] == -1.) and np.array_equal(packed[valid, :3], material.flat_rgb[valid].astype(np.float32))
    assert np.all(packed[valid, :3] > 0)
    achro = material.packed_table(achromatic=True)
    lum = (0.2126 * material.flat_rgb[:, 0] + 0.7152 * material.flat_rgb[:, 1] + 0.0722 * material.flat_rgb[:, 2]).astype(np.float32)
    assert np.all(achro[~valid] == -1.)
    for c in range(3):
        assert np.array_equal(achro[valid, c], lum[valid])
    # an entry with one non-positive channel is invalid as a whole
    m = merl.MERL()
    cube = np.ones((180, 90, 90, 3))
    cube[3, 4, 5, 1] = 0.
    cube[7, 8, 9] = (-1., 2., 2.)
    m.cube_rgb = cube
    p = m.packed_table()
    assert np.all(p[(3 * 90 + 4) * 90 + 5] == -1.) and np.all(p[(7 * 90 + 8) * 90 + 9] == -1.) and (p[:, 0] == -1.).sum() == 2
    m.cube_rgb = np.full((180, 90, 90, 3), -1.)
    with pytest.raises(ValueError, match='no valid entry'):
        m.packed_table()


def test_the_fixture_holds_the_conditions_the_gpu_tests_rest_on(material):
    """From the fixture alone: enough rows take the slow path (their per-axis nearest cell is invalid), and the rows whose two
    nearest entries are within 2e-6 rad of each other — the only rows where an index may differ — are under 1 %."""
    valid = (material.flat_rgb > 0).all(1)
    sets = mc.query_sets(SPHERE['a_rusink'])
    assert {k: v.shape[0] for k, v in sets.items()} == {'cslice': 8100, 'uniform': 4096, 'outside': 1536, 'scene': 31646}
    slow = {}
    for name, q in sets.items():
        idx, dist, gap = GOLD['q_%s_idx' % name], GOLD['q_%s_dist' % name], GOLD['q_%s_gap' % name]
        assert idx.shape == (q.shape[0],) and valid[idx].all()
        assert np.allclose(np.linalg.norm(q.astype(np.float64) - mc.grid_rusink(idx), axis=1), dist, rtol=0, atol=1e-12)
        first = mc.nearest_cell(q.astype(np.float64))
        slow[name] = int((~valid[first]).sum())
        assert np.array_equal(idx[valid[first]], first[valid[first]])      # the per-axis nearest cell is the tree's answer where valid
        assert (gap < 2e-6).mean() < 0.01, name
    assert slow['uniform'] >= 1000
    from nerfactor_amd.brdf.renderer import SphereRenderer
    sphere_slow = 0
    for s, (ims, spp) in (('a', (16, 1)), ('b', (6, 4))):
        r = SphereRenderer('white', ims=ims, spp=spp)
        rows = merl.dir2rusink(r.ldir, r.vdir)[r.lvis.astype(bool)]
        assert GOLD[s + '_ref_idx'].shape == (rows.shape[0],) and valid[GOLD[s + '_ref_idx']].all()
        sphere_slow += int((~valid[mc.nearest_cell(rows)]).sum())
    assert sphere_slow >= 100
