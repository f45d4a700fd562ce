"""Writes tests/golden/mesh_components_scene.npz: the two ray oracles of tests/mesh_cases.py on the analytic scene of
tests/mesh_component_cases.py (96 surface rows x 128 lights), against the whole mesh and against its largest component.
Both oracles test every ray against every one of the 11 912 triangles in NumPy, about a minute in all — too long for a test
that runs with every change, so the tests read this file; tests/test_cpu_mesh_components.py recomputes every twelfth row.

    python -m tests.golden.make_mesh_components_golden

Per mesh (`whole_*`, `largest_*`): emu float32 [96, 128] (mesh_cases.emu_lvis, the fp32 emulation of the kernel), lvis uint8
and edge bool [96, 128] (mesh_cases.oracle_lvis64, float64); `inputs`: the SHA-256 of the scene's arrays."""
import os

import numpy as np

from tests import mesh_cases
from tests import mesh_component_cases as mcc

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mesh_components_scene.npz')


def main():
    v, f = mcc.scene_mesh()
    xyz, normal, alpha, lxyz = mcc.scene_rows()
    out = {'inputs': np.frombuffer(bytes.fromhex(mcc.scene_digest()), dtype=np.uint8)}
    v1, f1, _ = mcc.filter_numpy(v, f, mcc.reference('j'), keep_largest=1)
    for name, (mv, mf) in (('whole', (v, f)), ('largest', (v1, f1))):
        out[name + '_emu'] = mesh_cases.emu_lvis(mv, mf, xyz, normal, alpha, lxyz, mcc.EPS)[0]
        ref = mesh_cases.oracle_lvis64(mv, mf, xyz, normal, alpha, lxyz, mcc.EPS)
        assert set(np.unique(ref['lvis'])) <= {0., 1.}
        out[name + '_lvis'], out[name + '_edge'] = ref['lvis'].astype(np.uint8), ref['edge']
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
