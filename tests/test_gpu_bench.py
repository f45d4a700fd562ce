"""bench.py as the driver runs it, `python bench.py --gpus 1 --steps K --warmup W` without --full: the headline leg alone —
its line and its `roofline` from the timed steps' events — and none of the CPU work --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


DUMPED = ['fp32_class_rgb', 'geometry_depth', 'geometry_lvis', 'geometry_normal', 'geometry_occu', 'nerf_rgb',
          'nerfactor_albedo', 'nerfactor_brdf', 'nerfactor_lvis', 'nerfactor_microfacet_albedo', 'nerfactor_microfacet_brdf',
          'nerfactor_microfacet_lvis', 'nerfactor_microfacet_normal', 'nerfactor_microfacet_rgb', 'nerfactor_microfacet_rgb_probes',
          'nerfactor_normal', 'nerfactor_rgb', 'nerfactor_rgb_probes', 'olat_rgb_olat', 'relight_rgb_probes', 'train_nerf_losses',
          'train_nerfactor_losses', 'train_nerfactor_microfacet_losses']


def _plain(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT',
                                                            'NFX_BENCH_REHEARSAL', 'NFX_REHEARSAL')}
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1'] + list(extra),
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['metric'].startswith('rays/sec') and line['unit'] == 'rays/s' and line['higher_is_better'] is True
    assert (line['n_gpus'], line['steps'], line['warmup'], line['dtype']) == (1, 2, 1, 'bf16')
    assert line['value'] == pytest.approx(800 * 800 / (line['ms_per_step'] * 1e-3), rel=1e-4)
    assert 0 < line['roofline']['frac'] < 1
    assert not {'cpu_baseline', 'parity'} & set(line), sorted(line)
    return line


def test_plain_run_times_the_headline_leg_alone(nfx_lib, cuda):
    assert 'legs' not in _plain()


def test_plain_run_dumps_the_last_timed_step_of_every_leg(nfx_lib, cuda, tmp_path):
    """--dump-outputs writes what every leg returned in its last timed step, so a plain run with it also runs the other legs'
    timed steps (without their CPU work): the same files as a --full run, the headline frame whole."""
    _plain('--dump-outputs', str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == [n + '.npy' for n in DUMPED]
    rgb = np.load(tmp_path / 'nerf_rgb.npy')
    assert rgb.shape == (800 * 800, 3) and rgb.dtype == np.float32 and np.isfinite(rgb).all()
