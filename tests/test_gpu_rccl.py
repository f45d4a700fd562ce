"""RCCL under test with the one rank a one-GPU box has (VERDICT r05 "missing" #2): the training
step's collectives — FlatBucket.all_reduce on a device tensor, broadcast_model, the max-over-ranks of the bench — through
`backend='nccl'` (= RCCL on ROCm) with world_size 1, eager and captured in the step's hipGraph, and bench.py launching
its own ranks.  Each case runs in a subprocess (tests/rccl_worker.py): process groups are process-wide state.

Reference: the training step is defined under a distribution strategy (nerfactor/trainvali.py:259-266, 285, 289, 322)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT',
                                                            'NFX_BENCH_REHEARSAL', 'NFX_REHEARSAL')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.update(extra)
    return env


def worker(case):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'rccl_worker.py'), case], env=_env(), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith('{')][-1])


def test_flat_bucket_all_reduce_on_rccl_with_one_rank(nfx_lib, cuda):
    """init_process_group('nccl', world_size=1) -> FlatBucket.all_reduce on the device bucket: the collective is really
    issued (counted), the values do not move, on the current stream and in the side-stream form (work queued before the
    call is seen by the collective, work queued after it sees its result)."""
    out = worker('bucket')
    assert out['backend'] == 'nccl'
    assert out['collectives_without_group'] == 0
    assert out['collectives_current_stream'] == 1 and out['unchanged_current_stream']
    assert out['collectives_side_stream'] == 2 and out['unchanged_side_stream']
    assert out['max_over_ranks'] == 1.5 and out['sum_over_ranks'] == 2.5


@pytest.mark.determinism
def test_train_step_under_a_one_rank_rccl_group_equals_the_step_without_a_group(nfx_lib, cuda):
    """optim.train_step x 10 (NeRFactor-microfacet, jitter on) with no process group, then under an initialised nccl
    group of one rank: ten all-reduces of [gradients | loss] on RCCL, losses / parameters / optimizer state bit for bit."""
    out = worker('step')
    assert out['backend'] == 'nccl' and out['collectives'] == 10
    assert out['finite'] and out['losses_equal'] and out['params_equal'] and out['vhat_equal']
    assert out['loss_last'] < out['loss_first']


@pytest.mark.determinism
def test_graphed_train_step_captures_the_rccl_all_reduce(nfx_lib, cuda):
    """optim.GraphedTrainStep(capture_collective=True) under the one-rank nccl group: the all-reduce is issued ONCE — at
    capture — and replayed as a node of the hipGraph with every later step (2 eager warm-up steps + 1 capture = 3 Python-
    level calls for 10 steps); the result equals the graphed step without a group bit for bit.  This is the decision of
    optim.GraphedTrainStep._capturable: an RCCL all-reduce IS capturable; with more than one rank it stays opt-in."""
    out = worker('graph')
    assert out['backend'] == 'nccl' and out['graphs'] == [1, 1]
    assert out['collectives'] == 3, out
    assert out['finite'] and out['losses_equal'] and out['params_equal'] and out['vhat_equal']


def _bench(args, **env):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=_env(**env), cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)


def test_bench_gpus_2_on_a_one_gpu_box_is_a_json_error(nfx_lib, cuda):
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("the box has two GPUs")
    res = _bench(['--gpus', '2', '--steps', '1', '--warmup', '0'])
    assert res.returncode == 2
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and 'error' in json.loads(lines[0]) and json.loads(lines[0])['gpus_visible'] == 1


def test_bench_launches_its_own_ranks(nfx_lib, cuda, tmp_path):
    """`python bench.py --gpus 2` with no torchrun around it and NFX_BENCH_REHEARSAL=1 (both ranks on GPU 0, gloo):
    bench.py re-executes itself as two ranks and rank 0 prints the one line with world_size 2.  WITH the CPU baselines and
    parity blocks that only rank 0 runs: none of them may contain a collective (round 6: the training legs' reference-step parity
    did — ten training steps of its own, whose all-reduce waited for ranks that were not there; it is one-process-only now)."""
    res = _bench(['--full', '--gpus', '2', '--steps', '1', '--warmup', '0', '--legs', 'nerf,train,nerfactor_microfacet', '--train-models',
                  'nerfactor_microfacet', '--cpu-budget', '1'], NFX_BENCH_REHEARSAL='1')
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['world_size'] == 2 and line['n_gpus'] == 2 and line['collective_backend'] == 'gloo' and 'rehearsal' in line
    assert line['config']['views_per_step'] == 2 and line['value'] > 0
    assert line['legs']['train_nerfactor_microfacet']['ms_per_step'] > 0 and line['legs']['nerfactor_microfacet']['ms_per_step'] > 0
    assert line['parity']['rays_above_tol'] == 0 and line['parity']['vs_reference_python']['rays_above_tol'] == 0
    assert 'cpu_baseline' not in line                  # (timed at N = 1 only)


def test_bench_force_group_runs_the_training_leg_on_rccl(nfx_lib, cuda):
    """--force-group: one rank, nccl group initialised, the line says `collective_backend: nccl` and the training leg's
    all-reduce went through RCCL (train.*.collective in the detail file)."""
    res = _bench(['--full', '--steps', '1', '--warmup', '0', '--legs', 'train', '--train-models', 'nerfactor_microfacet', '--no-cpu-baseline',
                  '--force-group'])
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith('{"metric"')][-1])
    assert line['collective_backend'] == 'nccl' and line['world_size'] == 1
    detail = json.load(open(os.path.join(ROOT, 'bench_detail.json')))
    assert detail['train']['nerfactor_microfacet']['collective'].startswith('nccl all_reduce')
