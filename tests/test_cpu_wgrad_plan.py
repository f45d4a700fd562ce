"""The host-side slab plan of the batched weight-gradient GEMMs (csrc/train.hip: wgrad_plan, nfx_wgrad_partial_bytes) through
the plan and bytes queries of the C-ABI, over every row count a small batch has and a sample of large ones, under every
option that bends the plan — and the device-side re-cut of the slabs that wgrad_lds_kernel does when it reads its row count
from device memory, restated here: the grid the host launched must cover every count up to the capacity.  No GPU needed."""
import itertools
import os

import numpy as np
import pytest

from tests.conftest import ROOT

NERF = [(63, 256)] + [(256, 256)] * 7 + [(63, 256), (256, 1), (256, 256), (256, 128), (27, 128), (128, 3)]   # capi_train.cpp:kNerfWgradDims
W128 = [(90, 128), (128, 128), (128, 128), (128, 128), (90, 128), (128, 8)]                                  # capi_train.cpp:mlp128_wgrad_calls
BRDF = [(18, 128), (128, 128), (128, 128), (128, 128), (18, 128), (128, 1)]                                  # capi_train.cpp:brdf_rows_wgrad_calls

# every multiple of 16 below 4096, then a sample up to ~70 000 that brackets the 16 384-row rule
ROWS = list(range(16, 4096, 16)) + [4096, 4112, 5008, 8192, 12304, 16368, 16384, 16400, 20000 // 16 * 16, 32768, 40016, 49152,
                                    65536, 65552, 70000 // 16 * 16]

K_WL_ROWS, MIN_SLAB, LDS_FROM = 64, 256, 16384       # pinned against the source text below


def device_slab(rows16, grid_x):
    """wgrad_lds_kernel with a count (train.hip: `if (bt.count)`): rows16 = round16(count), grid_x = gridDim.x = the host
    plan's n_slabs.  -> the slab length every block uses."""
    slab = ((rows16 + grid_x - 1) // grid_x + K_WL_ROWS - 1) // K_WL_ROWS * K_WL_ROWS
    return np.maximum(slab, MIN_SLAB)


def test_restated_constants_match_the_source():
    src = open(os.path.join(ROOT, 'nerfactor_amd', 'csrc', 'train.hip')).read()
    assert 'constexpr int kWlRows = 64;' in src
    assert 'rows = ((long long)*bt.count + 15) & ~15ll;' in src
    assert 'slab = ((rows + gridDim.x - 1) / gridDim.x + kWlRows - 1) / kWlRows * kWlRows;' in src
    assert 'if (slab < 256) slab = 256;' in src
    assert 'const long long r0 = (long long)blockIdx.x * slab;' in src
    # the grid's x is the host plan's slab count
    assert 'hipLaunchKernelGGL(nfx::wgrad_lds_kernel, dim3((unsigned)bt.n_slabs, (unsigned)blocks)' in src
    assert '*use_lds = force_lds >= 0 ? force_lds != 0 : rows >= 16384;' in src
    assert src.count('const int bs = lds ? 256 : 128;') == 2       # the bytes query and the launcher pad alike


@pytest.mark.parametrize('name,dims', [('nerf', NERF), ('width128', W128), ('brdf_rows', BRDF)])
def test_plan_and_bytes(nfx_lib, nfx_opt, name, dims):
    from nerfactor_amd import ops
    has_wide_dim = any(k > 128 or n > 128 for k, n in dims)
    checked_counted = 0
    for lds, slabs, rounds, narrow in itertools.product((None, 0, 1), (None, 1, 3, 4, 7, 'many'), (None, 0, 2), (None, 0)):
        for key, v in (('wgrad_lds', lds), ('wgrad_rounds', rounds), ('wgrad_narrow', narrow)):
            nfx_opt.unset(key) if v is None else nfx_opt.set(key, v)
        for rows in ROWS:
            forced = rows // 16 + 5 if slabs == 'many' else slabs
            nfx_opt.unset('wgrad_slabs') if forced is None else nfx_opt.set('wgrad_slabs', forced)
            plan = ops.selftest_wgrad_plan(dims, rows)
            slab, n_slabs = plan['slab'], plan['n_slabs']
            ctx = (name, rows, lds, forced, rounds, narrow, plan)
            assert plan['use_lds'] == (rows >= LDS_FROM if lds is None else bool(lds)), ctx
            assert plan['wide'] == (plan['use_lds'] and (has_wide_dim or narrow == 0)), ctx
            if plan['use_lds']:
                assert slab % 64 == 0 and slab >= MIN_SLAB, ctx
            else:
                assert slab % 16 == 0 and slab >= 16, ctx
            assert (n_slabs - 1) * slab < rows <= n_slabs * slab, ctx
            pad = 256 if plan['use_lds'] else 128
            want = sum(n_slabs * (-(-k // pad) * pad * (-(-n // pad) * pad) + -(-n // pad) * pad) * 4 for k, n in dims)
            assert ops.selftest_wgrad_partial_bytes(dims, rows) == want, ctx
            if plan['wide']:
                # every count <= rows: the slabs the device cuts for round16(count) rows, times the grid the host launched for
                # `rows`, reach round16(count) — no counted row is left out
                r16 = np.arange(0, rows + 1, 16, dtype=np.int64)
                short = r16[n_slabs * device_slab(r16, n_slabs) < r16]
                assert short.size == 0, ctx + (short[:4],)
                checked_counted += 1
    assert checked_counted > 0


def test_queries_refuse_bad_tables(nfx_lib):
    from nerfactor_amd import ops
    assert ops.selftest_wgrad_partial_bytes(NERF + NERF[:3], 256) == 0        # 17 calls
    assert ops.selftest_wgrad_partial_bytes(NERF, 24) == 0                     # rows not a multiple of 16
    with pytest.raises(nfx_lib.NfxError, match=r'\(-1\)'):
        ops.selftest_wgrad_plan(NERF + NERF[:3], 256)
    with pytest.raises(nfx_lib.NfxError, match=r'\(-1\)'):
        ops.selftest_wgrad_plan(NERF, 24)
    with pytest.raises(nfx_lib.NfxError, match=r'\(-1\)'):
        ops.selftest_wgrad_plan([(0, 4)], 16)
