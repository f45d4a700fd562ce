"""The pipelined fp32-class density kernel (csrc/nerf_sigma_x3_pipe.hip, the default) against the kernel it replaces
(nerf_geom_x3.hip:nerf_sigma_x3_kernel<false>, option sigma_x3_variant = 0): the same MFMAs on the same operands in the same
order, so the same bits — in plain mode, in both list modes and through the one-launch refinement of every ray's last sample
(nfx_nerf_sigma_refine_last).  Shapes: the smallest at which the kernel takes another path (one point, a partial and an exact
128-point tile, one point more, a tile that spans rays, and 256 x 128 + 1 points: the first count at which a workgroup of the
256-block grid runs a second tile, so the weight ring wraps from the sigma chunk back to chunk 0).  Both kernels take "which
sample is point m, where does its density go" from csrc/nerf_points.hpp: the 840 points of tests/nerf_point_cases.py go
through both in the two list forms and the last-sample form."""
import numpy as np
import pytest
import torch

from tests import common, nerf_point_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _inputs(n_rays, s, seed, dev):
    rng = np.random.default_rng(seed)
    rayo = rng.uniform(-1, 1, size=(n_rays, 3)).astype(np.float32) * 3
    rayd = rng.normal(size=(n_rays, 3)).astype(np.float32)
    rayd /= np.linalg.norm(rayd, axis=1, keepdims=True)
    z = np.sort(rng.uniform(2, 6, size=(n_rays, s)).astype(np.float32), -1)
    return tuple(torch.from_numpy(a).to(dev) for a in (rayo, rayd, z))


@pytest.fixture(scope='module')
def blobs(nfx_lib, cuda):
    """fp32-class GEOM blobs of a glorot network (the benchmark's seed) and of one fitted to a scene"""
    from nerfactor_amd import ops, synth
    from tests.golden import golden_inputs as gi
    out = []
    for net in (synth.nerf_nets(seed=0)[0], gi.trained_nerf_nets()[1]):
        ks, bs = synth.nerf_layers(net)
        out.append(ops.pack_nerf_geom_weights(ks, bs, 'fp32').to(cuda))
    return out


def _both(nfx_opt, fn):
    nfx_opt.set('sigma_x3_variant', 0)
    old = fn()
    nfx_opt.unset('sigma_x3_variant')
    return old, fn()


@pytest.mark.parametrize('n_rays,s', [(1, 1), (127, 1), (128, 1), (129, 1), (300, 3), (256 * 128 + 1, 1)])
def test_plain_mode_has_the_old_kernel_s_bits(nfx_lib, cuda, nfx_opt, blobs, n_rays, s):
    from nerfactor_amd import ops
    o, d, z = _inputs(n_rays, s, 11, cuda)
    for which, blob in enumerate(blobs):
        old, new = _both(nfx_opt, lambda: ops.nerf_sigma_fwd(o, d, z, blob, 'fp32'))
        assert torch.isfinite(old).all() and float(old.abs().max()) > 0
        assert torch.equal(new, old), (which, int((new != old).sum()))


def test_second_tile_of_a_workgroup_is_repeatable(nfx_lib, cuda, blobs):
    from nerfactor_amd import ops
    o, d, z = _inputs(256 * 128 + 1, 1, 12, cuda)
    first = ops.nerf_sigma_fwd(o, d, z, blobs[1], 'fp32')
    assert torch.equal(ops.nerf_sigma_fwd(o, d, z, blobs[1], 'fp32'), first)


@pytest.mark.parametrize('count', [0, 1, 129])
@pytest.mark.parametrize('stride', [4, 1])
def test_list_modes_have_the_old_kernel_s_bits_and_leave_the_rest_alone(nfx_lib, cuda, nfx_opt, blobs, stride, count):
    from nerfactor_amd import ops
    n, s = 300, 5
    o, d, z = _inputs(n, s, 13, cuda)
    rng = np.random.default_rng(count)
    picked = rng.permutation(n * s)[:count].astype(np.int32)
    lst = torch.full((n * s,), -1, dtype=torch.int32, device=cuda)     # capacity n s; entries past the count are never read
    lst[:count] = torch.from_numpy(picked).to(cuda)
    cnt = torch.tensor([count], dtype=torch.int32, device=cuda)
    listed = torch.zeros(n * s, dtype=torch.bool, device=cuda)
    listed[torch.from_numpy(picked.astype(np.int64)).to(cuda)] = True
    for blob in blobs:
        want = ops.nerf_sigma_fwd(o, d, z, blob, 'fp32').reshape(-1)

        def run():
            if stride == 1:
                out = torch.full((n, s), SENTINEL, device=cuda)
                ops.nerf_sigma_fwd_list(o, d, z, blob, lst, cnt, out, 'fp32')
                return out
            out = torch.full((n, s, 4), SENTINEL, device=cuda)
            p = ops._ptr
            nfx_lib.check(nfx_lib.lib.nfx_nerf_sigma_refine(p(o), p(d), p(z), n, s, p(blob), p(lst), p(cnt), p(out), ops._stream()),
                          'nfx_nerf_sigma_refine')
            return out
        old, new = _both(nfx_opt, run)
        assert torch.equal(new, old)
        sig = new.reshape(-1) if stride == 1 else new[..., 3].reshape(-1)
        assert torch.equal(sig[listed], want[listed])
        assert bool((sig[~listed] == SENTINEL).all())
        if stride == 4:
            assert bool((new[..., :3] == SENTINEL).all())


@pytest.mark.parametrize('n_rays,s', [(129, 64), (1, 2)])
def test_last_sample_entry_writes_that_density_and_nothing_else(nfx_lib, cuda, nfx_opt, blobs, n_rays, s):
    from nerfactor_amd import ops
    o, d, z = _inputs(n_rays, s, 14, cuda)
    gen = torch.Generator(device='cpu').manual_seed(3)
    before = torch.randn(n_rays, s, 4, generator=gen).to(cuda)
    for blob in blobs:
        want = ops.nerf_sigma_fwd(o, d, z[:, -1:].contiguous(), blob, 'fp32')[:, 0]
        for variant in (None, 0):
            if variant is None:
                nfx_opt.unset('sigma_x3_variant')
            else:
                nfx_opt.set('sigma_x3_variant', variant)
            rgbs = before.clone()
            assert ops.nerf_refine_last_sample(o, d, z, rgbs, blob) is rgbs
            assert torch.equal(rgbs[:, -1, 3], want)
            rest = torch.ones(n_rays, s, 4, dtype=torch.bool, device=cuda)
            rest[:, -1, 3] = False
            assert torch.equal(rgbs[rest].view(torch.int32), before[rest].view(torch.int32))


def test_last_sample_entry_leaves_a_one_sample_ray_alone(nfx_lib, cuda, blobs):
    from nerfactor_amd import ops
    o, d, z = _inputs(7, 1, 15, cuda)
    before = torch.full((7, 1, 4), SENTINEL, device=cuda)
    rgbs = before.clone()
    assert ops.nerf_refine_last_sample(o, d, z, rgbs, blobs[0]) is rgbs
    assert torch.equal(rgbs, before)


@pytest.mark.parametrize('s', [105, 7])
@pytest.mark.parametrize('name', pc.SETS)
def test_the_840_points_have_the_old_kernel_s_bits_in_every_point_form(nfx_lib, cuda, nfx_opt, name, s):
    """List with stride 4 (nfx_nerf_sigma_refine, the kernel call of nerf_refine_coarse), list with stride 1
    (nerf_sigma_fwd_list) and last sample (nerf_refine_last_sample) on the 840-point sets, as [8, 105] and [120, 7]: both
    kernels write the same bits, they are nerf_sigma_fwd's at those samples, and nothing else is written.  The list is 333
    samples in no order: two 128-point tiles and a partial one."""
    from nerfactor_amd import ops
    ps = pc.point_set(name)
    blob = ops.pack_nerf_geom_weights(*common.nerf_layers(ps.net), prec='fp32').to(cuda)
    o, d, z = (torch.from_numpy(np.array(a)).to(cuda) for a in ps.layout(s))
    n = pc.N // s
    want = ops.nerf_sigma_fwd(o, d, z, blob, 'fp32').reshape(-1)
    picked = np.random.default_rng(840).permutation(pc.N)[:333]
    lst = torch.full((pc.N,), -1, dtype=torch.int32, device=cuda)
    lst[:333] = torch.from_numpy(picked.astype(np.int32)).to(cuda)
    cnt = torch.tensor([333], dtype=torch.int32, device=cuda)
    listed = torch.zeros(pc.N, dtype=torch.bool, device=cuda)
    listed[torch.from_numpy(picked).to(cuda)] = True
    last = torch.zeros(n, s, dtype=torch.bool, device=cuda)
    last[:, -1] = True
    p = ops._ptr

    def stride4():
        out = torch.full((n, s, 4), SENTINEL, device=cuda)
        nfx_lib.check(nfx_lib.lib.nfx_nerf_sigma_refine(p(o), p(d), p(z), n, s, p(blob), p(lst), p(cnt), p(out), ops._stream()),
                      'nfx_nerf_sigma_refine')
        return out

    def stride1():
        return ops.nerf_sigma_fwd_list(o, d, z, blob, lst, cnt, torch.full((n, s), SENTINEL, device=cuda), 'fp32')

    def last_sample():
        return ops.nerf_refine_last_sample(o, d, z, torch.full((n, s, 4), SENTINEL, device=cuda), blob)

    for form, written in ((stride4, listed), (stride1, listed), (last_sample, last.reshape(-1))):
        old, new = _both(nfx_opt, form)
        assert torch.equal(new.view(torch.int32), old.view(torch.int32)), (form.__name__, int((new != old).sum()))
        sig = new.reshape(-1) if form is stride1 else new[..., 3].reshape(-1)
        assert torch.equal(sig[written], want[written]), form.__name__
        assert bool((sig[~written] == SENTINEL).all()), form.__name__
        if form is not stride1:
            assert bool((new[..., :3] == SENTINEL).all()), form.__name__
