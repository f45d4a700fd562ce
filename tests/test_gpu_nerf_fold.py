"""The bottleneck fold of the NeRF render path on the GPU (option `nerf_fold`, on by default for bf16): the density is
bit-identical to the unfolded kernels', the rgb logits stay inside the unfolded kernels' own bound against the bf16-rounded
oracle, the device-side fold writes the NumPy restatement's render blob bit for bit, every variant agrees with every other,
and training does not see the fold."""
import numpy as np
import pytest
import torch

from oracle import nerf_ref
from tests import common, nerf_fold_ref as nf

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def _inputs(n_rays, n_samples, seed=None):
    rng = np.random.default_rng(10 + n_rays if seed is None else seed)
    rayo = rng.uniform(-1, 1, size=(n_rays, 3)).astype(np.float32) * 3
    rayd = nerf_ref.l2_normalize(rng.normal(size=(n_rays, 3)).astype(np.float32), 1, 1e-12)
    z = np.sort(rng.uniform(2, 6, size=(n_rays, n_samples)).astype(np.float32), -1)
    return rayo, rayd, z


@pytest.mark.parametrize("blocks", [256, 3])
@pytest.mark.parametrize("n_rays,n_samples", [(1, 64), (300, 64), (77, 192), (4, 5), (2000, 64)])
def test_fold_keeps_the_density_and_the_rgb_bound(nfx_lib, cuda, nfx_opt, n_rays, n_samples, blocks):
    from nerfactor_amd import ops
    nfx_opt.set("nerf_blocks", str(blocks))       # 3: more tiles than workgroups, the 70-chunk stream wraps
    net = common.nerf_nets(seed=7)[0]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net)).to(cuda)
    rayo, rayd, z = _inputs(n_rays, n_samples)
    args = (dev(rayo, cuda), dev(rayd, cuda), dev(z, cuda), blob)
    nfx_opt.set("nerf_fold", "1")
    on = ops.nerf_mlp_fwd(*args)
    assert torch.equal(on, ops.nerf_mlp_fwd(*args, fold=True)) and torch.equal(on, ops.nerf_mlp_fwd(*args, fold=None))
    nfx_opt.set("nerf_fold", "0")
    off = ops.nerf_mlp_fwd(*args)
    assert torch.equal(off, ops.nerf_mlp_fwd(*args, fold=False))
    nfx_opt.unset("nerf_fold")
    assert torch.equal(on, ops.nerf_mlp_fwd(*args)), "the fold is the default"
    assert torch.equal(on[..., 3], off[..., 3])
    assert not torch.equal(on[..., :3], off[..., :3])
    pts = rayo[:, None, :] + rayd[:, None, :] * z[:, :, None]
    views = np.broadcast_to(rayd[:, None, :], pts.shape)
    want_q = nerf_ref.eval_nerf_at(pts, views, net, quant=nerf_ref.bf16_round)
    bound = 4e-3 * max(1., np.abs(want_q).max())
    # the rgb logits: the channels the fold touches (the density is the unfolded kernel's, bit for bit, above)
    for name, got in (('folded', on), ('unfolded', off)):
        err = np.max(np.abs(got.cpu().numpy()[..., :3] - want_q[..., :3]))
        print('%d x %d, %s: max abs(got - want_q) over rgb = %.3g, bound %.3g' % (n_rays, n_samples, name, err, bound))
        assert err < bound
    print('max abs(folded - unfolded) rgb logits = %.3g' % float((on - off).abs().max()))
    # fp32 has no folded path: the argument is ignored
    blob32 = ops.pack_nerf_weights(*common.nerf_layers(net), prec='fp32').to(cuda)
    a32 = args[:3] + (blob32,)
    assert torch.equal(ops.nerf_mlp_fwd(*a32, prec='fp32', fold=True), ops.nerf_mlp_fwd(*a32, prec='fp32', fold=False))


@pytest.mark.parametrize("seed", [0, 4, 7])
def test_device_fold_writes_the_restated_render_blob(nfx_lib, cuda, seed):
    """The fold is a deterministic fp32 running sum in ascending m (products of two bf16 values are exact): bit for bit."""
    from nerfactor_amd import ops
    for net in common.nerf_nets(seed=seed):
        blob = ops.pack_nerf_weights(*common.nerf_layers(net))
        got = ops.nerf_fold_blob(blob.to(cuda)).cpu().numpy()
        want = nf.fold_blob(blob.numpy())
        assert got.nbytes == want.nbytes
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad.size, bad[:8])


@pytest.mark.determinism
@pytest.mark.parametrize("fold", [1, 0])
def test_every_variant_agrees_with_every_other(nfx_lib, cuda, nfx_opt, fold):
    from nerfactor_amd import ops
    nfx_opt.set("nerf_fold", str(fold))
    net = common.nerf_nets(seed=8)[1]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net)).to(cuda)
    rayo, rayd, z = _inputs(777, 64)
    args = (dev(rayo, cuda), dev(rayd, cuda), dev(z, cuda), blob)
    outs = {}
    for variant in ("7", "6", "8", "1", "0"):
        for blocks in ("256", "5"):
            nfx_opt.set("nerf_variant", variant)
            nfx_opt.set("nerf_blocks", blocks)
            outs[variant, blocks] = ops.nerf_mlp_fwd(*args)
    ref = outs["7", "256"]
    for key, out in outs.items():
        common.assert_same_bits(ref, out, 'nerf_mlp_fwd fold=%d variant %s blocks %s' % ((fold,) + key), row_len=4)


def test_training_forward_is_unfolded(nfx_lib, cuda, nfx_opt):
    from nerfactor_amd import autograd, ops
    net = common.nerf_nets(seed=7)[0]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net)).to(cuda)
    rayo, rayd, z = _inputs(300, 64)
    args = (dev(rayo, cuda), dev(rayd, cuda), dev(z, cuda))
    for setting in ("1", "0"):
        nfx_opt.set("nerf_fold", setting)
        got = autograd.NerfMlp.apply(*args, blob, None, 'bf16')
        assert torch.equal(got, ops.nerf_mlp_fwd(*args, blob, fold=False))


def test_folded_forward_is_capture_safe(nfx_lib, cuda):
    """workspace from torch's allocator, no host synchronisation: the folded call records into a graph and replays"""
    from nerfactor_amd import ops
    net = common.nerf_nets(seed=7)[0]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net)).to(cuda)
    rayo, rayd, z = _inputs(300, 64)
    args = (dev(rayo, cuda), dev(rayd, cuda), dev(z, cuda), blob)
    want = ops.nerf_mlp_fwd(*args, fold=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.nerf_mlp_fwd(*args, fold=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.nerf_mlp_fwd(*args, fold=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_folded_entry_points_validate(nfx_lib, cuda):
    from nerfactor_amd import ops
    lib = nfx_lib.lib
    blob = ops.pack_nerf_weights(*common.nerf_layers(common.nerf_nets(seed=7)[0])).to(cuda)
    ws = torch.empty(lib.nfx_nerf_fold_workspace_bytes(), dtype=torch.uint8, device=cuda)
    assert lib.nfx_nerf_fold_blob(blob.data_ptr(), ws.data_ptr(), ws.numel() - 1, None) == -1
    assert 'too small' in nfx_lib.last_error()
    assert lib.nfx_nerf_fold_blob(blob.data_ptr(), blob.data_ptr() + 1024, ws.numel(), None) == -1
    assert 'overlaps' in nfx_lib.last_error()
    assert lib.nfx_nerf_fold_blob(None, ws.data_ptr(), ws.numel(), None) == -1
