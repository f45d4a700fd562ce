"""The bottleneck fold of the NeRF render path, without a GPU (csrc/nerf_fold.hip, nerf_fold_layout.hpp, nerf_mlp_v6.hip,
nerf_v6_engine.hpp).

The network's bottleneck layer has no activation and feeds rgb_out[0] only, so the render kernels multiply enc[7]'s output
by W' = Wb W0a directly and skip the bottleneck's 8 tiles.  Checked here: the arithmetic against the oracle, the fragment-
level restatement of the device fold kernel (row permutations included) through a lane-level walk of the 70-tile kernels, and
the LDS weight ring of the 70-chunk sequence in the happens-before model of test_cpu_ring_protocol.py."""
import os
import re

import numpy as np
import pytest

from oracle import nerf_ref
from tests import common, emu, nerf_fold_ref as nf

CSRC = os.path.join(os.path.dirname(__file__), '..', 'nerfactor_amd', 'csrc')


def _rays(n_rays, n_samples):
    """the inputs of tests/test_gpu_nerf.py::test_nerf_mlp_bf16_vs_oracle"""
    rng = np.random.default_rng(10 + n_rays)
    rayo = rng.uniform(-1, 1, size=(n_rays, 3)).astype(np.float32) * 3
    rayd = nerf_ref.l2_normalize(rng.normal(size=(n_rays, 3)).astype(np.float32), 1, 1e-12)
    z = np.sort(rng.uniform(2, 6, size=(n_rays, n_samples)).astype(np.float32), -1)
    pts = rayo[:, None, :] + rayd[:, None, :] * z[:, :, None]
    return pts, np.broadcast_to(rayd[:, None, :], pts.shape)


def _check(net, pts, views, what):
    want_q = nerf_ref.eval_nerf_at(pts, views, net, quant=nerf_ref.bf16_round)
    bound = 4e-3 * max(1., np.abs(want_q).max())      # the bound of test_nerf_mlp_bf16_vs_oracle
    for from_fp32 in (False, True):
        got = nf.eval_folded(pts, views, net, fold_from_fp32=from_fp32)
        err = np.max(np.abs(got[..., :3] - want_q[..., :3]))
        print('%s, fold from %s weights: max abs(folded - want_q) = %.3g, bound %.3g' % (
            what, 'fp32' if from_fp32 else 'bf16', err, bound))
        assert np.array_equal(got[..., 3], want_q[..., 3]), 'the density does not see the fold'
        assert err < bound


@pytest.mark.parametrize("n_rays,n_samples", [(1, 64), (300, 64), (77, 192), (4, 5)])
def test_folded_network_vs_oracle(n_rays, n_samples):
    net = common.nerf_nets(seed=7)[0]
    pts, views = _rays(n_rays, n_samples)
    _check(net, pts, views, '%d x %d' % (n_rays, n_samples))


@pytest.mark.parametrize("which", [0, 1])
def test_folded_bench_networks_vs_oracle(which):
    """16 384 points through each of the benchmark's two glorot seed-0 networks"""
    net = common.nerf_nets(seed=0)[which]
    pts, views = _rays(256, 64)
    _check(net, pts, views, 'bench net %d' % which)


@pytest.fixture(scope='module')
def packed(nfx_lib):
    from nerfactor_amd import ops
    net = common.nerf_nets(seed=4)[0]
    blob = ops.pack_nerf_weights(*common.nerf_layers(net), 'bf16').numpy()
    return net, blob, nf.fold_blob(blob)


def test_render_blob_layout(packed, nfx_lib):
    net, blob, rblob = packed
    assert rblob.nbytes == nfx_lib.lib.nfx_nerf_fold_workspace_bytes() == 1144 * 1024 + 2496 * 4
    w = blob[:1272 * 1024].reshape(1272, 1024)
    r = rblob[:1144 * 1024].reshape(1144, 1024)
    assert np.array_equal(r[:1024], w[:1024])                                        # the encoder
    assert np.array_equal(r[1024:1040], w[nf.chunk_off(72):nf.chunk_off(73)])        # the sigma tile
    assert np.array_equal(r[-8:], w[-8:])                                            # rgb_out[1]
    for u in range(4):                                                               # view rows and padding
        assert np.array_equal(r[nf.chunk_off_r(65 + u) + 16:nf.chunk_off_r(66 + u)], w[nf.chunk_off(73 + u) + 16:nf.chunk_off(74 + u)])
    fl, rfl = blob[1272 * 1024:].view(np.float32), rblob[1144 * 1024:].view(np.float32)
    keep = np.r_[0:nf.BIAS_RGB0, nf.BIAS_RGB1:nf.N_BIAS]
    assert np.array_equal(rfl[keep], fl[keep])
    # the folded fragments are the logical fold, de-permuted: fragment s, lane (h, n), element j = W'[F(s, h, j)][32 u + n]
    q = nerf_ref.bf16_round
    (wb, bb), (w0, b0) = net['bottleneck'][0], net['rgb_out'][0]
    wf = q(nf.fold_weights(q(wb), q(w0[:256])))
    frag = emu.bf16_bits_to_f32(rblob[:1144 * 1024].view(np.uint16).reshape(1144, 64, 8))
    for u in range(4):
        for s in range(16):
            for h in range(2):
                for j in range(8):
                    got = frag[nf.chunk_off_r(65 + u) + s, 32 * h:32 * h + 32, j]
                    assert np.array_equal(got, wf[nf.hidden_feature(s, h, j), 32 * u:32 * u + 32]), (u, s, h, j)
    assert np.array_equal(rfl[nf.BIAS_RGB0:nf.BIAS_RGB1], nf.fold_bias(bb, q(w0[:256]), b0))


def test_render_blob_through_lane_emulation_matches_the_restatement(packed):
    """The fragments the fold kernel is specified to write, walked lane by lane as the 70-tile kernels do, against the
    NumPy restatement of the folded network (tolerances of test_packed_blob_through_lane_emulation_matches_oracle): a wrong
    row permutation of the folded layer fails here."""
    net, blob, rblob = packed
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 3, size=(32, 3)).astype(np.float32)
    views = nerf_ref.l2_normalize(rng.normal(size=(32, 3)).astype(np.float32), 1, 1e-12)
    got = nf.nerf_tile_folded(rblob, pts, views)
    want = nf.eval_folded(pts[:, None, :], views[:, None, :], net)[:, 0, :]
    np.testing.assert_allclose(got, want, atol=2e-3, rtol=2e-3)
    # the density is the unfolded kernel's, lane for lane
    assert np.array_equal(got[:, 3], emu.nerf_tile(blob, pts, views)[:, 3])


# ----------------------------------------------------------------------------------------------------------------------
# The weight ring of the 70-chunk sequence.  test_cpu_ring_protocol.py's model (chunk c in slot c % ring, sequence a
# multiple of the ring) restated for an arbitrary chunk -> slot map over a cyclic sequence: position p of the walk holds
# chunk p % 70.  An event of tile i is ordered before an event of tile j iff i < j (the barrier of tile i lies between).
#   RAW  the chunk read at position p was issued in tile p - dist and has landed before the barrier of tile
#        p - dist + landed_after; its first read is the pre-read before the barrier of tile p - 1
#   WAR  the slot's previous occupant (the latest earlier position in the same slot) was last read in its own tile, which
#        must lie before the tile that issues the overwrite
# ----------------------------------------------------------------------------------------------------------------------
N_CHUNKS = 70


def slot_dma(k):        # variant 7: 6 slots, LDS-DMA
    return k % 6 if k < 66 else k - 65


def slot_staged(k):     # variants 6 / 8: register-staged, a 4th slot for chunk 69
    return 3 if k == 69 else k % 3


def violations(slot, dist, landed_after, n_chunks=N_CHUNKS, passes=3, slack=0):
    out = []
    for p in range(passes * n_chunks):            # three passes: the wrap is part of the protocol
        issue_tile = p - dist
        if not issue_tile + landed_after < p - 1:
            out.append(('RAW', p))
        prev = [r for r in range(p) if slot(r % n_chunks) == slot(p % n_chunks)]
        if prev and not prev[-1] + slack < issue_tile:
            out.append(('WAR', p))
    return out


@pytest.mark.parametrize('name,kw', [
    ('variant 6: chunk k+2 stored at the end of tile k', dict(slot=slot_staged, dist=2, landed_after=0)),
    ('variant 7: chunk k+3 issued in tile k, vmcnt leaves one chunk in flight', dict(slot=slot_dma, dist=3, landed_after=1)),
    ('variant 8: fetched in tile k-1, stored at the end of tile k', dict(slot=slot_staged, dist=2, landed_after=0)),
])
def test_folded_ring_protocols_are_race_free(name, kw):
    assert violations(**kw) == [], name


def test_folded_dma_ring_keeps_a_whole_tile_between_last_read_and_overwrite():
    """The DMA is issued at the START of a tile: the slot it targets was last read two tiles earlier or more, as on the
    unfolded ring (there: three), never in the tile just closed."""
    assert violations(slot=slot_dma, dist=3, landed_after=1, slack=1) == []


def test_the_restated_model_agrees_with_the_original_and_catches_bad_maps():
    # on a sequence that is a multiple of the ring, with chunk % ring, it is the model of test_cpu_ring_protocol.py
    assert violations(lambda k: k % 3, 2, 0, n_chunks=78) == []
    assert violations(lambda k: k % 6, 3, 1, n_chunks=78) == []
    assert any(v == ('WAR', 3) for v in violations(lambda k: k % 3, 3, 1, n_chunks=78))
    assert any(v[0] == 'RAW' for v in violations(lambda k: k % 6, 3, 2, n_chunks=78))
    # 70 chunks on the unchanged maps.  3 slots: chunk 0 of the next pass would be stored over chunk 69 while it is read.
    assert any(v[0] == 'WAR' and v[1] >= 70 for v in violations(lambda k: k % 3, 2, 0))
    # 6 slots: k % 6 survives with a barrier alone between the last read of chunks 66..69 and the DMA issued over them
    # at the start of the next tile — the bare s_barrier does not drain a wave's LDS reads, so the kernel keeps a whole
    # tile there (slot_dma), which k % 6 does not
    assert violations(lambda k: k % 6, 3, 1) == []
    assert any(v[0] == 'WAR' and v[1] >= 70 for v in violations(lambda k: k % 6, 3, 1, slack=1))


def test_ring_model_matches_the_kernel_constants():
    src = open(os.path.join(CSRC, 'nerf_v6_engine.hpp')).read()
    assert 'enum class Seq { Packed, Render, Geom };' in src
    assert 'template <int DMA, Seq S> constexpr int ring_of = DMA == 1 ? 6 : S == Seq::Render ? 4 : 3;' in src
    # the folded maps belong to the render sequence alone; the packed and the GEOM sequence use k % ring
    assert re.search(r'constexpr int slot_of\(int k\) \{\s*if \(S != Seq::Render\) return k % ring_of<DMA, S>;\s*'
                     r'return DMA == 1 \? \(k < 66 \? k % 6 : k - 65\) : \(k == 69 \? 3 : k % 3\);\s*\}', src)
    assert re.search(r'template <int DMA> constexpr int dist_of = DMA == 1 \? kDmaDist : DMA \? 3 : 2;', src)
    assert 'constexpr int kDmaDist = 3;' in src
    assert ('template <Seq S> constexpr int n_chunks = S == Seq::Render ? nerf::fold::kNChunks : S == Seq::Geom ? 66 : '
            'nerf::kNChunks;') in src
    lay = open(os.path.join(CSRC, 'nerf_fold_layout.hpp')).read()
    assert 'constexpr int kNChunks = 70;' in lay
    assert 'constexpr int kNChunks = 78;' in open(os.path.join(CSRC, 'nerf_layout.hpp')).read()
    assert '#if' not in src and '.hip"' not in open(os.path.join(CSRC, 'nerf_sigma_v6.hip')).read()
    assert max(slot_dma(k) for k in range(70)) == 5 and max(slot_staged(k) for k in range(70)) == 3
