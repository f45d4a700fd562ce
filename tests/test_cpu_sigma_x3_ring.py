"""The weight ring and the A-pair buffer of the pipelined fp32-class density kernel (csrc/nerf_sigma_x3_pipe.hip) in the
happens-before model of test_cpu_ring_protocol.py, as test_cpu_nerf_fold.py restates it for a cyclic sequence with an
explicit chunk -> slot map.  No GPU.

The kernel walks 66 positions per point tile: chunks 0..63 (the encoder), chunk 64 (the sigma tile) and one IDLE position,
the top of the point-tile loop, where nothing is fetched for itself, multiplied or read.  Chunk c lives in [hi | lo] slot
c % 3.  Position p issues the LDS-DMA of the chunk of position p + 2 at its start and waits for it (vmcnt(0)) before the
barrier that ends it; the reads of the chunk of position p are those of tile p and the pre-read of its first A pairs in tile
p - 1, in front of that tile's barrier.  An event of position i is ordered before an event of position j iff i < j.
  RAW  a chunk has landed, and a barrier has passed, before any wave reads it
  WAR  every wave's reads of a slot's previous occupant are COMPLETE, and a barrier has passed, before any wave issues the
       DMA over the slot.  The kernel issues that DMA in the tile right behind the barrier (three slots, distance two), so
       "complete" has to hold at the barrier itself: the barrier is `s_waitcnt vmcnt(0) lgkmcnt(0)` + `s_barrier`.  With a
       bare s_barrier a read would only be known to have been ISSUED there, and the model then asks for a whole tile in
       between (slack = 1), which three slots do not have."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(__file__), '..', 'nerfactor_amd', 'csrc')
N_CHUNKS, N_SEQ, RING, DIST, PRE_A = 65, 66, 3, 2, 3
SLOT_FRAGS = 24                  # mlp_engine.hpp:kSlotFrags, per half of a [hi | lo] slot
GEO_FWD_FRAGS = 8 * 8 + 32 * 16 + 8 * 24 + 16 * 16 + 16      # nerf_geom_layout.hpp:kGeoFwdFrags
GEO_FRAGS = GEO_FWD_FRAGS + (7 * 8 + 2 * 2) * 16
GEO_FLOATS = 8 * 256 + 32 + 256


def used_frags(k):
    return 4 if k < 8 else 16 if k < 40 else 20 if k < 48 else 16


def blob_frags(k):               # nerf_layout.hpp:chunk_frags (layer 0 and layer 5 are padded in the blob)
    return 8 if k < 8 else 16 if k < 40 else 24 if k < 48 else 16


def frag_offset(k):
    return sum(blob_frags(i) for i in range(k))


def chunk_at(p, n_seq=N_SEQ, n_chunks=N_CHUNKS):
    """the chunk of position p of the walk, None at an idle position"""
    c = p % n_seq
    return c if c < n_chunks else None


def violations(slot=lambda k: k % RING, dist=DIST, landed_after=0, n_seq=N_SEQ, n_chunks=N_CHUNKS, passes=3, slack=0):
    out = []
    for p in range(passes * n_seq):
        c = chunk_at(p, n_seq, n_chunks)
        if c is None:
            continue
        issue_tile = p - dist                       # (the first pass: the prologue and the first loop top, earlier still)
        if not issue_tile + landed_after < p - 1:   # landed before a barrier that precedes the pre-read in tile p - 1
            out.append(('RAW', p))
        prev = [r for r in range(p) if chunk_at(r, n_seq, n_chunks) is not None
                and slot(chunk_at(r, n_seq, n_chunks)) == slot(c)]
        if prev and not prev[-1] + slack < issue_tile:
            out.append(('WAR', p))
    return out


def test_the_shipped_protocol_is_race_free_over_three_passes():
    assert violations() == []


def test_every_chunk_is_fetched_exactly_once_per_pass_two_positions_ahead():
    """what the kernel's `K2 = (K + kDist) % kSeq; if (K2 < kNChunks) dma_chunk<K2>` and the loop top's dma_chunk<1> issue"""
    issued = {}
    for k in range(N_CHUNKS):                       # tile K
        k2 = (k + DIST) % N_SEQ
        if k2 < N_CHUNKS:
            issued.setdefault(k2, []).append(k)
    issued.setdefault(1, []).append(N_SEQ - 1)      # the idle position issues chunk 1
    assert sorted(issued) == list(range(N_CHUNKS))
    for c, by in issued.items():
        assert by == [(c - DIST) % N_SEQ], (c, by)
    assert (N_CHUNKS - 2 + DIST) % N_SEQ == N_SEQ - 1          # tile 63 would fetch the idle position's chunk: nothing


def test_the_model_catches_the_alternatives():
    # the 65-chunk sequence without the idle position: chunk 0 of the next pass is issued over chunk 63 while it is read
    assert any(v[0] == 'WAR' and v[1] >= 65 for v in violations(n_seq=65))
    # fetch distance 3 on three slots: the DMA overwrites the slot the tile is reading
    assert ('WAR', 3) in violations(dist=3, landed_after=1)
    # distance 2 with a chunk left in flight at the barrier: the pre-read of the next tile may see it missing
    assert any(v[0] == 'RAW' for v in violations(landed_after=1))
    # a bare s_barrier (reads merely issued): a whole tile between last read and overwrite is needed, and is not there
    assert any(v[0] == 'WAR' for v in violations(slack=1))
    # ... an explicit map on 65 chunks can not help either: chunk 0 needs a slot that differs from those of chunks 63 and 64
    # AND from those of chunks 1 and 2
    for s0 in range(RING):
        bad = violations(slot=lambda k: s0 if k == 0 else k % RING, n_seq=65)
        assert bad, s0


def test_dma_pieces_cover_every_used_fragment_inside_slot_and_blob():
    """dma_chunk<K>: wave w moves n = used / 4 one-KiB pieces per half, fragments [w n, (w + 1) n) of the chunk"""
    for k in range(N_CHUNKS):
        n = used_frags(k) // 4
        assert n * 4 == used_frags(k) and 1 <= n <= 5           # lds_dma_pieces<N>: 1 .. 5 pieces per statement
        frags = sorted(w * n + i for w in range(4) for i in range(n))
        assert frags == list(range(used_frags(k)))
        assert used_frags(k) <= blob_frags(k) <= SLOT_FRAGS
        for half in range(2):
            lds_end = (k % RING) * 2 * SLOT_FRAGS + half * SLOT_FRAGS + used_frags(k)
            assert lds_end <= RING * 2 * SLOT_FRAGS
            assert half * GEO_FRAGS + frag_offset(k) + used_frags(k) <= (half + 1) * GEO_FRAGS
    assert frag_offset(64) + 16 == GEO_FWD_FRAGS
    assert RING * 2 * SLOT_FRAGS * 1024 + GEO_FLOATS * 4 <= 160 * 1024


def test_the_a_pair_buffer_carries_across_tiles():
    """read_a<K, s + kPreA> into entry (s + kPreA) % 4 at k-step s, consumed from entry s % 4: every k-step multiplies its own
    fragment, and no entry is overwritten before its k-step has been issued"""
    buf = [None] * (PRE_A + 1)
    for e in range(PRE_A):                                      # the loop top: the head of chunk 0
        buf[e] = (0, e)
    for k in range(N_CHUNKS):
        ks = used_frags(k)
        assert ks % (PRE_A + 1) == 0
        for s in range(ks):
            e = s + PRE_A
            c, f = (k, e) if e < ks else (k + 1, e - ks)
            if c < N_CHUNKS:
                assert buf[e % (PRE_A + 1)] != (k, s)           # the entry being refilled is not this k-step's
                buf[e % (PRE_A + 1)] = (c, f)
                assert f < used_frags(c)
                assert c == k or c == k + 1                     # a pre-read never reaches past the next chunk
            assert buf[s % (PRE_A + 1)] == (k, s), (k, s)


def test_model_matches_the_kernel_constants():
    src = open(os.path.join(CSRC, 'nerf_sigma_x3_pipe.hip')).read()
    for line in ('constexpr int kRing = 3;', 'constexpr int kDist = 2;', 'constexpr int kPreA = 3;',
                 'constexpr int kNChunks = 65;', 'constexpr int kSeq = 66;',
                 'constexpr int slot_of(int k) { return k % kRing; }',
                 'constexpr int used_frags(int k) { return k < 8 ? 4 : k < 40 ? 16 : k < 48 ? 20 : 16; }',
                 'constexpr int K2 = (K + kDist) % kSeq;', 'if constexpr (K2 < kNChunks) dma_chunk<K2>(cx);',
                 'dma_chunk<0>(cx);', 'dma_chunk<1>(cx);'):
        assert line in src, line
    # both barriers (the tile's and the idle position's) wait for the DMA and drain the LDS reads
    assert len(re.findall(r'asm volatile\("s_waitcnt vmcnt\(0\) lgkmcnt\(0\)\\n\\ts_barrier" ::: "memory"\);', src)) == 2
    assert src.count('s_barrier"') == 2 and '__syncthreads' not in src
    lay = open(os.path.join(CSRC, 'nerf_geom_layout.hpp')).read()
    assert 'constexpr int kGeoFwdFrags = chunk_frag_offset(64) + 16;' in lay
    assert 'constexpr int kGeoBwdFrags = (7 * 8 + 2 * 2) * 16;' in lay
    assert 'constexpr int kGeoFloats = kGeoWSig + 256;' in lay
    eng = open(os.path.join(CSRC, 'mlp_engine.hpp')).read()
    assert 'constexpr int kSlotFrags = 24;' in eng
