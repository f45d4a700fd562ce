"""The lane-pair exchange of the render kernels' front end (mlp_engine.hpp: posenc_sets, exchange_sets; nerf_mlp_v6.hip),
restated in NumPy on the 64-lane map: no GPU.

Today's table (mlp_engine.hpp, the slot map above posenc): lane (h, p) holds in slot q = 8 s + j of column tile c, for an L-band
encoder of the point at column p of column tile c,
    q < 3L      : half 0 -> sin(2^(q/3) x[q%3]),  half 1 -> cos(2^(q/3) x[q%3])
    q = 3L      : half 0 -> x[0],                 half 1 -> x[2]
    q = 3L + 1  : half 0 -> x[1],                 half 1 -> 0
    else        : 0
The one-point-per-lane form: lane (h, p) encodes the point of column tile h alone, both sets of it (set 0 = the half-0 column
of the table, set 1 = the half-1 column), keeps the set of its own half, sends the other set to lane ^ 32 through ds_bpermute
(lane i receives what lane i ^ 32 sent) and files what it receives under the other column tile.  Values are symbols here — (point,
function, band, axis) as one integer — so that "the right slot holds the right function of the right point" is an equality."""
import numpy as np
import pytest

LANES = 64
ENCODERS = (10, 4)                 # PeSlots<10>: 4 k-steps, PeSlots<4>: 2 k-steps
ZERO = 0


def k_steps(bands):
    return (3 * bands + 2 + 7) // 8


def symbol(point, half, q, bands):
    """what the table puts into slot q of half `half` for point `point` (an integer >= 0); 0 is the value zero"""
    if q < 3 * bands:
        fn = 1 + half                                      # 1 sin, 2 cos
        return ((point * 4 + fn) * 16 + q // 3) * 4 + q % 3 + 1
    if q == 3 * bands:
        return ((point * 4 + 3) * 16) * 4 + (2 if half else 0) + 1          # x[0] | x[2]
    if q == 3 * bands + 1 and not half:
        return ((point * 4 + 3) * 16) * 4 + 1 + 1                           # x[1]
    return ZERO


def own_point(lane, n_pts, first=0):
    """flat index of the point lane (h, p) of a wave fetches: column p of column tile h, clamped to the last point"""
    h, p = lane >> 5, lane & 31
    m = first + h * 32 + p
    return min(m, n_pts - 1)


def per_lane_table(bands, n_pts, first=0):
    """[64 lanes, 2 column tiles, slots]: today's front end — every lane encodes both column tiles' points for its half"""
    nq = 8 * k_steps(bands)
    t = np.zeros((LANES, 2, nq), dtype=np.int64)
    for lane in range(LANES):
        h, p = lane >> 5, lane & 31
        for c in range(2):
            point = min(first + c * 32 + p, n_pts - 1)
            t[lane, c] = [symbol(point, h, q, bands) for q in range(nq)]
    return t


def exchanged(bands, n_pts, first=0, source=lambda lane: lane ^ 32, swap_slot=None):
    """[64, 2, slots] of the one-point-per-lane form, dword by dword (a dword = two bf16 slots) as exchange_sets does it.
    `source` and `swap_slot` are the mutations of test_the_model_has_teeth."""
    nq = 8 * k_steps(bands)
    sets = np.zeros((LANES, 2, nq), dtype=np.int64)                     # [lane, set, slot] of the lane's OWN point
    for lane in range(LANES):
        for half in range(2):
            sets[lane, half] = [symbol(own_point(lane, n_pts, first), half, q, bands) for q in range(nq)]
    h = (np.arange(LANES) >> 5)[:, None, None]
    dw = sets.reshape(LANES, 2, nq // 2, 2)                             # [lane, set, dword, element]
    s0, s1 = dw[:, 0], dw[:, 1]
    send = np.where(h, s0, s1)                                          # the set of the OTHER half
    got = send[[source(lane) for lane in range(LANES)]]                 # ds_bpermute
    c0 = np.where(h, got, s0)
    c1 = np.where(h, s1, got)
    if swap_slot is not None:
        c0, c1 = c0.copy(), c1.copy()
        c0[:, swap_slot], c1[:, swap_slot] = np.where(h, s1, got)[:, swap_slot], np.where(h, got, s0)[:, swap_slot]
    return np.stack((c0.reshape(LANES, nq), c1.reshape(LANES, nq)), 1)


def test_the_symbols_tell_every_entry_of_the_table_apart():
    for bands in ENCODERS:
        nq = 8 * k_steps(bands)
        assert k_steps(10) == 4 and k_steps(4) == 2
        syms = [symbol(pt, half, q, bands) for pt in range(64) for half in range(2) for q in range(nq)]
        nonzero = [s for s in syms if s != ZERO]
        assert len(set(nonzero)) == len(nonzero) == 64 * (6 * bands + 3)          # the 6L + 3 features of every point, once
        # zeros: slot 3L + 1 of half 1 and the padding
        assert syms.count(ZERO) == 64 * (2 * nq - 6 * bands - 3)


@pytest.mark.parametrize('bands', ENCODERS)
def test_keep_own_receive_partner_s_is_today_s_table(bands):
    """every lane, both column tiles, every slot — a full wave"""
    want, got = per_lane_table(bands, n_pts=64), exchanged(bands, n_pts=64)
    assert want.shape == got.shape == (LANES, 2, 8 * k_steps(bands))
    assert np.array_equal(want, got)
    # the kept set is out[.][h], the received one out[.][1 - h]: lane (h, p) encoded point 32 h + p itself
    for lane in range(LANES):
        h, p = lane >> 5, lane & 31
        own = {s >> 8 for s in got[lane, h] if s != ZERO}
        other = {s >> 8 for s in got[lane, 1 - h] if s != ZERO}
        assert own == {32 * h + p} and other == {32 * (1 - h) + p}


@pytest.mark.parametrize('bands', ENCODERS)
@pytest.mark.parametrize('n_pts', (1, 31, 32, 33, 63, 64, 65, 96))
def test_a_batch_that_ends_inside_the_wave(bands, n_pts):
    """Lanes past the end take the last point, encode it and take part: every lane's slots are today's, the padded ones included;
    in particular every slot of a STORED point is that point's, in both halves.  With the end inside column tile 0 or on its edge
    the lanes of half 0 hold valid points and their partners none; with the end inside column tile 1 a lane of half 1 past the
    end still sends the partner's column tile 0 its cosines.  first = 64: the same in the second wave of a tile."""
    for first in (0, 64):
        if first >= n_pts:
            continue
        want, got = per_lane_table(bands, n_pts, first), exchanged(bands, n_pts, first)
        assert np.array_equal(want, got)
        for lane in range(LANES):
            h, p = lane >> 5, lane & 31
            for c in range(2):
                m = first + 32 * c + p
                if m < n_pts:
                    assert got[lane, c].tolist() == [symbol(m, h, q, bands) for q in range(8 * k_steps(bands))]


@pytest.mark.parametrize('bands', ENCODERS)
def test_the_model_has_teeth(bands):
    """the two exchange mutations of profiles/nerf_front_end/mutations.txt fail here too"""
    want = per_lane_table(bands, n_pts=64)
    assert not np.array_equal(want, exchanged(bands, 64, source=lambda lane: lane))          # sent to `lane`, not `lane ^ 32`
    for dword in range(4 * k_steps(bands)):
        got = exchanged(bands, 64, swap_slot=dword)                                         # kept and received swapped for one dword
        # (a dword that is zero in both sets — the padding of the last k-step — cannot tell)
        assert np.array_equal(want, got) == (not want.reshape(LANES, 2, -1, 2)[:, :, dword].any())
