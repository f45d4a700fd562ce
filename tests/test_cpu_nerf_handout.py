"""The hand-out of point tiles in the LDS-DMA render kernel (nerf_mlp_v6.hip, option `nerf_handout`) as a model of its claim
protocol, in the style of test_cpu_ring_protocol.py.

A workgroup's first tile is its index b; every further one is grid + fetch_add(counter, 1).  It claims once in front of its loop
and once in every pass, behind layer 0; the claim of pass k is published to the workgroup's LDS word near the end of pass k and
read at the top of pass k + 1 as the tile of pass k + 2.  Workgroups meet only in the atomics, so a run of the launch is an ORDER
OF THE ATOMICS: which workgroup makes the next claim.  What a workgroup does between two of its claims is fixed.  For every order
(all of them where they can be enumerated, a seeded sample otherwise) the model checks that every tile is started exactly once,
that no workgroup ever holds more than two tiles it has not started, that every workgroup terminates, and where the counter
ends."""
import fnmatch
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = (1, 2, 3, 5)
TILES = range(0, 13)
ENUMERATE_UP_TO = 20000     # orders; beyond that a seeded sample
SAMPLED_ORDERS = 400


class Workgroup:
    """One workgroup between its atomics.  `claim(value)` is the atomic's return; everything up to the next atomic follows."""

    def __init__(self, b, grid, n_tiles, plus_grid=True, exit_ge=True, publish_late=False):
        self.b, self.grid, self.n = b, grid, n_tiles
        self.plus_grid, self.exit_ge, self.publish_late = plus_grid, exit_ge, publish_late
        self.cur = b                # the tile the next pass starts
        self.word = None            # the LDS word
        self.late = None            # publish_late: a claim waiting one more pass for its publication
        self.started = []
        self.unstarted = [b]        # held and not started: the bound is on its length
        self.max_held = 1
        self.passes = 0
        self.in_loop = False
        self.done = False

    def _index(self, value):
        return value + self.grid if self.plus_grid else value

    def _leaves(self, tile):
        return tile >= self.n if self.exit_ge else tile > self.n

    def _hold(self, tile):
        self.unstarted.append(tile)
        self.max_held = max(self.max_held, len(self.unstarted))

    def _top_of_pass(self):
        """-> True when a pass was started (it runs up to its claim), False when the workgroup left the loop."""
        if self._leaves(self.cur):
            self.done = True
            return False
        self.nxt = self.word        # read behind the barrier of the previous pass's last tile
        self.unstarted.remove(self.cur)
        self.started.append(self.cur)
        self.passes += 1
        return True

    def claim(self, value):
        assert not self.done
        tile = self._index(value)
        self._hold(tile)
        if not self.in_loop:        # the claim in front of the loop, written in front of the prologue's barrier
            self.word = tile
            self.in_loop = True
            self._top_of_pass()
            return
        # the claim of this pass; published between the barriers of its last two tiles ...
        if self.publish_late:       # ... or, in the variant the depth bound must catch, one pass later
            if self.late is not None:
                self.word = self.late
            self.late = tile
        else:
            self.word = tile
        self.cur = self.nxt
        self._top_of_pass()


def run(order_source, grid, n_tiles, **kw):
    """order_source(live) -> the index of the workgroup that claims next.  Returns (workgroups, final counter)."""
    wgs = [Workgroup(b, grid, n_tiles, **kw) for b in range(grid)]
    counter, steps = 0, 0
    while True:
        live = [w.b for w in wgs if not w.done]
        if not live:
            return wgs, counter
        steps += 1
        assert steps <= 4 * (grid + n_tiles) + 8, "a workgroup does not terminate"
        wgs[order_source(live)].claim(counter)
        counter += 1


def all_orders(grid, n_tiles, limit, **kw):
    """Every order of the atomics as the list of choices, depth first; None when there are more than `limit`."""
    out, stack = [], [[]]
    while stack:
        prefix = stack.pop()
        it = iter(prefix)
        branch = []

        def source(live):
            c = next(it, None)
            if c is None:
                branch.append(list(live))
                raise StopIteration
            return c
        try:
            run(source, grid, n_tiles, **kw)
            out.append(prefix)
            if len(out) > limit:
                return None
        except StopIteration:
            stack.extend(prefix + [c] for c in branch[0])
    return out


def orders_of(grid, n_tiles):
    # there are at most grid ** (number of atomics) orders, and grid + n_tiles atomics
    full = all_orders(grid, n_tiles, ENUMERATE_UP_TO) if grid ** (grid + n_tiles) <= ENUMERATE_UP_TO else None
    if full is not None:
        return [lambda live, it=iter(o): next(it) for o in full], True
    rng = random.Random(1000 * grid + n_tiles)
    return [lambda live, r=random.Random(rng.random()): r.choice(live) for _ in range(SAMPLED_ORDERS)], False


def check(wgs, counter, grid, n_tiles):
    started = sorted(t for w in wgs for t in w.started)
    assert started == list(range(n_tiles)), started
    assert all(w.done for w in wgs)
    assert max(w.max_held for w in wgs) <= 2, [w.max_held for w in wgs]
    lo = max(n_tiles - grid, 0)
    assert lo <= counter <= lo + 3 * grid, (counter, lo, grid)


@pytest.mark.parametrize('grid', GRIDS)
def test_every_tile_once_depth_two_and_the_counter(grid):
    enumerated = 0
    for n_tiles in TILES:
        # the launcher starts min(tiles, grid) workgroups and none for no tiles; the kernel's protocol holds for the bare grid too
        for g in sorted({grid, min(grid, n_tiles)} - {0}):
            sources, full = orders_of(g, n_tiles)
            enumerated += full
            for source in sources:
                wgs, counter = run(source, g, n_tiles)
                check(wgs, counter, g, n_tiles)
                # what the kernel's comment states: one claim in front of the loop and one per pass
                assert counter == n_tiles + g and sum(w.passes for w in wgs) == n_tiles
    assert enumerated >= (len(TILES) if grid <= 2 else 3)     # grids 1 and 2 are enumerated at every tile count


def test_one_workgroup_walks_every_tile_in_order():
    wgs, counter = run(lambda live: live[0], 1, 12)
    assert wgs[0].started == list(range(12)) and counter == 13


def test_the_model_catches_the_mutations():
    """The three mutations of profiles/nerf_handout/mutations.txt that live in the protocol, and a deeper claim queue."""
    def fails(grid, n_tiles, **kw):
        for seed in range(50):      # a mutated run has atomics of its own: seeded orders, not the enumerated ones
            source = lambda live, r=random.Random(seed): r.choice(live)
            try:
                wgs, counter = run(source, grid, n_tiles, **kw)
                check(wgs, counter, grid, n_tiles)
            except (AssertionError, ValueError):
                return True
        return False
    assert fails(2, 5, plus_grid=False)         # tiles 0 .. grid - 1 are started twice, the last ones never
    assert fails(2, 5, exit_ge=False)           # a workgroup starts tile n_tiles
    assert fails(3, 9, publish_late=True)       # the claim reaches the word a pass later: three tiles held (or a stale word)
    assert not fails(2, 5) and not fails(3, 9)


def test_the_new_entry_points_are_declared_bound_and_exported(nfx_lib):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nfx.h')).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, 'nerfactor_amd', 'csrc', 'libnfx.map')).read()
    exported = re.search(r'global:([^;]*);', version_script).group(1).split()
    for name in ('nfx_nerf_render_workspace_bytes', 'nfx_nerf_mlp_fwd_render'):
        assert re.search(r'^NFX_API\s[^;]*\b%s\s*\(' % name, header, flags=re.M), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
        assert name in nfx_lib.SIGNATURES
    assert 'nerf_handout' in nfx_lib.OPTION_KEYS
    # the render workspace is the render blob and a 16-byte control block behind it
    assert nfx_lib.lib.nfx_nerf_render_workspace_bytes() == nfx_lib.lib.nfx_nerf_fold_workspace_bytes() + 16
    assert nfx_lib.lib.nfx_nerf_fold_workspace_bytes() % 16 == 0
