"""The six tuned-network weight packers (csrc/pack_nets.cpp) against tests/golden/pack_digests.json: every blob, byte for
byte, is what the library of the commit named in that file produced — values, and which bytes are written at all (each
packer runs into a 0x00-filled and into a 0xA5-filled buffer).  Cases, inputs and digests: tests/golden/make_pack_digests.py."""
import hashlib
import json
import os

import pytest

from tests.golden import make_pack_digests as mpd

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pack_digests.json')) as _h:
    GOLDEN = json.load(_h)['cases']
CASES = mpd.cases()


def test_every_case_has_a_digest():
    assert sorted(c[0] for c in CASES) == sorted(GOLDEN)
    assert len(CASES) == 5 + 12 + 8 + 6 + 4


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_packed_blob_matches_the_recorded_digest(nfx_lib, case):
    for tag, fill in mpd.FILLS:
        want = GOLDEN[case[0]][tag]
        blob = mpd.pack(nfx_lib, case, fill)
        if hashlib.sha256(blob.tobytes()).hexdigest() != want['sha256']:
            kib, nbytes = mpd.first_difference(blob, want)
            # only digests are recorded, one CRC-32 per KiB: the first differing byte is known to its fragment
            print('%s into a 0x%s-filled buffer: %d bytes (recorded %d); first differing byte at offset %s, in fragment %s'
                  % (case[0], tag, blob.size, nbytes, 'unknown' if kib is None else '%d + [0, 1024)' % (1024 * kib), kib))
        assert blob.size == want['bytes']
        assert hashlib.sha256(blob.tobytes()).hexdigest() == want['sha256'], (case[0], tag)
