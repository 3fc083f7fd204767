"""CPU: the Group 4 restatement (tests/ccitt_reference.py) against source bitmaps.  libtiff (through Pillow) is the encoder; the restatement
was written from the recommendation's tables as a decoder, so agreement on these cases checks both the tables and the walk."""
import numpy as np
import pytest
from PIL import features

import ccitt_cases as cc
import ccitt_reference as cr

needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the Group 4 encoder of these cases")


@pytest.fixture(scope="module")
def encoded():
    return {name: (bm, cc.g4_encode(bm)) for name, bm in cc.bitmaps().items()}


def test_tables_are_prefix_free_and_complete_enough():
    # lookup_table asserts prefix-freeness while it builds; the all-zero prefix belongs to no run or mode code (EOL starts with it)
    assert cr.WHITE_TABLE[0] == 0 and cr.BLACK_TABLE[0] == 0 and cr.MODE_TABLE[0] == 0
    for white in (True, False):
        runs = sorted(r for _, r in cr.run_codes(white))
        assert runs == list(range(64)) + list(range(64, 2561, 64))
    assert (cr.WHITE_TABLE >> 12).max() == 12 and (cr.BLACK_TABLE >> 12).max() == 13 and (cr.MODE_TABLE >> 12).max() == 7


@needs_libtiff
@pytest.mark.parametrize("name", sorted(cc.bitmaps()))
@pytest.mark.parametrize("black_is_1", [False, True])
def test_restatement_equals_source(encoded, name, black_is_1):
    bm, stream = encoded[name]
    status, bits = cr.decode(stream, bm.shape[1], bm.shape[0], black_is_1)
    assert status == 0
    assert np.array_equal(bits, cc.expected_bits(bm, black_is_1))


@needs_libtiff
@pytest.mark.parametrize("name", ["rand_65x40", "text_640x200", "extended_2700x4", "rand_1x5"])
def test_with_and_without_eofb_and_trailing_bytes(encoded, name):
    bm, stream = encoded[name]
    h, w = bm.shape
    status, bits, used = cr.decode_ex(stream, w, h)
    assert status == 0
    tail = int.from_bytes(stream, "big") >> (len(stream) * 8 - used - 24) & 0xFFFFFF
    assert tail == cr.EOFB, "libtiff ends the strip with EOFB"
    cut = stream[:(used + 7) // 8]   # the lines only
    for s in (cut, stream + b"\x00\x01II*\x00junk after the data", cut + b"\xff" * 9):
        st, got = cr.decode(s, w, h)
        assert st == 0 and np.array_equal(got, bits)


@needs_libtiff
def test_rows_and_eofb(encoded):
    bm, stream = encoded["rand_65x40"]
    # fewer rows wanted than coded: stop after them
    st, got = cr.decode(stream, 65, 25)
    assert st == 0 and np.array_equal(got, cc.expected_bits(bm[:25], False))
    # more rows wanted than coded before EOFB / the end of the stream: corrupt
    assert cr.decode(stream, 65, 41)[0] == -1
    used = cr.decode_ex(stream, 65, 40)[2]
    assert cr.decode(stream[:(used + 7) // 8], 65, 41)[0] == -1


@needs_libtiff
def test_hostile_streams_end_with_minus_one(encoded):
    bm, stream = encoded["text_640x200"]
    assert cr.decode(stream[:len(stream) // 2], 640, 200)[0] == -1
    assert cr.decode(b"", 640, 200)[0] == -1
    assert cr.decode(b"\x00" * 64, 640, 200)[0] == -1
    rng = np.random.default_rng(99)
    for _ in range(20):
        junk = rng.integers(0, 256, 2048, dtype=np.uint8).tobytes()
        st, _ = cr.decode(junk, 640, 200)
        assert st in (0, -1)
    # H mode with two zero runs over and over: a0 does not advance
    zero_runs = "001" + cr.WHITE_TERM[0] + cr.BLACK_TERM[0]
    bits = zero_runs * 40
    data = int(bits, 2).to_bytes((len(bits) + 7) // 8, "big") if len(bits) % 8 == 0 else int(bits + "0" * (8 - len(bits) % 8), 2).to_bytes(len(bits) // 8 + 1, "big")
    assert cr.decode(data, 64, 4)[0] == -1


def test_fixtures_match_their_digests():
    """the committed streams decode to the committed digests (no libtiff needed)"""
    fx = cc.fixtures()
    assert sorted(fx) == sorted(cc.FIXTURES)
    for name, (stream, w, h, digests) in fx.items():
        assert len(stream) < 8192
        for black_is_1 in (False, True):
            st, bits = cr.decode(stream, w, h, black_is_1)
            assert st == 0 and cc.sha(bits) == digests[black_is_1], name
