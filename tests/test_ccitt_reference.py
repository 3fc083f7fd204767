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


# ---- libtiff as a second decoder: the restatement shares its design with the kernel, libtiff shares nothing with either ----
@needs_libtiff
def test_libtiff_decode_equals_restatement_on_fixtures():
    for name, (stream, w, h, _) in cc.fixtures().items():
        st, bits = cr.decode(stream, w, h)
        assert st == 0 and np.array_equal(cc.libtiff_bits(stream, w, h), bits), name


def test_pass_code_at_the_line_end_is_corrupt():
    """rand_65x40 with bit 5230 or 5309 flipped ends row 39 with a pass code whose b1 = b2 = 65 = columns (a0 = 63).  T.6
    identifies pass mode "when the position of b2 lies to the left of a1", and a1 <= columns: the stream is non-conforming, and libtiff
    reads the two pixels as white where a decoder that takes the code paints them black."""
    stream, w, h, _ = cc.fixtures()["rand_65x40"]
    for bit in (5230, 5309):
        assert cr.decode(cc.flip_bit(stream, bit), w, h)[0] == -1, bit
    # the shortest such stream: one white line by a pass code alone
    assert cr.decode(cc.bits_to_bytes("0001"), 8, 1)[0] == -1
    assert cr.decode(cc.bits_to_bytes("1"), 8, 1)[0] == 0   # V0 against the imaginary line: the legal coding


# Streams the restatement accepts and libtiff reads differently, where the restatement is right by T.6: (file, label), with the clause.
# At most two may ever stand here.
SWEEP_EXCEPTIONS = ()


@needs_libtiff
def test_damage_sweep_accepted_streams_equal_libtiff():
    """every damaged stream of cc.damage_sweep that the restatement accepts must decode in libtiff to the same picture.  Measured: the
    restatement accepts 92 of 1602 (begins_black_65x12: 89 flips, 3 cuts), 62 of 1691 (rand_65x40) and 28 of 153 (rand_7x9); libtiff
    confirms all 182.  Before a pass code with b2 = columns became -1, bits 5230 and 5309 of rand_65x40 were accepted and differed."""
    assert len(SWEEP_EXCEPTIONS) <= 2
    accepted, differ = {}, []
    for name in cc.SWEEP_FILES:
        stream, w, h, damaged = cc.damage_sweep(name)
        assert cr.decode(stream, w, h)[0] == 0
        accepted[name] = 0
        for (label, d), (st, bits) in zip(damaged, cc.sweep_restatement(name)):
            if st != 0:
                continue
            accepted[name] += 1
            lib = cc.libtiff_bits(d, w, h)
            if (lib is None or not np.array_equal(lib, bits)) and (name, label) not in SWEEP_EXCEPTIONS:
                differ.append((name, label))
    print("accepted by the restatement:", accepted)
    assert differ == []
    assert sum(accepted.values()) >= 80 and accepted["begins_black_65x12"] >= 80, accepted   # never pass with nothing to compare


# ---- the second encoder: legal codings that libtiff's encoder never writes ----
@needs_libtiff
def test_policy_encoder_without_forced_horizontal_equals_libtiff(encoded):
    """p_horiz = 0 is the plain T.6 procedure, which is libtiff's too: the streams are the same, bit for bit, EOFB included"""
    same = [name for name, (bm, stream) in encoded.items() if cc.g4_encode_policy(bm, np.random.default_rng(0), 0.0) == stream]
    assert len(same) >= 15 and {"rand_65x40", "text_640x200", "extended_2700x4", "begins_black_65x12", "checker_65x20"} <= set(same)


@needs_libtiff
@pytest.mark.parametrize("p_horiz", [0.0, 0.3, 1.0])
def test_policy_encoder_round_trips_through_libtiff_and_restatement(p_horiz):
    cases = {**cc.bitmaps(), **cc.policy_bitmaps()}
    cases["exact_fit"], exact = cc.exact_fit_stream(p_horiz)
    for name, bm in cases.items():
        h, w = bm.shape
        want = cc.expected_bits(bm, False)
        for eofb in (True, False):
            stats = {}
            stream = exact if name == "exact_fit" and not eofb else cc.g4_encode_policy(bm, np.random.default_rng(5), p_horiz, eofb, stats)
            assert np.array_equal(cc.libtiff_bits(stream, w, h), want), (name, eofb)
            st, bits = cr.decode(stream, w, h)
            assert st == 0 and np.array_equal(bits, want), (name, eofb)
            if p_horiz == 1.0 and stats:
                assert stats["vertical"] == 0 and stats["horizontal"] > 0, (name, stats)
    # the exact-fit stream really ends on its last bit: the lines use every bit of it
    bm = cases["exact_fit"]
    assert cr.decode_ex(exact, bm.shape[1], bm.shape[0])[2] == 8 * len(exact)


def test_policy_encoder_long_runs_and_full_lines():
    """8192 black pixels are three 2560 make-ups, the 512 make-up and a zero terminating code; a line of `columns` changing elements
    that ends in horizontal mode is legal (its last pair lies at the line's end and is no changing element) and decodes"""
    maps = cc.policy_bitmaps()
    bits = cc.g4_encode_policy_bits(maps["black_8192_over_white"][:1], np.random.default_rng(0), 0.0)
    ext, black = dict((r, c) for c, r in cr.run_codes(False)), cr.BLACK_TERM
    assert bits == "001" + cr.WHITE_TERM[0] + ext[2560] * 3 + ext[512] + black[0]
    alt = maps["alternating_8192"]
    stats = {}
    stream = cc.g4_encode_policy(alt[:2], np.random.default_rng(0), 1.0, True, stats)
    st, got = cr.decode(stream, 8192, 2)
    assert st == 0 and np.array_equal(got, cc.expected_bits(alt[:2], False))
    # columns = 1, one black pixel: VL1 (a1 = 0 under b1 = 1), then the pair (1 black, 0 white) in horizontal mode
    st, got = cr.decode(cc.bits_to_bytes("010" + "001" + black[1] + cr.WHITE_TERM[0]), 1, 1)
    assert st == 0 and np.array_equal(got, [[0]])
