"""CPU: the integer restatement of the strip decoders (tests/tiff_reference.py) equals Pillow / libtiff on every case of
tests/tiff_cases.py, its encoders round-trip, and every status rule of lumina_ocr_strip_image_decode is hit by a hand-made stream."""
import numpy as np
import pytest

import tiff_cases as tc
import tiff_reference as tr

C, E = tr.CLEAR, tr.EOI


@pytest.mark.parametrize("name", list(tc.strip_cases()))
def test_restatement_equals_pillow(name):
    c = tc.strip_cases()[name]
    status, rgb, strip_status, _ = tr.decode_page(c["strips"], c["height"], c["width"], c["rps"], c["params"], c["palette"])
    assert status == 0 and strip_status == [0] * len(c["strips"])
    assert np.array_equal(rgb, tc.pillow_rgb(c["file"]))


def test_noise_case_reaches_12_bits_and_a_table_full_clear():
    for name in ("lzw_noise_40x300_libtiff", "lzw_noise_40x300_own"):
        c = tc.strip_cases()[name]
        assert len(c["strips"]) == 1 and 15000 < len(c["strips"][0]) < 18000
        ctr = tr.lzw_decode(c["strips"][0], 40 * 300)[2]
        assert ctr["widest"] == 12 and ctr["clears"] >= 2


def test_encoders_round_trip():
    rng = np.random.default_rng(2)
    for data in (b"a", b"ab" * 700, bytes(5000), rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), rng.integers(0, 2, 40000, dtype=np.uint8).tobytes()):
        assert tr.lzw_decode(tr.lzw_encode(data), len(data))[:2] == (0, data)
        assert tr.lzw_decode(tr.lzw_encode(data, eoi=False), len(data))[:2] == (0, data)
        for eod in (False, True):
            assert tr.packbits_decode(tr.packbits_encode(data, eod), len(data), eod) == (0, data)


def lzw_status(codes, total):
    return tr.lzw_decode(tr.pack_codes(codes), total)[0]


def test_lzw_status_rules():
    assert lzw_status([(C, 9), (65, 9), (66, 9)], 2) == 0
    assert lzw_status([(C, 9), (65, 9), (66, 9), (E, 9), (300, 9)], 2) == 0          # codes after the last needed one are ignored
    assert lzw_status([(C, 9), (65, 9), (258, 9)], 3) == 0                            # KwKwK: A, AA
    assert tr.lzw_decode(tr.pack_codes([(C, 9), (65, 9), (258, 9), (259, 9)]), 6)[1] == b"AAAAAA"
    assert tr.lzw_decode(tr.pack_codes([(C, 9), (65, 9), (258, 9)]), 2)[1] == b"AA"   # clipped at the strip's end
    assert lzw_status([(65, 9), (66, 9)], 2) == -2                                    # the first code is not Clear
    assert tr.lzw_decode(b"\x00\x01" + bytes(30), 8)[0] == -2                         # old-style LZW (LSB first) starts 00 01
    assert lzw_status([(C, 9), (65, 9), (260, 9)], 8) == -1                           # a code above the next free entry
    assert lzw_status([(C, 9), (258, 9)], 8) == -1                                    # a code >= 258 right after Clear
    assert lzw_status([(C, 9), (65, 9), (C, 9), (300, 9)], 8) == -1
    assert lzw_status([(C, 9), (65, 9), (E, 9)], 2) == -1                             # EOI before the strip is full
    assert lzw_status([(C, 9), (E, 9)], 1) == -1
    assert lzw_status([(C, 9), (65, 9)], 2) == -1                                     # the data ends before the strip is full
    assert tr.lzw_decode(b"", 1)[0] == -1 and tr.lzw_decode(b"\x80", 1)[0] == -1
    assert tr.lzw_decode(b"\xff" * 64, 100)[0] == -2                                  # all ones
    assert lzw_status([(C, 9), (C, 9), (C, 9), (65, 9)], 1) == 0                      # Clear may repeat


def test_lzw_full_table_needs_clear():
    data = np.random.default_rng(5).integers(0, 256, 8000, dtype=np.uint8).tobytes()
    codes = tr.lzw_codes(data)
    k = [i for i, (c, _) in enumerate(codes) if c == C][1]    # the Clear the encoder sends when the table is full
    assert codes[k][1] == 12
    assert tr.lzw_decode(tr.pack_codes(codes), len(data))[:2] == (0, data)
    bad = codes[:k] + [(65, 12)] + codes[k + 1:]
    assert tr.lzw_decode(tr.pack_codes(bad), len(data))[0] == -1
    # the width rule: 9 bits up to entry 509, 10 from the code after entry 510 is made (early change)
    widths = [b for _, b in codes[:k + 1]]
    assert widths.index(10) == 1 + 1 + (511 - 258) and widths.index(11) == widths.index(10) + 512 and widths.index(12) == widths.index(11) + 1024


def test_packbits_status_rules():
    assert tr.packbits_decode(bytes([2, 1, 2, 3]), 3) == (0, b"\x01\x02\x03")
    assert tr.packbits_decode(bytes([254, 7]), 3) == (0, b"\x07\x07\x07")
    assert tr.packbits_decode(bytes([129, 7]), 128) == (0, b"\x07" * 128)
    assert tr.packbits_decode(bytes([254, 7]), 2) == (0, b"\x07\x07")                   # clipped at the strip's end
    assert tr.packbits_decode(bytes([128, 0, 9]), 1) == (0, b"\x09")                    # 128 is skipped in a TIFF
    assert tr.packbits_decode(bytes([128, 0, 9]), 1, eod=True)[0] == -1                 # and ends a /RunLengthDecode stream
    assert tr.packbits_decode(bytes([0, 9, 128]), 1, eod=True) == (0, b"\x09")
    assert tr.packbits_decode(bytes([2, 1, 2]), 3)[0] == -1                             # a literal past the input
    assert tr.packbits_decode(bytes([0, 1, 254]), 4)[0] == -1                           # a repeat at the last byte
    assert tr.packbits_decode(bytes([0, 1]), 2)[0] == -1 and tr.packbits_decode(b"", 1)[0] == -1


def test_raw_and_page_status():
    assert tr.decode_strip(b"abc", 3, tr.CODEC_NONE)[:2] == (0, b"abc") and tr.decode_strip(b"abcd", 3, tr.CODEC_NONE)[:2] == (0, b"abc")
    assert tr.decode_strip(b"ab", 3, tr.CODEC_NONE)[0] == -1
    good = tr.lzw_encode(bytes(8))
    p = (tr.CODEC_LZW, 1, 1, 8, 0, 0, 0)
    assert tr.decode_page([good, good], 2, 8, 1, p)[0] == 0
    assert tr.decode_page([good], 2, 8, 1, p)[0] == -2                                  # a wrong strip count
    assert tr.decode_page([good, good[:3]], 2, 8, 1, p)[0] == -1
    assert tr.decode_page([good[:3], b"\x00\x01\x02"], 2, 8, 1, p)[0] == -2             # the lowest of the strips
