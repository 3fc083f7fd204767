"""The host half of the QR pass (lumina_ocr/utils/qrcodes.py): data codewords -> text, the reasons for what is out of scope, the
provider's entries, their confidence and Markdown line, and the suppression of the lines the detector found inside a symbol."""
import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import layout
from lumina_ocr.utils import qrcodes as qr
from lumina_ocr.utils.ocr_postprocessor import TextBlock


def row(version, level, data, box=(10, 20, 93, 103), errors=0, rotation=0, mask=0):
    codes = np.array([box + (version, level, mask, len(data), errors, rotation, 0, 0)], np.int32)
    d = np.zeros((1, qr.MAX_DATA), np.int32)
    d[0, :len(data)] = data
    return codes, d


def test_segments_numeric_alphanumeric_byte_and_mixed():
    for version in (1, 9, 10):
        for data, want in (("0123456789012", "0123456789012"), ("7", "7"), ("42", "42"), ("HELLO WORLD $%*+-./:", "HELLO WORLD $%*+-./:"), ("A", "A"),
                           ("héllo wörld ✓", "héllo wörld ✓"), (["2024", "INV-", "ä/b"], "2024INV-ä/b"), ([b"\xe9t\xe9", "99"], "été99")):
            level = 0 if version == 1 else 2
            cw = synth.qr_data_codewords(data, version, level)
            assert len(cw) == qr.data_codewords(version, level)
            assert qr.codewords_text(version, cw) == (want, None), (version, data)


def test_count_widths_of_versions_one_to_nine_and_ten():
    assert [qr.count_bits(m, 9) for m in (1, 2, 4)] == [10, 9, 8] and [qr.count_bits(m, 10) for m in (1, 2, 4)] == [12, 11, 16]
    text = "WIDTHS 123"
    c9, c10 = synth.qr_data_codewords(text, 9, 3), synth.qr_data_codewords(text, 10, 3)
    assert c9[:8] != c10[:8]
    assert qr.codewords_text(9, c9) == (text, None) == qr.codewords_text(10, c10)
    assert qr.codewords_text(10, c9) != (text, None) and qr.codewords_text(9, c10) != (text, None)      # read at the other width: not the text


def test_terminator_shorter_than_four_bits_at_capacity():
    # 1-L holds 19 codewords = 152 bits; byte mode: 4 + 8 + 8 n -> n = 17 leaves 4 bits, so use numeric: 4 + 10 + 10 * 13 + 7 = 151 bits (41 digits): 1 bit left
    digits = "1234567890" * 4 + "1"
    assert len(synth.qr_segment_bits(digits, 1)) == 151
    cw = synth.qr_data_codewords(digits, 1, 0)
    assert len(cw) == 19 and qr.codewords_text(1, cw) == (digits, None)
    full = "abcdefghijklmnopq"                                           # byte mode, 4 + 8 + 8 * 17 = 148 bits: the whole four-bit terminator, no pad codeword
    assert len(synth.qr_segment_bits(full, 1)) == 148 and synth.qr_segment_bits(full, 1)[:4] == [0, 1, 0, 0]
    cw = synth.qr_data_codewords(full, 1, 0)
    assert len(cw) == 19 and cw[-1] & 15 == 0 and qr.codewords_text(1, cw) == (full, None)
    alnum = "ABCDEFGHIJKLMNOPQRSTUVWXY"                                  # 4 + 9 + 11 * 12 + 6 = 151 bits
    assert len(synth.qr_segment_bits(alnum, 1)) == 151 and qr.codewords_text(1, synth.qr_data_codewords(alnum, 1, 0)) == (alnum, None)


def test_eci_26_is_utf8_and_bytes_that_are_no_utf8_are_latin1():
    cw = synth.qr_data_codewords([("bits", 7, 4), ("bits", 26, 8), "grüß"], 2, 1)
    assert qr.codewords_text(2, cw) == ("grüß", None)
    assert qr.codewords_text(2, synth.qr_data_codewords(b"caf\xe9", 2, 1)) == ("café", None)


def test_unsupported_reasons():
    put = lambda *bits: synth.qr_data_codewords([("bits", v, k) for v, k in bits] + ["TAIL"], 2, 1)
    assert qr.codewords_text(2, put((8, 4), (1, 8), (0x1234 & 0x1FFF, 13))) == ("", "kanji")
    assert qr.codewords_text(2, put((3, 4), (0, 4), (1, 4), (0xAB, 8))) == ("", "structured append")
    assert qr.codewords_text(2, put((5, 4))) == ("", "FNC1") == qr.codewords_text(2, put((9, 4), (17, 8)))
    assert qr.codewords_text(2, put((7, 4), (3, 8))) == ("", "ECI 3")
    assert qr.codewords_text(2, put((7, 4), (0x80 | 1, 8), (44, 8))) == ("", "ECI 300")
    assert qr.codewords_text(2, put((6, 4))) == ("", "mode 6")


def test_a_bit_stream_that_runs_past_its_codewords_is_no_symbol():
    cw = synth.qr_data_codewords("0123456789", 1, 3)                     # 9 codewords
    assert qr.codewords_text(1, cw) == ("0123456789", None)
    cw[1] |= 0x3F                                                        # the count now asks for more digits than the symbol holds
    assert qr.codewords_text(1, cw) == (None, None)
    assert qr.read_qrcodes(*row(1, 3, cw)) == []
    assert qr.codewords_text(1, [0x40, 0xFF]) == (None, None) and qr.codewords_text(1, [0x10, 0x0F, 0xFF]) == (None, None)   # 999 > "3 digits" is no number


def test_entries_polygon_confidence_and_markdown():
    cw = synth.qr_data_codewords("https://lumina.example/a?b=1", 5, 2)
    codes, data = row(5, 2, cw, box=(10, 20, 157, 167), errors=9, rotation=3, mask=6)
    found = qr.read_qrcodes(codes, data)
    assert len(found) == 1
    f = found[0]
    assert (f["kind"], f["content"], f["version"], f["level"], f["mask"], f["rotation"], f["errors"]) == ("QRCode", "https://lumina.example/a?b=1", 5, "Q", 6, 270, 9)
    assert f["polygon"] == [10.0, 20.0, 158.0, 20.0, 158.0, 168.0, 10.0, 168.0] and f["box"] == (10, 20, 157, 167)        # TL, TR, BR, BL
    # confidence = 1 - errors / (blocks * floor(ec / 2)): 5-Q has four blocks of 18 check codewords
    assert qr.capacity_errors(5, 2) == 36 and f["confidence"] == 1.0 - 9 / 36.0
    assert qr.confidence(1, 0, 0) == 1.0 and qr.confidence(1, 0, 3) == 0.0 and qr.confidence(10, 3, 112) == 0.0
    boxes = layout.build_barcode_boxes(found, page_number=3)
    assert boxes == [{"type": "barcode", "kind": "QRCode", "content": "https://lumina.example/a?b=1", "confidence": 0.75, "polygon": f["polygon"],
                      "page_number": 3}]
    assert layout.validate_layout_boxes(boxes) == []
    merged, _ = layout.reading_order([([0, 0, 50, 0, 50, 10, 0, 10], "above", 0.9), ([0, 300, 50, 300, 50, 310, 0, 310], "below", 0.9)])
    assert layout.page_markdown(merged, barcodes=found).split("\n") == ["above", ":barcode: https://lumina.example/a?b=1", "below"]
    # out of scope: reported with the reason, content empty
    kanji = synth.qr_data_codewords([("bits", 8, 4), ("bits", 1, 8), ("bits", 0x0AAA, 13)], 1, 0)
    un = qr.read_qrcodes(*row(1, 0, kanji))
    assert len(un) == 1 and un[0]["content"] == "" and un[0]["unsupported"] == "kanji"
    assert layout.build_barcode_boxes(un)[0]["unsupported"] == "kanji" and layout.validate_layout_boxes(layout.build_barcode_boxes(un)) == []
    # 1-D codes first, then the QR symbols, through the one builder
    strip = {"kind": "Code128", "content": "X", "confidence": 1.0, "polygon": [0.0] * 8, "box": (0, 0, 1, 1)}
    assert [b["kind"] for b in layout.build_barcode_boxes([strip] + found)] == ["Code128", "QRCode"]


def test_lines_inside_a_symbol_are_dropped():
    found = qr.read_qrcodes(*row(1, 1, synth.qr_data_codewords("X", 1, 1), box=(100, 100, 183, 183)))
    inside = [[110, 120], [170, 120], [170, 140], [110, 140]]
    outside = [[200, 120], [300, 120], [300, 140], [200, 140]]
    assert bc.inside_any(inside, found) and not bc.inside_any(outside, found)
    assert bc.inside_any([v for p in inside for v in p], found)
