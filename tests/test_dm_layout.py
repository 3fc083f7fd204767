"""The host half of the Data Matrix pass (lumina_ocr/utils/datamatrix.py): data codewords -> text in each of the six encodation
schemes, the macros, GS1, the reasons for what is out of scope, the provider's entries, their confidence and Markdown line, the
suppression of the lines the detector found inside a symbol, and the provider's switch."""
import numpy as np
import pytest

from lumina_ocr import synth
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import datamatrix as dm
from lumina_ocr.utils import layout

S16, S26 = dm.size_index(16, 16), dm.size_index(26, 26)


def row(size, data, box=(10, 20, 93, 103), errors=0, rotation=0):
    codes = np.array([box + (dm.SIZES[size][0], dm.SIZES[size][1], len(data), errors, rotation, 0, 0, 0)], np.int32)
    d = np.zeros((1, dm.MAX_DATA), np.int32)
    d[0, :len(data)] = data
    return codes, d


def text_of(data, size, scheme="ascii"):
    cw = synth.dm_data_codewords(data, size, scheme)
    assert len(cw) == dm.SIZES[size][2]
    return dm.codewords_text(cw)


def test_ascii_digit_pairs_upper_shift_and_pads():
    assert synth.dm_data_codewords("A1", 0) == [66, 50, 129] and synth.dm_data_codewords("00990", 0) == [130, 229, 49]
    assert synth.dm_data_codewords(b"\xe9", 0) == [235, 0xE9 - 127, 129]
    for data, want in (("Hello, World", "Hello, World"), ("0123456789012", "0123456789012"), ("7", "7"), ("café ✓", "café ✓"), (b"caf\xe9", "café"),
                       ("\x00\x7f~", "\x00\x7f~")):
        assert text_of(data, S26) == (want, None), data
    # the pads behind the first are randomised by their position and never read as data
    cw = synth.dm_data_codewords("AB", S16)
    assert cw[:3] == [66, 67, 129] and cw[3:] == [dm.randomised_pad(k) for k in range(4, 13)] and len(set(cw[3:])) > 4
    assert all(1 <= v <= 254 for v in cw) and dm.codewords_text(cw) == ("AB", None)
    assert text_of("ABCDEFGHIJKL", S16) == ("ABCDEFGHIJKL", None)                   # no pad at all


def test_c40_and_text_shifts_unlatch_and_end_of_data():
    mixed = "AB12 cd{~}\x01_!éZ"
    for scheme in ("c40", "text"):
        assert text_of(mixed, S26, scheme) == (mixed, None), scheme
    assert synth.dm_data_codewords("ABC", 0, "c40")[0] == dm.LATCH_C40 and synth.dm_data_codewords("abc", 0, "text")[0] == dm.LATCH_TEXT
    # "ABC" in 10 x 10: latch + one pair fill the symbol: no unlatch
    assert synth.dm_data_codewords("ABC", 0, "c40") == [230, (1600 * 14 + 40 * 15 + 16 + 1) >> 8, (1600 * 14 + 40 * 15 + 16 + 1) & 255]
    assert text_of("ABC", 0, "c40") == ("ABC", None)
    # room left: unlatch, then the pad
    cw = synth.dm_data_codewords("ABC", 1, "c40")
    assert cw[3:] == [254, 129] and dm.codewords_text(cw) == ("ABC", None)
    # one character and one codeword left: ASCII without an unlatch (14 x 14 holds 8: latch, three pairs, J)
    cw = synth.dm_data_codewords("ABCDEFGHIJ", dm.size_index(14, 14), "c40")
    assert len(cw) == 8 and 254 not in cw and cw[7] == ord("J") + 1 and dm.codewords_text(cw) == ("ABCDEFGHIJ", None)
    # one character left and more room than that: unlatch first (12 x 12 holds 5)
    cw = synth.dm_data_codewords("ABCD", 1, "c40")
    assert cw == [230, cw[1], cw[2], 254, ord("D") + 1] and dm.codewords_text(cw) == ("ABCD", None)
    # two values left over go to ASCII behind an unlatch
    cw = synth.dm_data_codewords("ABCDE", S16, "c40")
    assert cw[:4] == [230, cw[1], cw[2], 254] and cw[4:6] == [ord("D") + 1, ord("E") + 1] and dm.codewords_text(cw) == ("ABCDE", None)
    # a value that is of no set is no symbol
    assert dm.codewords_text([230, 0xFF, 0xFF, 129]) == (None, None)
    # FNC1 in shift set 2 is GS
    v = 1600 * 1 + 40 * 27 + 14 + 1
    assert dm.codewords_text([230, v >> 8, v & 255, 254]) == ("\x1dA", None)


def test_x12_and_edifact():
    assert text_of("AB*12>CD \r9", S26, "x12") == ("AB*12>CD \r9", None)
    with pytest.raises(ValueError):
        synth.dm_data_codewords("lower", S26, "x12")
    for n in range(1, 10):                                                           # every position of the unlatch in its triple
        text = "EDI-FACT."[:n]
        assert text_of(text, S26, "edifact") == (text, None), n
    cw = synth.dm_data_codewords("ABCD", S26, "edifact")
    assert cw[0] == dm.LATCH_EDIFACT and cw[4] >> 2 == 0x1F and cw[5] == 129         # the unlatch, then ASCII from the next byte on
    assert synth.dm_data_codewords("ABCD", 1, "edifact")[:4] == cw[:4]               # 12 x 12: five codewords, one left for the unlatch
    text = "EDIFACT FILLS THE SYMBOL 22."                                          # 28 characters = 21 codewords behind the latch: 20 x 20 is full
    cw = synth.dm_data_codewords(text, dm.size_index(20, 20), "edifact")
    assert len(text) == 28 and len(cw) == 22 and dm.codewords_text(cw) == (text, None)
    assert dm.codewords_text(synth.dm_data_codewords(text, S26, "edifact")) == (text, None)       # the same with room: unlatch and pads
    cw = synth.dm_data_codewords([("edifact", "ABCD"), "9"], S16)                    # ASCII goes on behind the unlatch
    assert dm.codewords_text(cw) == ("ABCD9", None)
    assert dm.codewords_text([240, 0x04, 0x20, 0xC4, 66, 67]) == ("ABCDAB", None)    # at most two codewords left: they are ASCII, no unlatch
    with pytest.raises(ValueError):
        synth.dm_data_codewords("lower", S26, "edifact")


def test_base256_both_length_forms_and_randomisation():
    raw = bytes(range(200, 230))
    cw = synth.dm_data_codewords(raw, S26, "base256")
    assert cw[0] == 231 and dm.unrandomise_255(cw[1], 2) == 30 and [dm.unrandomise_255(v, i + 3) for i, v in enumerate(cw[2:32])] == list(raw)
    assert cw[2:32] != list(raw) and cw[32] == 129
    assert dm.codewords_text(cw) == (raw.decode("iso-8859-1"), None)
    fills = bytes(range(65, 65 + 42))                                                # 44 codewords: latch, length 0 = "to the end", 42 bytes
    cw = synth.dm_data_codewords(fills, S26, "base256")
    assert len(cw) == 44 and dm.unrandomise_255(cw[1], 2) == 0 and dm.codewords_text(cw) == (fills.decode(), None)
    # the two-byte length (250 and more) is beyond every size in scope; codewords_text reads it all the same
    n = 300
    body = [249 + n // 250, n % 250] + [65 + k % 26 for k in range(n)]
    long = [231] + [(v + (149 * (i + 2)) % 255 + 1) % 256 for i, v in enumerate(body)]
    assert dm.codewords_text(long) == ("".join(chr(65 + k % 26) for k in range(n)), None)
    assert dm.codewords_text([231, (40 + (149 * 2) % 255 + 1) % 256, 1, 2]) == (None, None)      # the length runs past the codewords
    assert text_of("grüß", S16, "base256") == ("grüß", None)                 # UTF-8 bytes


def test_macros_gs1_and_mixed_parts():
    assert dm.codewords_text(synth.dm_data_codewords([[236], "PAYLOAD"], S16)) == ("[)>\x1e05\x1dPAYLOAD\x1e\x04", None)
    assert dm.codewords_text(synth.dm_data_codewords([[237], "PAYLOAD"], S16)) == ("[)>\x1e06\x1dPAYLOAD\x1e\x04", None)
    assert dm.codewords_text([66, 236, 129]) == (None, None)                         # a macro anywhere else is no symbol
    gs1 = synth.dm_data_codewords([[232], "0109501101530003", "10AB", [232], "21X"], S26)
    assert dm.is_gs1(gs1) and dm.codewords_text(gs1) == ("010950110153000310AB\x1d21X", None)
    assert not dm.is_gs1(synth.dm_data_codewords("0109501101530003", S26))
    found = dm.read_datamatrix(*row(S26, gs1))
    assert found[0]["gs1"] is True and layout.build_barcode_boxes(found)[0]["gs1"] is True
    mixed = synth.dm_data_codewords(["ID ", ("c40", "ABC"), ("base256", b"\x00\x01"), "99"], S26)
    assert dm.codewords_text(mixed) == ("ID ABC\x00\x0199", None)


def test_unsupported_reasons_and_invalid_codewords():
    tail = [66, 67, 129]
    assert dm.codewords_text([233, 0x12, 1, 1] + tail) == ("", "structured append")
    assert dm.codewords_text([234] + tail) == ("", "reader programming")
    assert dm.codewords_text([241, 27] + tail) == ("", "ECI")
    un = dm.read_datamatrix(*row(S16, synth.dm_data_codewords([[241, 27], "AB"], S16)))
    assert len(un) == 1 and un[0]["content"] == "" and un[0]["unsupported"] == "ECI"
    assert layout.build_barcode_boxes(un)[0]["unsupported"] == "ECI" and layout.validate_layout_boxes(layout.build_barcode_boxes(un)) == []
    for bad in (242, 250, 255):
        assert dm.codewords_text([66, bad, 129]) == (None, None)
    assert dm.read_datamatrix(*row(0, [66, 250, 129])) == []
    assert dm.codewords_text([231]) == (None, None)


def test_entries_polygon_confidence_and_markdown():
    cw = synth.dm_data_codewords("https://lumina.example/a?b=1", S26)
    codes, data = row(S26, cw, box=(10, 20, 113, 123), errors=7, rotation=3)
    found = dm.read_datamatrix(codes, data)
    assert len(found) == 1
    f = found[0]
    assert (f["kind"], f["content"], f["rows"], f["cols"], f["rotation"], f["errors"]) == ("DataMatrix", "https://lumina.example/a?b=1", 26, 26, 270, 7)
    assert f["polygon"] == [10.0, 20.0, 114.0, 20.0, 114.0, 124.0, 10.0, 124.0] and f["box"] == (10, 20, 113, 123) and "gs1" not in f
    assert dm.capacity_errors(S26) == 14 and f["confidence"] == 0.5 and dm.capacity_errors(dm.size_index(52, 52)) == 42
    assert dm.confidence(0, 0) == 1.0 and dm.confidence(0, 2) == 0.0
    boxes = layout.build_barcode_boxes(found, page_number=3)
    assert boxes == [{"type": "barcode", "kind": "DataMatrix", "content": "https://lumina.example/a?b=1", "confidence": 0.5, "polygon": f["polygon"],
                      "page_number": 3}]
    assert layout.validate_layout_boxes(boxes) == []
    merged, _ = layout.reading_order([([0, 0, 50, 0, 50, 10, 0, 10], "above", 0.9), ([0, 300, 50, 300, 50, 310, 0, 310], "below", 0.9)])
    assert layout.page_markdown(merged, barcodes=found).split("\n") == ["above", ":barcode: https://lumina.example/a?b=1", "below"]
    # rows that are no size of the table, or whose ndata is not the size's, are left out
    assert dm.read_datamatrix(np.array([[0, 0, 9, 9, 11, 11, 3, 0, 0, 0, 0, 0]], np.int32), data) == []
    assert dm.read_datamatrix(np.array([[0, 0, 9, 9, 10, 10, 4, 0, 0, 0, 0, 0]], np.int32), data) == []
    # 1-D codes first, then QR, then Data Matrix, through the one builder
    strip = {"kind": "Code128", "content": "X", "confidence": 1.0, "polygon": [0.0] * 8, "box": (0, 0, 1, 1)}
    square = {"kind": "QRCode", "content": "Y", "confidence": 1.0, "polygon": [0.0] * 8, "box": (0, 0, 1, 1)}
    assert [b["kind"] for b in layout.build_barcode_boxes([strip, square] + found)] == ["Code128", "QRCode", "DataMatrix"]


def test_lines_inside_a_symbol_are_dropped():
    found = dm.read_datamatrix(*row(0, synth.dm_data_codewords("X", 0), box=(100, 100, 183, 183)))
    inside = [[110, 120], [170, 120], [170, 140], [110, 140]]
    outside = [[200, 120], [300, 120], [300, 140], [200, 140]]
    assert bc.inside_any(inside, found) and not bc.inside_any(outside, found)
    assert bc.inside_any([v for p in inside for v in p], found)


def test_the_provider_reads_its_switch_from_the_environment(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    for value, want in (("1", True), ("true", True), ("0", False), ("", False), (None, False)):
        if value is None:
            monkeypatch.delenv("LUMINA_OCR_DATAMATRIX", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_DATAMATRIX", value)
        s = object.__new__(svc.OCRService)           # beside the process's singleton
        s._initialized = False
        svc.OCRService.__init__(s)
        assert s._use_datamatrix is want and s.get_status()["datamatrix"] is want, value


def test_encoder_and_matrix_round_trip_every_size():
    for s in range(dm.NUM_SIZES):
        cw = synth.dm_interleave(synth.dm_data_codewords("7", s), s)
        m = synth.dm_matrix(cw, s)
        assert m.shape == dm.SIZES[s][:2] and m[:, 0].all() and m[-1].all() and not m[0, -1]
        place = dm.placement_of(s)
        back = [sum(int(m[place[8 * k + b]]) << (7 - b) for b in range(8)) for k in range(len(cw))]
        assert back == cw
