"""CPU: the host half of the Aztec pass (lumina_ocr/utils/aztec.py): stuffed codewords -> bits -> text through every mode, latch and
shift, binary shifts, FLG(n), what is out of scope, the entries the provider reports, and the switches."""
import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.utils import aztec as az
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import layout

U, L, M, P, D = az.UPPER, az.LOWER, az.MIXED, az.PUNCT, az.DIGIT


def bits_of(*fields):
    """(value, width) ... -> bits"""
    return [(v >> (n - 1 - i)) & 1 for v, n in fields for i in range(n)]


def code(mode, name):
    return az.TABLES[mode].index(name), 4 if mode == D else 5


def row(compact, layers, words, box=(10, 20, 54, 64), errors=0, rotation=0):
    codes = np.array([box + (layers, int(compact), az.word_width(layers), len(words), errors, rotation, 0, 0)], np.int32)
    data = np.zeros((1, az.MAX_DATA), np.int32)
    data[0, :len(words)] = words
    return codes, data


def test_every_table_has_its_width_and_the_tables_are_the_recalled_ones():
    assert [len(t) for t in az.TABLES] == [32, 32, 32, 32, 16]
    assert az.TABLES[U][2] == "A" and az.TABLES[U][27] == "Z" and az.TABLES[U][28:] == ["LL", "ML", "DL", "BS"]
    assert az.TABLES[L][2] == "a" and az.TABLES[L][28:] == ["US", "ML", "DL", "BS"]
    assert az.TABLES[M][2] == "\x01" and az.TABLES[M][14] == "\r" and az.TABLES[M][20] == "@" and az.TABLES[M][27] == "\x7f" and az.TABLES[M][28:] == ["LL", "UL", "PL", "BS"]
    assert az.TABLES[P][:6] == ["FLG", "\r", "\r\n", ". ", ", ", ": "] and az.TABLES[P][6] == "!" and az.TABLES[P][30] == "}" and az.TABLES[P][31] == "UL"
    assert az.TABLES[D][2] == "0" and az.TABLES[D][11] == "9" and az.TABLES[D][12:] == [",", ".", "UL", "US"]


def test_every_mode_latch_and_shift():
    b = bits_of(code(U, "A"), code(U, "LL"), code(L, "b"), code(L, "US"), code(U, "C"), code(L, "d"),           # A b C d: US shifts one character
                code(L, "PS"), code(P, "!"), code(L, "e"),                                                        # PS shifts one character
                code(L, "ML"), code(M, "@"), code(M, "\t"), code(M, "PL"), code(P, ": "), code(P, "{"), code(P, "UL"),   # L -> M -> P -> U
                code(U, "DL"), code(D, "4"), code(D, "."), code(D, "US"), code(U, "Z"), code(D, "2"), code(D, "PS"), code(P, "\r\n"), code(D, "UL"),
                code(U, "ML"), code(M, "LL"), code(L, "z"), code(L, "ML"), code(M, "UL"), code(U, "Q"), code(U, " "))
    assert az.bits_text(b) == ("AbCd!e@\t: {4.Z2\r\nzQ ", None, False)
    # the encoder's own latches decode to what went in, through every pair of modes
    for text in ("Hello, World. 12345 AB", "a1B2c3;d\x1be@f", "12.5,A:b\t9{}", "\x01\x02abc\r\nDEF. X, Y: Z!", "Az\xe9\xff caf\xe9 99"):
        assert az.bits_text(az.content_bits(text)) == (text, None, False), text
    # a stream that ends inside a field ends there
    assert az.bits_text(bits_of(code(U, "A"), (1, 1), (1, 1), (1, 1))) == ("A", None, False)
    assert az.bits_text(bits_of(code(U, "A"), code(U, "BS"), (3, 4))) == ("A", None, False)


def test_binary_shift_short_and_long():
    short = bytes(range(200, 231))                                       # 31 bytes: the 5-bit length
    b = bits_of(code(U, "X"), code(U, "BS"), (31, 5), *[(v, 8) for v in short], code(U, "Y"))
    assert az.bits_text(b) == ("X" + short.decode("iso-8859-1") + "Y", None, False)
    long = bytes((7 * i) % 251 + 1 for i in range(70))                   # 70 bytes: 0, then 11 bits of 70 - 31
    b = bits_of(code(U, "LL"), code(L, "BS"), (0, 5), (39, 11), *[(v, 8) for v in long], code(L, "k"))
    text = az.bits_text(b)[0]
    assert text.encode("iso-8859-1") == long + b"k"
    assert az.bits_text(az.content_bits(long))[0].encode("iso-8859-1") == long
    w = az.BitWriter()
    w.text("12")
    w.binary(b"\x00\xfe")                                                # from Digit the writer goes to Upper first
    assert az.bits_text(w.bits)[0] == "12\x00\xfe"


def test_fnc1_first_and_later_and_eci():
    flg = lambda n: [code(U, "PS"), (0, 5), (n, 3)]
    b = bits_of(*flg(0), code(U, "A"), *flg(0), code(U, "B"))
    assert az.bits_text(b) == ("A\x1dB", None, True)
    b = bits_of(code(U, "A"), *flg(0), code(U, "B"))
    assert az.bits_text(b) == ("A\x1dB", None, False)
    assert az.bits_text(az.content_bits("0195", gs1=True)) == ("0195", None, True)
    utf = "Grüße € 5"
    assert az.bits_text(az.content_bits(utf, eci=26)) == (utf, None, False)
    assert az.bits_text(az.content_bits("caf\xe9", eci=3)) == ("caf\xe9", None, False)
    b = bits_of(*flg(2), (4, 4), (8, 4), code(U, "BS"), (2, 5), (0xC3, 8), (0xA9, 8))      # ECI 26, then two UTF-8 bytes
    assert az.bits_text(b) == ("\xe9", None, False)


def test_unsupported_reasons_and_invalid_words():
    flg = lambda n: [code(U, "PS"), (0, 5), (n, 3)]
    assert az.bits_text(bits_of(*flg(7), code(U, "A"))) == ("", "FLG(7)", False)
    assert az.bits_text(bits_of(*flg(1), (9, 4), code(U, "A"))) == ("", "ECI 7", False)
    assert az.bits_text(bits_of(*flg(6), *[(d + 2, 4) for d in (8, 9, 9, 9, 9, 9)], code(U, "A"))) == ("", "ECI 899999", False)
    assert az.bits_text(bits_of(*flg(1), (15, 4), code(U, "A"))) == (None, None, False)     # an ECI digit that is none
    assert az.bits_text(bits_of(code(U, "ML"), code(M, "UL"), code(U, "A"), code(U, " "), code(U, "B"))) == ("", "structured append", False)
    words = az.stuff_bits(bits_of(*flg(7), code(U, "A")), 6)
    un = az.read_aztec(*row(True, 1, words))
    assert len(un) == 1 and un[0]["content"] == "" and un[0]["unsupported"] == "FLG(7)"
    boxes = layout.build_barcode_boxes(un)
    assert boxes[0]["unsupported"] == "FLG(7)" and layout.validate_layout_boxes(boxes) == []
    for w in (6, 8, 10):
        for bad in (0, (1 << w) - 1, 1 << w):
            assert az.unstuff_words([5, bad, 9], w) is None and az.codewords_text([5, bad, 9], w) == (None, None, False)
        assert az.unstuff_words([1, (1 << w) - 2], w) == [0] * (w - 1) + [1] * (w - 1)
    assert az.read_aztec(*row(True, 1, [5, 0, 9])) == []
    # stuffing: runs of zeros and ones survive the round trip in every width
    rng = np.random.RandomState(5)
    for w in (6, 8, 10):
        bits = [0] * 23 + [1] * 29 + [int(v) for v in rng.randint(0, 2, 100)] + [0] * 12
        words = az.stuff_bits(bits, w)
        assert all(0 < v < (1 << w) - 1 for v in words)
        back = az.unstuff_words(words, w)
        assert back[:len(bits)] == bits and all(back[len(bits):]) and len(back) - len(bits) < w


def test_entries_polygon_confidence_and_markdown():
    words, nd = az.symbol_words("https://lumina.example/a?b=1", False, 2)
    codes, data = row(False, 2, words[:nd], box=(10, 20, 78, 88), errors=5, rotation=3)
    found = az.read_aztec(codes, data)
    assert len(found) == 1
    f = found[0]
    assert (f["kind"], f["content"], f["layers"], f["compact"], f["rotation"], f["errors"]) == ("Aztec", "https://lumina.example/a?b=1", 2, False, 270, 5)
    assert f["polygon"] == [10.0, 20.0, 79.0, 20.0, 79.0, 89.0, 10.0, 89.0] and f["box"] == (10, 20, 78, 88) and "gs1" not in f
    ec = az.total_words(False, 2) - nd
    assert f["confidence"] == 1.0 - 5.0 / (ec // 2) and az.confidence(10, 0) == 1.0 and az.confidence(10, 9) == 0.0
    boxes = layout.build_barcode_boxes(found, page_number=3)
    assert boxes == [{"type": "barcode", "kind": "Aztec", "content": "https://lumina.example/a?b=1", "confidence": f["confidence"], "polygon": f["polygon"],
                      "page_number": 3}]
    assert layout.validate_layout_boxes(boxes) == []
    assert layout.validate_layout_boxes([dict(boxes[0], kind="Aztek")]) != []
    merged, _ = layout.reading_order([([0, 0, 50, 0, 50, 10, 0, 10], "above", 0.9), ([0, 300, 50, 300, 50, 310, 0, 310], "below", 0.9)])
    assert layout.page_markdown(merged, barcodes=found).split("\n") == ["above", ":barcode: https://lumina.example/a?b=1", "below"]
    gs1 = az.read_aztec(*row(True, 2, az.symbol_words("0109501101530003", True, 2, gs1=True)[0][:az.symbol_words("0109501101530003", True, 2, gs1=True)[1]]))
    assert gs1[0]["gs1"] is True and gs1[0]["content"] == "0109501101530003" and layout.build_barcode_boxes(gs1)[0]["gs1"] is True
    # rows that are no symbol in scope are left out
    assert az.read_aztec(np.array([[0, 0, 9, 9, 5, 1, 8, 3, 0, 0, 0, 0]], np.int32), data) == []      # compact has four layers at most
    assert az.read_aztec(np.array([[0, 0, 9, 9, 12, 0, 10, 3, 0, 0, 0, 0]], np.int32), data) == []    # twelve layers are out of scope
    assert az.read_aztec(np.array([[0, 0, 9, 9, 2, 0, 8, 3, 0, 0, 0, 0]], np.int32), data) == []      # two layers have 6-bit words
    # 1-D codes first, then QR, Data Matrix, Aztec, through the one builder
    other = lambda kind: {"kind": kind, "content": "X", "confidence": 1.0, "polygon": [0.0] * 8, "box": (0, 0, 1, 1)}
    assert [b["kind"] for b in layout.build_barcode_boxes([other("Code128"), other("QRCode"), other("DataMatrix")] + found)] == ["Code128", "QRCode", "DataMatrix", "Aztec"]
    inside = [[20, 30], [60, 30], [60, 50], [20, 50]]
    assert bc.inside_any(inside, found) and not bc.inside_any([[200, 120], [300, 120], [300, 140], [200, 140]], found)


def test_the_provider_reads_its_switch_from_the_environment(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    for value, want in (("1", True), ("true", True), ("0", False), ("", False), (None, False)):
        if value is None:
            monkeypatch.delenv("LUMINA_OCR_AZTEC", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_AZTEC", value)
        s = object.__new__(svc.OCRService)           # beside the process's singleton
        s._initialized = False
        svc.OCRService.__init__(s)
        assert s._use_aztec is want and s.get_status()["aztec"] is want, value
        assert s._use_datamatrix is False and s._use_qrcodes is False


def test_the_pipeline_checks_its_arguments():
    from lumina_ocr.pipeline import OcrPipeline

    class Eng:
        num_classes, cls_loaded = 6625, False

    p = OcrPipeline(Eng(), aztec=True)
    assert p.aztec is True and p.aztec_params == arch.AZTEC_PARAMS and p.aztec_params is not arch.AZTEC_PARAMS
    assert OcrPipeline(Eng()).aztec is False
    assert OcrPipeline(Eng(), aztec=True, aztec_params=dict(arch.AZTEC_PARAMS, quiet=2)).aztec_params["quiet"] == 2
    with pytest.raises(ValueError, match="aztec_params"):
        OcrPipeline(Eng(), aztec=True, aztec_params=dict(arch.AZTEC_PARAMS, timing_max=3))
    assert set(arch.AZTEC_PARAMS) == {"threshold", "min_module", "max_module", "quiet", "centre_tol", "ring_tol", "mark_max", "max_finders", "max_codes"}
