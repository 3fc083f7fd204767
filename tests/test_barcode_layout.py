"""The host half of the barcodes (lumina_ocr/utils/barcodes.py, utils/layout.py): symbols to text, the `barcode` entries and their
schema, the `:barcode:` line of the Markdown at its place, and the lines on a code that leave the output."""
import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import layout


def test_code128_symbols_to_text():
    assert bc.code128_text([104, 40, 69, 76, 76, 79, 0, 55, 79, 82, 76, 68, 43, 106]) == "Hello World"
    assert bc.code128_text([105, 12, 34, 56, 78, 47, 106]) == "12345678"
    assert bc.code128_text([103, 33, 34, 65, 100, 67, 68, 0, 106]) == "AB\x01cd"                    # set A, CODE B
    assert bc.code128_text([104, 65, 98, 65, 66, 0, 106]) == "a\x01b"                               # SHIFT: one character of set A
    assert bc.code128_text([103, 33, 98, 65, 34, 0, 106]) == "AaB"                                  # SHIFT from A to B
    assert bc.code128_text([104, 33, 99, 12, 34, 100, 34, 0, 106]) == "A1234B"                      # CODE C and back
    assert bc.code128_text([105, 102, 12, 101, 65, 0, 106]) == "12\x01"                             # FNC1 dropped; C -> A
    assert bc.code128_text([104, 102, 96, 97, 100, 33, 0, 106]) == "A"                              # FNC1-4 of set B dropped
    assert bc.code128_text([103, 101, 33, 0, 106]) == "A"                                           # FNC4 of set A dropped
    assert bc.code128_text([104, 33, 0]) is None and bc.code128_text([33, 0, 106]) is None and bc.code128_text([104, 103, 0, 106]) is None


def test_code39_symbols_to_text():
    assert bc.code39_text([43, 10, 11, 36, 1, 2, 38, 39, 42, 43]) == "AB-12 $%"
    assert bc.code39_text([43, 43]) == "" and bc.code39_text([43, 10]) is None and bc.code39_text([43, 43, 43]) is None


def _rows(*codes):
    rows = np.array([c[0] for c in codes], np.int32).reshape(-1, 8)
    syms = np.zeros((len(codes), 64), np.int32)
    for i, c in enumerate(codes):
        syms[i, :len(c[1])] = c[1]
    return rows, syms


def test_entries_schema_and_validator():
    s1, s2 = synth.code128_symbols("INV-2024"), synth.code39_symbols("LOT 7")
    rows, syms = _rows(((100, 200, 299, 249, 0, len(s1), 40, 0), s1), ((400, 100, 429, 399, 1, len(s2), 30, 3), s2))
    found = bc.read_barcodes(rows, syms)
    assert [(f["kind"], f["content"], f["reversed"], f["vertical"]) for f in found] == [("Code128", "INV-2024", False, False), ("Code39", "LOT 7", True, True)]
    assert found[0]["confidence"] == 40 / 50 and found[1]["confidence"] == 1.0                      # rows / extent across the bars
    assert found[0]["polygon"] == [100.0, 200.0, 300.0, 200.0, 300.0, 250.0, 100.0, 250.0]
    boxes = layout.build_barcode_boxes(found, 2)
    assert boxes[0] == {"type": "barcode", "kind": "Code128", "content": "INV-2024", "confidence": 0.8, "polygon": found[0]["polygon"], "page_number": 2}
    assert layout.validate_layout_boxes(boxes) == []
    assert layout.validate_layout_boxes([dict(boxes[0], kind="QR")]) != [] and layout.validate_layout_boxes([dict(boxes[0], content=5)]) != []
    assert layout.validate_layout_boxes([dict(boxes[0], confidence=2.0)]) != []
    # a row whose symbols are no message is left out
    assert bc.read_barcodes(*_rows(((0, 0, 9, 9, 0, 4, 9, 0), [104, 103, 0, 106]))) == []


def _line(x0, y0, x1, y1, text):
    return ([x0, y0, x1, y0, x1, y1, x0, y1], text, 0.9)


def test_markdown_line_at_the_barcodes_place_and_off_is_unchanged():
    lines = [_line(50, 20, 400, 50, "Invoice 17"), _line(50, 300, 400, 330, "Total 12.00"), _line(50, 400, 300, 430, "Thanks")]
    merged, ordered = layout.reading_order(lines)
    s = synth.code128_symbols("INV-17")
    found = bc.read_barcodes(*_rows(((60, 100, 300, 160, 0, len(s), 61, 0), s)))
    plain = layout.page_markdown(merged)
    assert plain == "Invoice 17\nTotal 12.00\nThanks"
    assert layout.page_markdown(merged, barcodes=found) == "Invoice 17\n:barcode: INV-17\nTotal 12.00\nThanks"
    assert layout.page_markdown(merged, barcodes=None) == plain and layout.page_markdown(merged, barcodes=[]) == plain
    assert layout.page_markdown(merged, None, None) == plain
    below = bc.read_barcodes(*_rows(((60, 500, 300, 560, 0, len(s), 61, 0), s)))
    assert layout.page_markdown(merged, barcodes=below).endswith("Thanks\n:barcode: INV-17")
    assert [m.text for m in merged] == ["Invoice 17", "Total 12.00", "Thanks"]                      # the caller's lines are not touched


def test_lines_on_a_code_are_dropped():
    s = synth.code128_symbols("X")
    found = bc.read_barcodes(*_rows(((60, 100, 300, 160, 0, len(s), 61, 0), s)))
    on_it, beside, above = _line(70, 110, 290, 150, "||I1l|"), _line(320, 110, 500, 150, "SKU"), _line(60, 40, 300, 90, "Ship to")
    assert [bc.inside_any(t[0], found) for t in (on_it, beside, above)] == [True, False, False]
    assert bc.inside_any([[70, 110], [290, 110], [290, 150], [70, 150]], found)                     # four points as well as eight numbers
    assert not bc.inside_any(on_it[0], [])
