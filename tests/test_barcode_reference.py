"""The restatement of the barcode pass (tests/barcode_reference.py) against ground truth: what was rendered is what is read, and what
is no barcode reads as none."""
import numpy as np
import pytest

from lumina_ocr import arch, synth

import barcode_reference as br

P = arch.BARCODE_PARAMS


def blank(h, w):
    return np.full((h, w, 3), 255, np.uint8)


def read(page):
    _, rc, rs = br.barcodes(page)
    return {tuple(int(v) for v in c[:4]): (t, int(c[4]), int(c[7])) for c, t in zip(rc, br.decoded(rc, rs))}


def put(page, x, y, text, kind="Code128", m=2, height=12, **kw):
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    return synth.render_barcode(page, x, y, syms, kind, m, height, **kw)


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("text,kind,start", [("Code 128-B text", "Code128", 104), ("0123456789", "Code128", 105), ("aB\x01c12345\x02\x03", "Code128", 104),
                                             ("CODE-39 $/+%.", "Code39", 43)])
def test_what_is_rendered_is_read(m, text, kind, start):
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    assert syms[0] == start
    page = blank(20, synth.barcode_length(syms, kind, m) + 40)
    box = put(page, 17, 4, text, kind, m=m)
    assert read(page) == {box: (text, int(kind == "Code39"), 0)}


def test_mixed_sets_use_a_shift():
    syms = synth.code128_symbols("aB\x01c12345\x02\x03")
    assert 98 in syms and 99 in syms and 101 in syms       # SHIFT, CODE C, CODE A


@pytest.mark.parametrize("kind", ["Code128", "Code39"])
def test_reversed_and_vertical(kind):
    page = blank(330, 330)
    want = {put(page, 20, 10, "REV-1", kind, reversed=True): ("REV-1", int(kind == "Code39"), 1),
            put(page, 10, 40, "VERT", kind, vertical=True): ("VERT", int(kind == "Code39"), 2),
            put(page, 60, 40, "BOTH", kind, vertical=True, reversed=True): ("BOTH", int(kind == "Code39"), 3)}
    assert read(page) == want


def test_two_codes_on_one_row_and_a_code_from_x0():
    page = blank(24, 420)
    want = {put(page, 0, 3, "edge"): ("edge", 0, 0), put(page, 200, 5, "C39", "Code39"): ("C39", 1, 0)}
    assert read(page) == want


def test_rows_and_hull():
    page = blank(40, 200)
    box = put(page, 10, 6, "ab", height=20)
    page[15, :] = 255                                       # one unreadable row: the reads above and below still join (row_gap 2)
    _, rc, _ = br.barcodes(page)
    assert len(rc) == 1 and tuple(rc[0][:4]) == box and int(rc[0][6]) == 19
    page[16:18, :] = 255                                    # three: two groups of 9 and 8 rows
    _, rc, _ = br.barcodes(page)
    assert [int(c[6]) for c in rc] == [9, 8]


def test_every_decoy_yields_no_barcode():
    page, gt = synth.synth_barcode_decoys()
    assert {g["kind"] for g in gt} == {"grid", "comb", "text", "bad_check", "short", "no_quiet", "no_quiet39"}
    assert read(page) == {}
    # the same codes without what spoils them are read: the decoys test the rule, not the renderer
    good = blank(80, 420)
    a = put(good, 30, 5, "DECOY-128", height=P["min_rows"])
    b = put(good, 60, 30, "NOQUIET", height=P["min_rows"])
    assert read(good) == {a: ("DECOY-128", 0, 0), b: ("NOQUIET", 0, 0)}


def test_synthetic_page():
    page, gt = synth.synth_barcode_page(1, h=360, w=900, text_lines=3)
    assert read(page) == {g["box"]: (g["text"], int(g["kind"] == "Code39"), int(g["reversed"]) | 2 * int(g["vertical"])) for g in gt}
