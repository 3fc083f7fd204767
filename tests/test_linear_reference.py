"""The restatement of the barcode pass with a set of kinds (tests/linear_reference.py) against ground truth: what the renderer
(synth.render_linear: an encoder from digit strings, written from the tables) draws is what is read, through the host text; with the
kinds of lumina_ocr_barcodes it is tests/barcode_reference.py; and what is no barcode reads as none."""
import numpy as np
import pytest

from lumina_ocr import synth
from lumina_ocr.utils import barcodes as bc

import barcode_reference as br
import linear_pages as lp
import linear_reference as lr


def read(page, kinds=lr.ALL_KINDS):
    _, rc, rs = lr.barcodes(page, kinds)
    return lp.found(rc, rs)


def strip(kind, digits, m=2, ratio=2.0, margin=30, **kw):
    el = synth.linear_elements(kind, digits, m, ratio)
    page = lp.blank(16, sum(el) + 2 * margin)
    return page, synth.render_linear(page, margin, 3, kind, digits, m, 10, ratio, **kw)


# the check digits were verified by hand (mod 10, weights 3 and 1)
@pytest.mark.parametrize("kind,digits,name,content,flags", [
    ("EAN13", "4006381333931", "EAN13", "4006381333931", 0), ("EAN13", "5901234123457", "EAN13", "5901234123457", 0),
    ("EAN13", "0036000291452", "UPCA", "036000291452", 0), ("EAN8", "96385074", "EAN8", "96385074", 0), ("UPCE", "01234565", "UPCE", "01234565", 0),
    ("ITF", "00012345678905", "ITF", "00012345678905", 4), ("ITF", "123456", "ITF", "123456", 0)])
def test_known_answers(kind, digits, name, content, flags):
    page, box = strip(kind, digits)
    assert read(page) == {box: (name, content, flags)}
    if kind != "UPCE" and digits != "123456":          # (UPC-E's check is its expansion's, below; six-digit ITF carries none)
        assert synth.check_digit(digits[:-1]) == int(digits[-1])


def test_upce_expansion_and_check():
    assert bc.upce_to_upca([0, 1, 2, 3, 4, 5, 6, 5]) == [int(c) for c in "012345000065"]
    assert synth.check_digit("01234500006") == 5
    _, rc, rs = lr.barcodes(strip("UPCE", "01234565")[0], 16)
    assert [int(v) for v in rs[0][:8]] == [0, 1, 2, 3, 4, 5, 6, 5] and int(rc[0][4]) == bc.KIND_UPCE and int(rc[0][5]) == 8
    for body in ("123450", "123451", "123452", "123453", "123454", "123459", "987657"):      # every branch of the expansion, both number systems
        for ns in "01":
            full = bc.upce_to_upca([int(ns)] + [int(c) for c in body] + [0])[:11]
            digits = ns + body + str(synth.check_digit("".join(map(str, full))))
            page, box = strip("UPCE", digits)
            assert read(page) == {box: ("UPCE", digits, 0)}, digits


@pytest.mark.parametrize("kind,digits", [("EAN13", "4006381333931"), ("EAN8", "96385074"), ("UPCE", "01234565")])
def test_one_digit_altered_gives_no_read(kind, digits):
    for pos in range(1, len(digits) - (1 if kind == "UPCE" else 0)):
        bad = digits[:pos] + str((int(digits[pos]) + 1) % 10) + digits[pos + 1:]
        assert read(strip(kind, bad)[0]) == {}, bad
    assert read(strip(kind, digits)[0]) != {}


def test_every_ean13_first_digit_and_every_digit_in_every_set():
    for first in range(10):
        body = "%d%s" % (first, "01234567895"[first:] + "01234567895"[:first])
        digits = body + str(synth.check_digit(body))
        page, box = strip("EAN13", digits)
        assert read(page) == {box: lp.name_of("EAN13", digits) + (0,)}, digits


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("kind,digits,ratio", [("EAN13", lp.EAN13_A, 2.0), ("EAN8", lp.EAN8, 2.0), ("UPCE", lp.UPCE, 2.0), ("ITF", lp.ITF14, 2.0),
                                               ("ITF", lp.ITF14, 2.5), ("ITF", lp.ITF14, 3.0), ("ITF", "12" * 32, 2.0)])
def test_module_widths_ratios_and_directions(m, kind, digits, ratio):
    for rev in (False, True):
        page, box = strip(kind, digits, m, ratio, reversed=rev)
        flags = int(rev) | (4 if digits == lp.ITF14 else 0)
        assert read(page) == {box: (kind, digits, flags)}
        _, rc, _ = lr.barcodes(page)
        assert len(rc) == 0                                 # the default kinds see nothing in it


def test_itf_lengths():
    assert read(strip("ITF", "1234")[0]) == {}             # four digits: below the minimum
    page, box = strip("ITF", "12" * 32)
    assert read(page) == {box: ("ITF", "12" * 32, 0)}
    assert read(strip("ITF", "12" * 33)[0]) == {}          # 66 digits: more than the 32 pairs a row's wave holds


def test_regimes_on_the_pages_the_device_is_tested_on():
    pages, wants = lp.regime_pages()
    for i in range(len(pages)):
        _, rc, rs = lp.reference(("regime", i), pages[i], lr.ALL_KINDS)
        assert lp.found(rc, rs) == wants[i], i
    assert len(wants[0]) == 18 and len(wants[1]) == 10 and len(wants[2]) == 3
    assert {v[2] for v in wants[0].values()} == {0, 1, 2, 3, 4, 5}      # upright, upside down, vertical, ITF-14


@pytest.mark.parametrize("kinds", [4, 8, 16, 32])
def test_a_single_kind_reads_its_strips_only(kinds):
    pages, wants = lp.regime_pages()
    for i in range(len(pages)):
        _, rc, rs = lp.reference(("regime", i), pages[i], kinds)
        assert lp.found(rc, rs) == lp.only(wants[i], kinds) and (i == 2 or len(rc) > 0)


def test_the_default_kinds_are_the_old_restatement():
    pages, _ = lp.regime_pages()
    todo = [(("regime", i), pages[i]) for i in range(len(pages))] + [(("reference", i), p) for i, p in enumerate(lp.reference_pages())]
    n = 0
    for key, page in todo:
        new, old = lp.reference(key, page, 3), lp.old_reference(key, page)
        assert all(np.array_equal(a, b) for a, b in zip(new, old)), key
        assert len(lr.barcodes(page, lr.ALL_KINDS)[1]) > len(old[1]) if key[0] == "reference" else True
        n += len(old[1])
    assert n >= 10
    assert lr.read128 is br.read128 and lr.read39 is br.read39 and lr.element is br.element


# seeds and sizes of the text-only pages: synth.synth_page(h, w, seed, n_lines)
TEXT_PAGES = [(300, 520, 5, 8), (420, 640, 1, 12), (640, 420, 2, 18), (360, 900, 3, 10), (500, 700, 4, 16)]


@pytest.mark.parametrize("h,w,seed,n_lines", TEXT_PAGES)
def test_text_pages_hold_no_barcode(h, w, seed, n_lines):
    page = synth.synth_page(h, w, seed, n_lines=n_lines)[0]
    assert lr.ink_mask(page, lr.P["threshold"]).mean() > 0.01
    assert read(page) == {}


def test_decoys_hold_no_barcode():
    assert read(synth.synth_barcode_decoys()[0]) == {}
