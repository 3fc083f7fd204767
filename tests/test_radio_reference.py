"""CPU: the restatement of the round selection marks (tests/radio_reference.py) against the ground truth of synth.synth_radio_page, on
the pages that must hold none (synth.synth_round_decoys and every other generator's pages), and its two lists against each other.
These are conditions on arch.ROUND_MARK_PARAMS, not measurements."""
import numpy as np
import pytest
from PIL import Image, ImageDraw

from lumina_ocr import arch, synth

import mark_reference as mr
import radio_reference as rr
from table_reference import ink_mask

P, R = arch.MARK_PARAMS, arch.ROUND_MARK_PARAMS
SIZES = [(1100, 1500), synth.A4_200DPI]
DIAMETERS = [P["min_side"], 13, 32, 63, 64]
STROKES = [1, synth.RADIO_MAX_STROKE]


def both_lists(page: np.ndarray):
    """-> (checkbox rows, round rows) of the restatements, after asserting that no box is in both"""
    ink = ink_mask(page, P["threshold"])
    sq, rd = mr.marks_of_ink(ink), rr.rounds_of_ink(ink)
    assert not {tuple(r[:4]) for r in sq.tolist()} & {tuple(r[:4]) for r in rd.tolist()}
    return sq, rd


def check_radio_page(page: np.ndarray, gt):
    sq, rd = both_lists(page)
    state = lambda rows: sorted((tuple(r[:4]), "selected" if r[7] else "unselected") for r in rows.tolist())
    assert state(rd) == sorted((g["box"], g["state"]) for g in gt if g["shape"] == "round")
    assert np.array_equal(sq, mr.selection_marks(page)[1])
    drawn = {g["box"]: g["state"] for g in gt if g["shape"] == "square"}
    assert {b: s for b, s in state(sq) if b in drawn} == drawn        # (a block inside a checkbox is a second row: mark_reference's own rule)
    return rd


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("h,w", SIZES, ids=["1100x1500", "a4"])
def test_every_radio_button_is_found_with_its_state_and_every_checkbox_as_before(seed, h, w):
    page, gt = synth.synth_radio_page(seed, h, w, noise=3.0 if seed & 1 else 0.0)
    kinds = [g["shape"] for g in gt]
    assert kinds.count("round") == 13 and kinds.count("square") == 3 and sum(g["in_table"] for g in gt) == 4
    check_radio_page(page, gt)
    for diameter in DIAMETERS:
        for stroke in STROKES:
            page, gt = synth.synth_radio_page(seed, h, w, diameter=diameter, stroke=stroke, noise=3.0 if seed & 1 else 0.0)
            rd = check_radio_page(page, gt)
            assert len(rd) == 13 and all(r[2] - r[0] + 1 == diameter and r[3] - r[1] + 1 == diameter for r in rd.tolist())
            assert {g["stroke"] for g in gt if g["shape"] == "round"} == {max(1, min(stroke, diameter // 12))}


def test_both_states_and_the_largest_stroke_are_drawn():
    """coverage of the generator, not of the code"""
    gts = [g for s in range(8) for g in synth.synth_radio_page(s)[1] if g["shape"] == "round"]
    assert {g["state"] for g in gts} == {"selected", "unselected"} and {g["stroke"] for g in gts} >= {1, 2, 3, 4}
    assert max(g["stroke"] for g in synth.synth_radio_page(0, diameter=64, stroke=synth.RADIO_MAX_STROKE)[1]) == synth.RADIO_MAX_STROKE


@pytest.mark.parametrize("seed", range(8))
def test_decoys_hold_no_round_mark(seed):
    page, gt = synth.synth_round_decoys(seed, noise=3.0 if seed & 1 else 0.0)
    assert [g["kind"] for g in gt] == ["disc", "on_rule", "lettered", "concentric"]
    sq, rd = both_lists(page)
    assert len(rd) == 0, rd.tolist()


def test_decoy_letters_are_candidates():
    """the decoys are not rejected for their size: letters of the page are candidates by their boxes, and a ring drawn with a decoy
    shape's pen on the same page IS found"""
    page, _ = synth.synth_round_decoys(0)
    ink = ink_mask(page, P["threshold"])
    row, s, e = mr.runs_of(ink)
    root = mr.run_roots(row, s, e)
    n = len(row)
    x0, x1, y1 = np.full(n, 1 << 30), np.full(n, -1), np.full(n, -1)
    np.minimum.at(x0, root, s), np.maximum.at(x1, root, e), np.maximum.at(y1, root, row)
    roots = np.nonzero(root == np.arange(n))[0]
    w, h = x1[roots] - x0[roots] + 1, y1[roots] - row[roots] + 1
    assert int(((w >= 12) & (w <= 64) & (h >= 12) & (h <= 64) & (4 * np.abs(w - h) <= np.minimum(w, h))).sum()) >= 20
    img = Image.fromarray(page)
    ImageDraw.Draw(img).ellipse((1300, 900, 1339, 939), outline=(10, 10, 10), width=2)
    assert rr.rounds_of_ink(ink_mask(np.asarray(img), P["threshold"]))[:, :4].tolist() == [[1300, 900, 1339, 939]]


def test_text_form_table_and_marks_pages_hold_no_round_mark():
    """the pages and seeds of tests/test_mark_reference.py"""
    h, w = synth.A4_200DPI
    for seed in range(6):
        assert len(both_lists(synth.synth_page(h, w, seed)[0])[1]) == 0
    assert len(both_lists(synth.synth_form_page(0)[0])[1]) == 0
    assert len(both_lists(synth.synth_table_page(3, n_tables=2)[0])[1]) == 0
    for seed in range(6):
        for stroke in (0, 1, 2, 3, 4):
            sq, rd = both_lists(synth.synth_marks_page(seed, stroke=stroke, noise=3.0 if seed & 1 else 0.0)[0])
            assert len(rd) == 0 and len(sq) >= 16


def ring_page(h=120, w=200, at=(60, 30), d=40, stroke=2, dot=False):
    img = Image.new("RGB", (w, h), (255, 255, 255))
    synth._draw_radio(ImageDraw.Draw(img), at[0], at[1], d, stroke, dot, (0, 0, 0))
    return np.asarray(img).copy()


def test_each_test_of_the_definition_rejects_on_its_own():
    base = ring_page()
    (row,) = rr.rounds_of_ink(ink_mask(base, 128)).tolist()
    assert row[:4] == [60, 30, 99, 69] and row[7] == 0 and row[5] == 0 and row[4] == 160
    (row,) = rr.rounds_of_ink(ink_mask(ring_page(dot=True), 128)).tolist()
    assert row[7] == 1 and 16 * row[5] >= row[6] > 0
    b = rr.band_of(40, 40)
    assert b == R["band_min"] + 40 // R["band_div"] == 14
    for dx, dy, found in ((-b, 0, False), (-b - 1, 0, True), (40 + b - 1, 20, False), (40 + b, 20, True), (20, -b, False), (20, -b - 1, True),
                          (20, 40 + b - 1, False), (20, 40 + b, True), (-b, -b, False), (40 + b - 1, 40 + b - 1, False), (40 + b, 40 + b, True)):
        pg = base.copy()
        pg[30 + dy, 60 + dx] = 0                                       # one ink pixel just inside / just outside the band
        assert (len(rr.rounds_of_ink(ink_mask(pg, 128))) == 1) is found, (dx, dy)
    pg = base.copy()
    pg[30:36, 60:66] = 0                                               # ink in a corner of the box: beyond the outer circle
    assert len(rr.rounds_of_ink(ink_mask(pg, 128))) == 0
    pg = base.copy()
    pg[30:70, 92:100] = 255                                            # an open ring: a C
    assert len(rr.rounds_of_ink(ink_mask(pg, 128))) == 0
    pg = base.copy()
    pg[50, 68] = 0                                                     # a speck in the moat (q = (2 * 8 - 39)^2 + 1 between core and ring zone)
    assert len(rr.rounds_of_ink(ink_mask(pg, 128))) == 0
    assert len(rr.rounds_of_ink(ink_mask(ring_page(stroke=6), 128))) == 0          # a thick ring: an O
    assert len(rr.rounds_of_ink(ink_mask(ring_page(d=11), 128))) == 0 and len(rr.rounds_of_ink(ink_mask(ring_page(d=12, stroke=1), 128))) == 1
    assert len(rr.rounds_of_ink(ink_mask(ring_page(d=64, at=(60, 20)), 128))) == 1 and len(rr.rounds_of_ink(ink_mask(ring_page(d=65, at=(60, 20)), 128))) == 0


def test_a_frame_is_never_a_round_mark_whatever_the_parameters():
    """disjoint by construction: with parameters that let every shape through, a box that passes the frame test still is no round mark"""
    loose = dict(out_max=1 << 20, ring_div=1, band_div=4, band_min=0)
    page = synth.synth_marks_page(2, 500, 700, n_marks=6, table=False)[0]
    ink = ink_mask(page, 128)
    sq, rd = mr.marks_of_ink(ink), rr.rounds_of_ink(ink, rp=loose)
    assert len(sq) >= 6 and not {tuple(r[:4]) for r in sq.tolist()} & {tuple(r[:4]) for r in rd.tolist()}
    for x0, y0, x1, y1 in sq[:, :4].tolist():
        assert rr.round_of_box(ink, x0, y0, x1, y1, rp=loose) is None


def test_zone_bounds_nest_at_every_size():
    for ring_div in (1, 4, 12, 64):
        for d in range(4, 65):
            outer, inner, core = rr.zone_bounds(d, d - d // 5, ring_div)
            assert outer > inner >= core >= 0


def test_run_pages_and_page_result_carry_round_marks(monkeypatch):
    from oracle import pipeline as op
    page, gt = synth.synth_radio_page(2, 560, 760, n_marks=4, table=False, max_side=40)
    quads = np.array([[g["label_box"][0], g["label_box"][1], g["label_box"][2], g["label_box"][1], g["label_box"][2], g["label_box"][3],
                       g["label_box"][0], g["label_box"][3]] for g in gt], np.int32)
    fake = dict(quads=quads, texts=[g["label"] for g in gt], scores=np.ones(len(gt), np.float32), det_scores=np.ones(len(gt), np.float32))
    monkeypatch.setattr(op, "run_pages", lambda *a, **k: ([dict(fake)], page[None]))
    out, _ = rr.run_pages(None, None, page[None], None)
    assert len(out[0]["round_marks"]) == 3 and len(out[0]["marks"]) >= 1
    boxes, md, found = rr.page_result(out[0])
    assert [(m["box"], m["state"], m["shape"]) for m in found] == [(g["box"], g["state"], g["shape"]) for g in gt]
    assert [b["state"] for b in boxes if b["type"] == "selection_mark"] == [g["state"] for g in gt]
    assert all(":%s: %s" % (g["state"], g["label"]) in md for g in gt)            # (two marks of one row share a line of the Markdown)
    assert md.count(":selected:") + md.count(":unselected:") == len(gt)
