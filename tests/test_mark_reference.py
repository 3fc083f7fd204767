"""CPU: the restatement of the selection-mark extraction (tests/mark_reference.py) against a per-pixel flood-fill statement of the same
definition, against the ground truth of synth.synth_marks_page, and on the pages that must have no marks; the host's nesting rule."""
import numpy as np
import pytest
from PIL import Image, ImageDraw

from lumina_ocr import arch, synth
from lumina_ocr.utils import marks

import mark_reference as mr

P = arch.MARK_PARAMS


def flood_fill_marks(ink: np.ndarray, min_side: int, max_side: int) -> np.ndarray:
    """The definition pixel by pixel: 8-connected components by flood fill from every unvisited ink pixel in raster order (so a
    component's seed is its first pixel, the start of its first run), then steps 3-6 with plain loops."""
    h, w = ink.shape
    seen = np.zeros_like(ink, bool)
    out = []
    for sy in range(h):
        for sx in range(w):
            if not ink[sy, sx] or seen[sy, sx]:
                continue
            stack, x0, y0, x1, y1 = [(sy, sx)], sx, sy, sx, sy
            seen[sy, sx] = True
            while stack:
                y, x = stack.pop()
                x0, y0, x1, y1 = min(x0, x), min(y0, y), max(x1, x), max(y1, y)
                for ny in range(max(0, y - 1), min(h, y + 2)):
                    for nx in range(max(0, x - 1), min(w, x + 2)):
                        if ink[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
            bw, bh = x1 - x0 + 1, y1 - y0 + 1
            if not (min_side <= bw <= max_side and min_side <= bh <= max_side and 4 * abs(bw - bh) <= min(bw, bh)):
                continue
            t = 1 + min(bw, bh) // 8
            top = sum(any(ink[y0 + k, x] for k in range(t)) for x in range(x0, x1 + 1))
            bottom = sum(any(ink[y1 - k, x] for k in range(t)) for x in range(x0, x1 + 1))
            left = sum(any(ink[y, x0 + k] for k in range(t)) for y in range(y0, y1 + 1))
            right = sum(any(ink[y, x1 - k] for k in range(t)) for y in range(y0, y1 + 1))
            if top < bw - bw // 8 or bottom < bw - bw // 8 or left < bh - bh // 8 or right < bh - bh // 8:
                continue
            xs, ys = range(x0 + bw // 4, x1 - bw // 4 + 1), range(y0 + bh // 4, y1 - bh // 4 + 1)
            ink_in, area_in = sum(int(ink[y, x]) for y in ys for x in xs), len(xs) * len(ys)
            out.append((y0, x0, y1, x1, sy * w + sx, top + bottom + left + right, ink_in, area_in, int(16 * ink_in >= area_in)))
    out.sort()
    return np.array([(t[1], t[0], t[3], t[2]) + t[5:] for t in out], np.int32).reshape(-1, 8)


def frames_page(rng: np.random.Generator, h: int, w: int) -> np.ndarray:
    """bool [h,w]: random frames (some broken, some filled, some overlapping, some cut by the page edge) under random dots"""
    ink = rng.random((h, w)) < float(rng.choice([0.0, 0.02, 0.1]))
    for _ in range(int(rng.integers(2, 7))):
        s, t = int(rng.integers(3, 30)), int(rng.integers(1, 4))
        s2 = s + int(rng.integers(-2, 3))
        y, x = int(rng.integers(-4, h - 4)), int(rng.integers(-4, w - 4))
        fr = np.zeros((max(s, 1), max(s2, 1)), bool)
        fr[:t], fr[-t:], fr[:, :t], fr[:, -t:] = True, True, True, True
        kind = int(rng.integers(0, 4))
        if kind == 1:
            fr[:] = True
        elif kind == 2 and s > 8 and s2 > 8:
            fr[s // 3:2 * s // 3, s2 // 3:2 * s2 // 3] = True
        elif kind == 3:
            fr[int(rng.integers(0, fr.shape[0])), :] = False
        ya, xa = max(0, y), max(0, x)
        yb, xb = min(h, y + fr.shape[0]), min(w, x + fr.shape[1])
        if yb > ya and xb > xa:
            ink[ya:yb, xa:xb] |= fr[ya - y:yb - y, xa - x:xb - x]
    return ink


@pytest.mark.parametrize("seed", range(24))
def test_restatement_equals_the_flood_fill_statement(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(20, 70)), int(rng.integers(20, 90))
    ink = frames_page(rng, h, w)
    for lo, hi in ((4, 64), (6, 20), (12, 64)):
        assert np.array_equal(mr.marks_of_ink(ink, lo, hi), flood_fill_marks(ink, lo, hi))


def test_the_flood_fill_pages_do_hold_marks():
    """coverage of the generator above, not of the code: the equality is not one between empty lists"""
    per_page = [len(mr.marks_of_ink(frames_page(np.random.default_rng(s), 60, 80), 4, 64)) for s in range(24)]
    assert sum(1 for n in per_page if n) >= 6


def test_mask_is_the_tables_mask():
    import table_reference as tr
    page = synth.synth_marks_page(1, 300, 420, n_marks=4, table=False, noise=3.0)[0]
    mask, _ = mr.selection_marks(page)
    assert np.array_equal(mask, tr.pack_mask(tr.ink_mask(page))) and mask.dtype == np.uint64 and mask.shape == (300, 7)


def _found(page, **kw):
    return [(m["box"], m["state"]) for m in marks.select_marks(mr.selection_marks(page, **kw)[1])]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("stroke", [0, 1, 2, 3, 4])
def test_every_drawn_box_is_found_with_its_state_and_nothing_else(seed, stroke):
    page, gt = synth.synth_marks_page(seed, stroke=stroke, noise=3.0 if seed & 1 else 0.0)
    assert len(gt) == 16 and sum(g["in_table"] for g in gt) == 4
    assert sorted(_found(page)) == sorted((g["box"], g["state"]) for g in gt)


@pytest.mark.parametrize("side", list(range(P["min_side"], P["max_side"] + 1, 4)) + [P["max_side"]])
def test_every_side_from_min_to_max(side):
    for stroke in (1, 2, 3, 4):
        page, gt = synth.synth_marks_page(side, 700, 1000, n_marks=10, side=side, stroke=stroke, table=False, noise=3.0)
        assert len(gt) == 10 and all(g["box"][2] - g["box"][0] + 1 == side for g in gt)
        assert sorted(_found(page)) == sorted((g["box"], g["state"]) for g in gt)


def test_sides_just_outside_the_range_are_rejected():
    for side in (P["min_side"] - 1, P["max_side"] + 1):
        page, gt = synth.synth_marks_page(3, 700, 1000, n_marks=10, side=side, stroke=2, table=False)
        assert len(gt) == 10
        drawn = {g["box"] for g in gt}
        assert not any(box in drawn for box, _ in _found(page))      # (the clear block inside a 65-pixel frame is a square of its own)
        ink = mr.ink_mask(page)
        assert sorted(tuple(r[:4]) for r in mr.marks_of_ink(ink, 4, 100) if tuple(r[:4]) in drawn) == sorted(drawn)   # only the side keeps them out


def test_text_form_and_table_pages_have_no_marks():
    h, w = synth.A4_200DPI
    for seed in range(6):
        assert len(mr.selection_marks(synth.synth_page(h, w, seed)[0])[1]) == 0
    assert len(mr.selection_marks(synth.synth_form_page(0)[0])[1]) == 0
    assert len(mr.selection_marks(synth.synth_table_page(3, n_tables=2)[0])[1]) == 0


def test_round_and_open_shapes_are_not_marks():
    img = Image.new("RGB", (400, 120), (255, 255, 255))
    d = ImageDraw.Draw(img)
    d.ellipse((10, 10, 50, 50), outline=(0, 0, 0), width=2)                 # a radio button
    d.line((100, 10, 100, 50), fill=(0, 0, 0), width=2)
    d.line((100, 50, 140, 50), fill=(0, 0, 0), width=2)                     # an L
    d.rectangle((200, 10, 240, 50), outline=(0, 0, 0), width=2)
    d.rectangle((215, 0, 225, 20), fill=(255, 255, 255))                    # a frame with a gap in its top side
    d.rectangle((300, 10, 340, 50), outline=(0, 0, 0), width=2)             # and a whole one
    assert _found(np.asarray(img)) == [((300, 10, 340, 50), "unselected")]


def test_nesting_rule_and_host_fields():
    rows = [[10, 10, 49, 49, 160, 300, 400, 1], [16, 16, 43, 43, 112, 196, 196, 1], [100, 10, 129, 39, 118, 0, 256, 0],
            [100, 10, 129, 39, 120, 0, 256, 0], [48, 48, 70, 70, 92, 0, 144, 0]]
    kept = marks.drop_nested(rows)
    assert kept == [rows[0], rows[2], rows[4]]           # the inner square goes; of two equal boxes the first stays; overlap is not nesting
    found = marks.select_marks(np.array(rows, np.int32))
    assert [m["state"] for m in found] == ["selected", "unselected", "unselected"]
    assert found[0]["box"] == (10, 10, 49, 49) and found[0]["polygon"] == [10.0, 10.0, 49.0, 10.0, 49.0, 49.0, 10.0, 49.0]
    assert found[0]["confidence"] == 1.0 and found[1]["confidence"] == 118 / 120 and all(isinstance(m["confidence"], float) for m in found)
    assert marks.select_marks(np.zeros((0, 8), np.int32)) == []
    # the block kind of the generator is exactly this case: two device rows, one mark
    page, gt = synth.synth_marks_page(0, 300, 420, n_marks=0, table=False)
    img = Image.fromarray(page)
    synth._draw_mark(ImageDraw.Draw(img), 50, 100, 48, 2, "block", (0, 0, 0))
    rows = mr.selection_marks(np.asarray(img))[1]
    assert [r[:4] for r in rows.tolist()] == [[50, 100, 97, 147], [54, 104, 93, 143]] and _found(np.asarray(img)) == [((50, 100, 97, 147), "selected")]


def test_run_pages_and_page_result_carry_marks(monkeypatch):
    """the restated pipeline's marks half, with the networks stubbed out (the full pipeline runs in the GPU provider test)"""
    from oracle import pipeline as op
    page, gt = synth.synth_marks_page(2, 500, 700, n_marks=4, table=False)
    quads = np.array([[g["label_box"][0], g["label_box"][1], g["label_box"][2], g["label_box"][1], g["label_box"][2], g["label_box"][3],
                       g["label_box"][0], g["label_box"][3]] for g in gt], np.int32)
    fake = dict(quads=quads, texts=[g["label"] for g in gt], scores=np.ones(len(gt), np.float32), det_scores=np.ones(len(gt), np.float32))
    monkeypatch.setattr(op, "run_pages", lambda *a, **k: ([dict(fake)], page[None]))
    out, _ = mr.run_pages(None, None, page[None], None, table_params=True)
    assert len(out[0]["marks"]) >= 4 and out[0]["hrules"].shape == (0, 5)
    boxes, md, found = mr.page_result(out[0])
    assert [b["state"] for b in boxes if b["type"] == "selection_mark"] == [g["state"] for g in gt]
    assert sorted(md.splitlines()) == sorted(":%s: %s" % (g["state"], g["label"]) for g in gt)
