"""CPU: round selection marks (radio buttons) in the result schema, on hand-made device rows: the merge with the checkboxes, nesting
across the two shapes, the entries' keys, the Markdown tokens, and select_marks without round rows unchanged."""
import numpy as np
import pytest

from lumina_ocr.pipeline import PageDetections
from lumina_ocr.utils import layout, marks, tables

from test_mark_layout import _grid, _service, q, row


def rrow(x0, y0, d, state, edge=None):
    """a round mark's device row: edge = the four coverage counts, the core's area about a fifth of the box"""
    area = (d * d) // 5
    return [x0, y0, x0 + d - 1, y0 + d - 1, 4 * d if edge is None else edge, area // 2 if state else 0, area, int(state)]


def test_merge_order_and_shapes():
    sq = [row(300, 50, 30, True), row(100, 200, 30, False), row(100, 400, 30, True)]
    rd = [rrow(100, 50, 30, False), rrow(50, 200, 30, True), rrow(100, 400, 20, False), rrow(400, 400, 24, True)]
    found = marks.select_marks(np.array(sq, np.int32), np.array(rd, np.int32))
    assert [(m["box"][:2], m["shape"]) for m in found] == [((100, 50), "round"), ((300, 50), "square"), ((50, 200), "round"), ((100, 200), "square"),
                                                            ((100, 400), "square"), ((400, 400), "round")]
    # (the round mark at (100, 400) lies inside the checkbox at the same corner: dropped; at equal corners the checkbox comes first)
    assert [m["state"] for m in found] == ["unselected", "selected", "selected", "unselected", "selected", "selected"]
    r = found[0]
    assert r["polygon"] == [100.0, 50.0, 129.0, 50.0, 129.0, 79.0, 100.0, 79.0] and r["confidence"] == 1.0 and isinstance(r["confidence"], float)
    assert marks.select_marks([], [rrow(10, 10, 20, True, edge=70)])[0]["confidence"] == 70 / 80


def test_drop_nested_runs_over_the_union():
    ring, dot = rrow(100, 100, 48, True), rrow(114, 114, 20, True)            # a centre dot clear of its ring, round enough to be a row
    box, inner_ring = row(300, 100, 48, False), rrow(310, 110, 28, False)     # a radio button drawn inside a checkbox
    outer_ring, inner_box = rrow(500, 100, 48, True), row(512, 112, 24, True)
    found = marks.select_marks([box, inner_box], [ring, dot, inner_ring, outer_ring])
    assert [(m["box"], m["shape"]) for m in found] == [((100, 100, 147, 147), "round"), ((300, 100, 347, 147), "square"), ((500, 100, 547, 147), "round")]
    assert [m["box"] for m in marks.select_marks([], [dot, ring])] == [(100, 100, 147, 147)]
    assert len(marks.select_marks([], [ring, rrow(140, 140, 30, False)])) == 2           # overlap is not nesting


def test_without_round_rows_the_result_is_what_it_was():
    rows = [row(10, 10, 40, True), row(16, 16, 28, True), row(100, 10, 30, False, edge=118), row(100, 10, 30, False), row(48, 48, 23, False)]
    want = []
    for x0, y0, x1, y1, edge, _, _, state in marks.drop_nested(rows):                # the function as it stood before the round marks
        w, h = x1 - x0 + 1, y1 - y0 + 1
        want.append(dict(box=(x0, y0, x1, y1), state=marks.STATES[1 if state else 0], confidence=float(edge) / float(2 * (w + h)),
                         polygon=[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]))
    for got in (marks.select_marks(np.array(rows, np.int32)), marks.select_marks(rows, None), marks.select_marks(rows, np.zeros((0, 8), np.int32))):
        assert [{k: v for k, v in m.items() if k != "shape"} for m in got] == want and len(want) == 3
        assert all(m["shape"] == "square" and list(m)[:4] == ["box", "state", "confidence", "polygon"] for m in got)
    assert marks.select_marks(np.zeros((0, 8), np.int32)) == [] and marks.select_marks([], []) == []


def test_entries_keep_the_reference_keys_and_validate():
    found = marks.select_marks([row(100, 120, 30, False)], [rrow(100, 50, 30, True, edge=100)])
    boxes = layout.build_mark_boxes(found, 2)
    assert [set(b) for b in boxes] == [{"type", "state", "confidence", "polygon", "page_number"}] * 2       # no `shape`: the reference's keys
    assert [(b["state"], b["confidence"]) for b in boxes] == [("selected", 100 / 120), ("unselected", 1.0)]
    assert layout.validate_layout_boxes(boxes) == []


def test_tokens_in_the_markdown_and_in_a_table_cell():
    dets = [(q(150, 52), "yes", 0.9), (q(400, 52), "no", 0.9), (q(150, 200), "later", 0.9)]
    merged, _ = layout.reading_order(dets)
    found = marks.select_marks([row(350, 50, 30, False)], [rrow(100, 50, 30, True), rrow(600, 300, 30, False)])
    assert layout.page_markdown(merged, marks=found) == ":selected: yes :unselected: no\nlater\n:unselected:"
    (t,) = tables.find_tables(*_grid([100, 300, 500], [50, 150, 250]), 8)
    dets = [(q(160, 80), "a", 0.9), (q(360, 80), "c", 0.9), (q(160, 180), "d", 0.9)]
    merged, ordered = layout.reading_order(dets)
    tables.fill_cells([t], ordered)
    found = marks.select_marks([row(320, 180, 30, True)], [rrow(120, 80, 30, True), rrow(320, 80, 30, False)])
    md = layout.page_markdown(merged, [t], marks=found)
    assert md == "<table>\n<tr><td>:selected: a</td><td>:unselected: c</td></tr>\n<tr><td>d</td><td>:selected:</td></tr>\n</table>"


def test_finish_page_with_round_marks_and_the_switches(monkeypatch):
    s = _service()
    quads = np.array([q(150, 52), q(400, 52), q(150, 200)], np.int32)
    det = lambda sq, rd: PageDetections(quads, ["yes", "no", "later"], np.array([0.9, 0.8, 0.7], np.float32), np.ones(3, np.float32), 1000, 700,
                                        marks=sq, round_marks=rd)
    sq, rd = np.array([row(350, 50, 30, False)], np.int32), np.array([rrow(100, 50, 30, True)], np.int32)
    on = s._finish_page(det(sq, rd), b"jpeg", (700, 1000), 1, (1000, 700), 0.0)
    assert [b["state"] for b in on.layout_boxes if b["type"] == "selection_mark"] == ["selected", "unselected"]
    assert on.json_output["selection_marks_count"] == 2 and on.markdown.startswith(":selected: yes :unselected: no")
    assert layout.validate_layout_boxes(on.layout_boxes) == []
    off = s._finish_page(det(sq, None), b"jpeg", (700, 1000), 1, (1000, 700), 0.0)
    empty = s._finish_page(det(sq, np.zeros((0, 8), np.int32)), b"jpeg", (700, 1000), 1, (1000, 700), 0.0)
    assert off.layout_boxes == empty.layout_boxes and off.markdown == empty.markdown == "yes :unselected: no\nlater"
    assert off.json_output == empty.json_output and off.json_output["selection_marks_count"] == 1
    for env, want in ((None, False), ("0", False), ("1", True)):
        monkeypatch.delenv("LUMINA_OCR_RADIO_BUTTONS", raising=False) if env is None else monkeypatch.setenv("LUMINA_OCR_RADIO_BUTTONS", env)
        assert _service()._use_round_marks is want


def test_the_option_alone_is_an_error_result_and_the_pipeline_refuses_it(monkeypatch):
    from lumina_ocr.pipeline import OcrPipeline
    from PIL import Image
    monkeypatch.setenv("LUMINA_OCR_RADIO_BUTTONS", "1")
    monkeypatch.delenv("LUMINA_OCR_SELECTION_MARKS", raising=False)
    monkeypatch.setenv("LUMINA_OCR_ALLOW_SYNTHETIC", "1")
    r = _service().process_image_sync(Image.new("RGB", (64, 48), (255, 255, 255)))
    assert not r.success and "LUMINA_OCR_SELECTION_MARKS" in r.error        # errors are data; no engine was built for it

    class NoEngine:
        num_classes, cls_loaded = 6625, False
    with pytest.raises(ValueError, match="round_marks"):
        OcrPipeline(NoEngine(), round_marks=True)
    pipe = OcrPipeline(NoEngine(), marks=True, round_marks=True)
    assert pipe.round_marks and pipe.round_mark_params == __import__("lumina_ocr").arch.ROUND_MARK_PARAMS
