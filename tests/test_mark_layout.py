"""CPU: selection marks in the result schema — `selection_mark` entries (reference backend/services/ocr_service.py:313-322), their place
among the other entries, the Markdown tokens, and everything unchanged when the option is off or a page has no marks."""
import numpy as np

from lumina_ocr.pipeline import PageDetections
from lumina_ocr.utils import layout, marks, tables

SNAP = 8


def q(x, y, w=80, h=30):
    return [x, y, x + w, y, x + w, y + h, x, y + h]


def row(x0, y0, side, state, edge=None):
    area = (side - 2 * (side // 4)) ** 2
    return [x0, y0, x0 + side - 1, y0 + side - 1, 4 * side if edge is None else edge, area if state else 0, area, int(state)]


def _grid(xs, ys):
    h = [(xs[0] - 1, y - 1, xs[-1] + 1, y + 1, 0) for y in ys]
    v = [(x - 1, ys[0] - 1, x + 1, ys[-1] + 1, 0) for x in xs]
    return h, v


def test_entries_have_the_reference_keys_and_validate():
    found = marks.select_marks(np.array([row(100, 50, 30, True), row(100, 120, 30, False, edge=110)], np.int32))
    boxes = layout.build_mark_boxes(found, 3)
    assert [set(b) for b in boxes] == [{"type", "state", "confidence", "polygon", "page_number"}] * 2      # the reference, :315-321
    assert [(b["type"], b["state"], b["page_number"]) for b in boxes] == [("selection_mark", "selected", 3), ("selection_mark", "unselected", 3)]
    assert boxes[0]["polygon"] == [100.0, 50.0, 129.0, 50.0, 129.0, 79.0, 100.0, 79.0] and boxes[0]["confidence"] == 1.0
    assert boxes[1]["confidence"] == 110 / 120 and isinstance(boxes[1]["confidence"], float)
    assert layout.validate_layout_boxes(boxes) == [] and layout.build_mark_boxes([], 1) == []


def test_token_goes_in_front_of_the_line_to_the_right():
    dets = [(q(150, 52), "yes", 0.9), (q(400, 52), "no", 0.9), (q(150, 200), "later", 0.9), (q(20, 300), "left of its mark", 0.9)]
    merged, _ = layout.reading_order(dets)
    found = marks.select_marks([row(100, 50, 30, True), row(350, 50, 30, False), row(300, 300, 30, True)])
    md = layout.page_markdown(merged, marks=found)
    # the third mark has text on its row, but none that starts to its right: a row of its own after the text
    assert md == ":selected: yes :unselected: no\nlater\nleft of its mark\n:selected:"
    # a line higher or lower than the mark's centre is not its line
    assert layout.page_markdown(merged, marks=marks.select_marks([row(100, 120, 30, False)])) == "yes no\nlater\nleft of its mark\n:unselected:"
    # two marks in front of one line keep the marks' order
    assert layout.page_markdown(merged, marks=marks.select_marks([row(40, 200, 30, True), row(90, 200, 30, False)])).splitlines()[1] == \
        ":selected: :unselected: later"


def test_mark_in_a_table_cell():
    (t,) = tables.find_tables(*_grid([100, 300, 500], [50, 150, 250]), SNAP)
    dets = [(q(160, 80), "a&b", 0.9), (q(360, 80), "c", 0.9), (q(160, 180), "d", 0.9), (q(120, 5), "before", 0.9)]
    merged, ordered = layout.reading_order(dets)
    tables.fill_cells([t], ordered)
    found = marks.select_marks([row(120, 80, 30, True), row(320, 180, 30, False), row(600, 80, 30, False)])
    md = layout.page_markdown(merged, [t], marks=found)
    assert md == ("before\n<table>\n<tr><td>:selected: a&amp;b</td><td>c</td></tr>\n<tr><td>d</td><td>:unselected:</td></tr>\n</table>\n"
                  ":unselected:")
    assert [c["content"] for c in t["cells"]] == ["a&b", "c", "d", ""]           # the table itself is not changed by writing it
    boxes = layout.build_layout_boxes(ordered) + layout.build_mark_boxes(found) + layout.build_table_boxes([t]) + layout.build_paragraph_boxes(merged)
    assert layout.validate_layout_boxes(boxes) == []


def test_without_marks_the_markdown_is_what_it_was():
    (t,) = tables.find_tables(*_grid([100, 300, 500], [50, 150, 250]), SNAP)
    dets = [(q(160, 80), "a", 0.9), (q(360, 80), "c", 0.9), (q(120, 300), "after", 0.9), (q(120, 5), "before", 0.9), (q(600, 80), "beside", 0.9)]
    merged, ordered = layout.reading_order(dets)
    tables.fill_cells([t], ordered)
    for tabs in (None, [], [t]):
        want = layout.page_markdown(merged, tabs)
        assert layout.page_markdown(merged, tabs, marks=None) == want and layout.page_markdown(merged, tabs, marks=[]) == want
    assert layout.page_markdown(merged, [t]) == "before\n<table>\n<tr><td>a</td><td>c</td></tr>\n<tr><td></td><td></td></tr>\n</table>\nbeside\nafter"
    # and marks that touch nothing leave every other row as it was
    with_mark = layout.page_markdown(merged, [t], marks=marks.select_marks([row(700, 400, 30, True)]))
    assert with_mark == layout.page_markdown(merged, [t]) + "\n:selected:"
    assert layout.page_markdown(merged, marks=marks.select_marks([row(700, 400, 30, True)])) == layout.page_markdown(merged) + "\n:selected:"


def _service():
    from lumina_ocr.services import ocr_service as svc
    s = object.__new__(svc.OCRService)
    s._initialized = False
    svc.OCRService.__init__(s)
    return s


def _det(marks_rows=None, rules=False):
    quads = np.array([q(150, 52), q(400, 52), q(150, 200)], np.int32)
    d = PageDetections(quads, ["yes", "no", "later"], np.array([0.9, 0.8, 0.7], np.float32), np.ones(3, np.float32), 1000, 700)
    if rules:
        h, v = _grid([90, 600], [40, 100])
        d.hrules, d.vrules = np.array(h, np.int32), np.array(v, np.int32)
    d.marks = marks_rows
    return d


def test_finish_page_entry_order_counts_and_the_switch():
    s = _service()
    rows = np.array([row(100, 50, 30, True), row(106, 56, 18, True), row(350, 50, 30, False)], np.int32)      # the second is nested in the first
    on = s._finish_page(_det(rows, rules=True), b"jpeg", (700, 1000), 2, (1000, 700), 0.0)
    types = [b["type"] for b in on.layout_boxes]
    assert types == ["word"] * 3 + ["line"] * 3 + ["selection_mark"] * 2 + ["table", "table_cell"] + ["paragraph"] * types.count("paragraph")
    assert types.count("paragraph") >= 1 and layout.validate_layout_boxes(on.layout_boxes) == []
    assert [b["state"] for b in on.layout_boxes if b["type"] == "selection_mark"] == ["selected", "unselected"]
    assert all(b["page_number"] == 2 for b in on.layout_boxes)
    assert on.json_output["selection_marks_count"] == 2 and on.json_output["tables_count"] == 1
    assert "<td>:selected: yes :unselected: no</td>" in on.markdown
    # option off (marks None): the output of a provider that has no marks at all
    off = s._finish_page(_det(None, rules=True), b"jpeg", (700, 1000), 2, (1000, 700), 0.0)
    assert "selection_marks_count" not in off.json_output
    assert off.layout_boxes == [b for b in on.layout_boxes if b["type"] != "selection_mark"]
    assert ":selected:" not in off.markdown and off.markdown == on.markdown.replace(":selected: ", "").replace(":unselected: ", "")
    # option on, page without marks: the same boxes and strings as off, and a count of 0
    none = s._finish_page(_det(np.zeros((0, 8), np.int32), rules=True), b"jpeg", (700, 1000), 2, (1000, 700), 0.0)
    assert none.layout_boxes == off.layout_boxes and none.markdown == off.markdown and none.html == off.html
    assert none.json_output == dict(off.json_output, selection_marks_count=0)


def test_environment_switch(monkeypatch):
    for env, want in ((None, False), ("0", False), ("1", True), ("true", True)):
        if env is None:
            monkeypatch.delenv("LUMINA_OCR_SELECTION_MARKS", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_SELECTION_MARKS", env)
        assert _service()._use_marks is want
