"""CPU: rules -> tables (lumina_ocr/utils/tables.py) and the `table` / `table_cell` entries and Markdown block of layout.py."""
import numpy as np

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout, tables

import table_reference as tr

SNAP = arch.TABLE_PARAMS["snap"]
T = 3   # rule thickness of the hand-made grids


def grid(xs, ys, skip_h=(), skip_v=(), x_off=0, short=0):
    """Rules of a full grid on centre-lines xs / ys, thickness T, one rule per elementary side (so that sides can be left out:
    skip_h = {(line k, column c)}, skip_v = {(line k, row r)}); short: the horizontal rule of line 1, column 0 ends that many pixels early."""
    h = [(xs[c] - 1, ys[k] - 1, xs[c + 1] + 1 - (short if (k, c) == (1, 0) else 0), ys[k] + 1, 0)
         for k in range(len(ys)) for c in range(len(xs) - 1) if (k, c) not in skip_h]
    v = [(xs[k] - 1 + x_off, ys[r] - 1, xs[k] + 1 + x_off, ys[r + 1] + 1, 0) for k in range(len(xs)) for r in range(len(ys) - 1) if (k, r) not in skip_v]
    return h, v


def shape(t):
    return [(c["row_index"], c["column_index"], c["row_span"], c["column_span"]) for c in t["cells"]]


def test_one_by_one_and_three_by_four():
    (t,) = tables.find_tables(*grid([100, 400], [50, 150]), SNAP)
    assert (t["row_count"], t["column_count"], t["xs"], t["ys"]) == (1, 1, [100, 400], [50, 150]) and shape(t) == [(0, 0, 1, 1)]
    assert t["polygon"] == [100.0, 50.0, 400.0, 50.0, 400.0, 150.0, 100.0, 150.0] == t["cells"][0]["polygon"]      # TL, TR, BR, BL
    xs, ys = [100, 300, 500, 700, 900], [50, 150, 250, 350]
    (t,) = tables.find_tables(*grid(xs, ys), SNAP)
    assert (t["row_count"], t["column_count"], t["xs"], t["ys"]) == (3, 4, xs, ys)
    assert shape(t) == [(r, c, 1, 1) for r in range(3) for c in range(4)]
    assert t["cells"][5]["polygon"] == [300.0, 150.0, 500.0, 150.0, 500.0, 250.0, 300.0, 250.0]


def test_rules_as_the_device_gives_them_whole_lines():
    h = [(99, 49 + 100 * k, 501, 51 + 100 * k, 1206) for k in range(3)]
    v = [(99 + 200 * k, 49, 101 + 200 * k, 251, 606) for k in range(3)]
    (t,) = tables.find_tables(np.array(h, np.int32), np.array(v, np.int32), SNAP)
    assert (t["row_count"], t["column_count"]) == (2, 2) and len(t["cells"]) == 4


def test_two_tables_on_a_page_ordered_by_top_left():
    h1, v1 = grid([600, 800, 1000], [400, 500, 600])
    h2, v2 = grid([100, 300], [400, 500])
    h3, v3 = grid([100, 300, 500], [50, 150])
    ts = tables.find_tables(h1 + h2 + h3, v1 + v2 + v3, SNAP)
    assert [(t["ys"][0], t["xs"][0], t["row_count"], t["column_count"]) for t in ts] == [(50, 100, 1, 2), (400, 100, 1, 1), (400, 600, 2, 2)]
    boxes = layout.build_table_boxes(ts, 3, first_table_index=5)
    assert [b["table_index"] for b in boxes if b["type"] == "table"] == [5, 6, 7] and all(b["page_number"] == 3 for b in boxes)


def test_spanning_header():
    xs, ys = [100, 300, 500, 700], [50, 150, 250]
    (t,) = tables.find_tables(*grid(xs, ys, skip_v={(1, 0), (2, 0)}), SNAP)      # no inner vertical rule in the first row
    assert (t["row_count"], t["column_count"]) == (2, 3)
    assert shape(t) == [(0, 0, 1, 3), (1, 0, 1, 1), (1, 1, 1, 1), (1, 2, 1, 1)]
    assert t["cells"][0]["polygon"] == [100.0, 50.0, 700.0, 50.0, 700.0, 150.0, 100.0, 150.0]
    boxes = layout.build_table_boxes([t])
    assert boxes[1]["column_span"] == 3 and "row_span" not in boxes[1] and all("column_span" not in b and "row_span" not in b for b in boxes[2:])
    (t,) = tables.find_tables(*grid(xs, ys + [350], skip_h={(2, 0)}), SNAP)       # first column: rows 1 and 2 are one cell
    assert (1, 0, 2, 1) in shape(t) and len(t["cells"]) == 8


def test_l_shaped_merge_falls_back_to_elementary_cells():
    xs, ys = [100, 300, 500], [50, 150, 250]
    (t,) = tables.find_tables(*grid(xs, ys, skip_v={(1, 0)}, skip_h={(1, 0)}), SNAP)     # (0,0) + (0,1) + (1,0): an L
    assert shape(t) == [(r, c, 1, 1) for r in range(2) for c in range(2)]


def test_rule_ends_short_by_snap_and_by_snap_plus_one():
    xs, ys = [100, 300, 500], [50, 150, 250]
    for short, merged in ((SNAP + 1, False), (SNAP + 2, True)):
        # a rule drawn to xs[1] + 1 - short ends short - 1 pixels before the grid line: the side is covered while short - 1 <= snap
        (t,) = tables.find_tables(*grid(xs, ys, short=short), SNAP)
        assert (t["row_count"], t["column_count"]) == (2, 2)
        assert shape(t) == ([(0, 0, 2, 1), (0, 1, 1, 1), (1, 1, 1, 1)] if merged else [(0, 0, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1)])
    # touching: a vertical rule whose centre-line is snap (not snap + 1) beyond the end of the horizontal rules still joins them
    h = [(100, 49, 400, 51, 0), (100, 149, 400, 151, 0)]
    for off, n in ((SNAP, 1), (SNAP + 1, 0)):
        v = [(99, 49, 101, 151, 0), (400 + off - 1, 49, 400 + off + 1, 151, 0)]
        assert len(tables.find_tables(h, v, SNAP)) == n


def test_grid_lines_are_rounded_means_of_close_centre_lines():
    h = [(100, 49, 300, 51, 0), (300, 52, 500, 54, 0), (100, 149, 500, 151, 0)]        # centre-lines 50 and 53 -> one grid line at 52
    v = [(99, 49, 101, 151, 0), (499, 49, 501, 151, 0)]
    (t,) = tables.find_tables(h, v, SNAP)
    assert t["ys"] == [(2 * (50 + 53) + 2) // 4, 150] == [52, 150] and t["row_count"] == 1


def test_a_lone_underline_and_ruled_pages_are_no_tables():
    assert tables.find_tables([(100, 50, 600, 52, 0)], [], SNAP) == []
    assert tables.find_tables([(100, 50, 600, 52, 0), (100, 150, 600, 152, 0)], [(99, 50, 101, 152, 0)], SNAP) == []      # one vertical rule only
    _, h, v = tr.table_rules(synth.synth_page(700, 1000, 0, n_lines=16, ruled=True)[0])
    assert len(h) >= 10 and len(v) == 0 and tables.find_tables(h, v, SNAP) == []


def _table_with_lines():
    xs, ys = [100, 300, 500], [50, 150, 250]
    (t,) = tables.find_tables(*grid(xs, ys, skip_v={(1, 0)}), SNAP)                    # header across both columns
    q = lambda x, y: [x, y, x + 80, y, x + 80, y + 30, x, y + 30]
    dets = [(q(120, 300), "after <the> table", 0.9), (q(320, 180), "b & c", 0.8), (q(120, 180), "a", 0.9), (q(120, 80), "head", 0.9),
            (q(120, 5), "before", 0.9), (q(600, 180), "beside", 0.9)]
    merged, ordered = layout.reading_order(dets)
    return t, merged, ordered


def test_cell_content_and_half_open_intervals():
    t, merged, ordered = _table_with_lines()
    where = tables.fill_cells([t], ordered)
    assert [c["content"] for c in t["cells"]] == ["head", "a", "b & c"]
    assert sorted(where) == [-1, -1, -1, 0, 0, 0]
    assert tables.cell_at(t, 300, 200)["column_index"] == 1 and tables.cell_at(t, 299.75, 200)["column_index"] == 0      # left side included
    assert tables.cell_at(t, 100, 50)["row_index"] == 0 and tables.cell_at(t, 500, 200) is None and tables.cell_at(t, 200, 250) is None
    two = [(q, "x%d" % i, 0.9) for i, q in enumerate(([110, 160, 190, 160, 190, 190, 110, 190], [200, 160, 280, 160, 280, 190, 200, 190]))]
    tables.fill_cells([t], layout.reading_order(two)[1])
    assert t["cells"][1]["content"] == "x0 x1"                                         # one space, reading order


def test_entries_have_the_reference_keys_and_validate():
    t, merged, ordered = _table_with_lines()
    tables.fill_cells([t], ordered)
    boxes = layout.build_table_boxes([t], 2)
    # the reference, backend/services/ocr_service.py:331-352
    assert set(boxes[0]) == {"type", "table_index", "row_count", "column_count", "polygon", "page_number"}
    assert set(boxes[2]) == {"type", "content", "row_index", "column_index", "polygon", "page_number"}
    assert set(boxes[1]) == set(boxes[2]) | {"column_span"}
    assert [b["type"] for b in boxes] == ["table", "table_cell", "table_cell", "table_cell"]
    allb = layout.build_layout_boxes(ordered, 2) + boxes + layout.build_paragraph_boxes(merged, 2)
    assert layout.validate_layout_boxes(allb) == []
    types = [b["type"] for b in allb]
    assert types == sorted(types, key=["word", "line", "table", "table_cell", "paragraph"].index) or types.index("table") > max(i for i, k in enumerate(types) if k == "line")
    bad = dict(boxes[0], row_count=0)
    assert layout.validate_layout_boxes([bad]) and layout.validate_layout_boxes([dict(boxes[2], row_index="1")])
    assert layout.validate_layout_boxes([dict(boxes[1], column_span=1)]) and layout.validate_layout_boxes([dict(boxes[2], content=None)])


def test_markdown_block():
    t, merged, ordered = _table_with_lines()
    tables.fill_cells([t], ordered)
    md = layout.page_markdown(merged, [t])
    assert md == ("before\n<table>\n<tr><td colspan=\"2\">head</td></tr>\n<tr><td>a</td><td>b &amp; c</td></tr>\n</table>\nbeside\n"
                  "after <the> table")
    plain = layout.page_markdown(merged)
    assert plain == "before\nhead\na b & c beside\nafter <the> table"                   # without the argument: today's output
    assert layout.page_markdown(merged, []) == plain and layout.page_markdown(merged, None) == plain
    assert layout.table_markdown(dict(row_count=1, cells=[dict(row_index=0, column_index=0, row_span=2, column_span=1, content="<x>")])) == \
        "<table>\n<tr><td rowspan=\"2\">&lt;x&gt;</td></tr>\n</table>"


def test_synthetic_table_page_ground_truth():
    for seed, kw in ((0, {}), (1, dict(spans=True, rows=4, cols=3)), (2, dict(n_tables=2, noise=3.0)), (3, dict(thickness=2, spans=True)), (4, dict(thickness=5))):
        page, gt = synth.synth_table_page(seed, **kw)
        _, h, v = tr.table_rules(page)
        ts = tables.find_tables(h, v, SNAP)
        assert len(ts) == len(gt) >= 1
        for t, g in zip(ts, gt):
            assert (t["xs"], t["ys"], t["row_count"], t["column_count"]) == (g["xs"], g["ys"], g["row_count"], g["column_count"])
            assert shape(t) == [(c["row_index"], c["column_index"], c["row_span"], c["column_span"]) for c in g["cells"]]
            for c in g["cells"]:      # the rendered text lies inside its cell
                cx, cy = (c["box"][0] + c["box"][2]) / 2, (c["box"][1] + c["box"][3]) / 2
                hit = tables.cell_at(t, cx, cy)
                assert (hit["row_index"], hit["column_index"]) == (c["row_index"], c["column_index"])
