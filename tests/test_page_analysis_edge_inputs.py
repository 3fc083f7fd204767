"""CPU: the restatements on the pages of tests/page_edge_inputs.py — inputs none of them had seen: sides past 4096, hard components,
lists at their capacity.  The GPU file (tests/test_gpu_page_analysis_edges.py) asserts that the device EQUALS the restatements on
these pages; this file is what shows that the restatements alone are right there:
  * mark_reference agrees with the per-pixel flood-fill statement of tests/test_mark_reference.py on every page;
  * the counts the pages are constructed to have are the counts found (72 roots in a row, 2048 / 2049 marks and rules, the nested
    frames, the comb, the whole frames of the long pages), and table_reference finds the rule drawn across every chunk border;
  * every restatement of every page runs in bounded time.  Measured on a CPU build host: the slowest page (65535 x 12) takes 0.22 s
    in mark_reference, 0.06 s in table_reference and 0.02 s in page_orient_reference; the bound asserted is 5 s per page and
    restatement (twenty times the slowest, so that a loaded machine does not trip it)."""
import time

import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.utils import marks

import mark_reference as mr
import page_edge_inputs as pe
import page_orient_reference as pr
import table_reference as tr
from test_mark_reference import flood_fill_marks

P = arch.MARK_PARAMS
BOUND_S = 5.0
TABLE_SETS = [dict(threshold=128, gap=2, min_len=64, max_thick=12), dict(threshold=128, gap=1, min_len=8, max_thick=3)]


def _timed(fn, *a, **kw):
    t = time.perf_counter()
    out = fn(*a, **kw)
    dt = time.perf_counter() - t
    assert dt < BOUND_S, "%s took %.2f s" % (fn.__name__, dt)
    return out


def _marks_equal_flood_fill(ink: np.ndarray) -> np.ndarray:
    got = _timed(mr.marks_of_ink, ink, P["min_side"], P["max_side"])
    assert np.array_equal(got, flood_fill_marks(ink, P["min_side"], P["max_side"]))
    return got


@pytest.mark.parametrize("shape", pe.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_pages(shape):
    h, w = shape
    inks, frames = pe.long_inks(h, w)
    assert len(frames) >= 3 and any(f[3] == w - 1 for f in frames)
    for turned in (False, True):
        for i, ink in enumerate(inks):
            whole = [f[1:] for f in frames if f[0] == i]
            if turned:
                ink, whole = np.ascontiguousarray(ink.T), [(y0, x0, y1, x1) for x0, y0, x1, y1 in whole]
            found = _marks_equal_flood_fill(ink)
            assert {tuple(r[:4]) for r in found.tolist()} >= set(whole)          # every frame that lies whole on the page is a mark
            page = pe.page_of(ink)
            mask, rows = _timed(mr.selection_marks, page)
            assert np.array_equal(rows, found) and mask.shape == (ink.shape[0], (ink.shape[1] + 63) // 64)
            for kw in TABLE_SETS:
                _timed(tr.table_rules, page, **kw)
            _timed(pr.energies, page)
    # the rule drawn across every border, on the page that holds it (feature 9: 200 pixels around the border), in both directions
    page_i, row = divmod(9, h // 2)
    _, rh, rv = tr.table_rules(pe.page_of(inks[page_i]))
    want = [[max(0, b - 96), 2 * row, min(w - 1, b + 103), 2 * row] for b in pe.long_borders(w)]
    assert all(r in rh[:, :4].tolist() for r in want) and len(rv) == 0
    _, rh, rv = tr.table_rules(pe.page_of(np.ascontiguousarray(inks[page_i].T)))
    assert all([r[1], r[0], r[3], r[2]] in rv[:, :4].tolist() for r in want) and len(rh) == 0


def test_hard_components():
    inks = pe.hard_inks()
    found = {name: _marks_equal_flood_fill(ink) for name, ink in inks.items()}
    # five nested frames: every one is a mark of its own on the device's list; the host's nesting rule keeps the outer one
    (x, y), sides = pe.NESTED_AT, pe.NESTED_SIDES
    assert [r[:4] for r in found["nested"].tolist()] == [[x + 2 * k, y + 2 * k, x + 2 * k + s - 1, y + 2 * k + s - 1] for k, s in enumerate(sides)]
    assert [m["box"] for m in marks.select_marks(found["nested"])] == [(x, y, x + sides[0] - 1, y + sides[0] - 1)]
    # the comb joined by its last row is ONE component whose box passes the frame test; the comb of 1-pixel teeth fails it
    (x, y), s = pe.COMB_AT, pe.COMB_SIDE
    assert [r[:4] for r in found["combs"].tolist()] == [[x, y, x + s - 1, y + s - 1]]
    assert len(found["small_spirals"]) == 3
    # one component each: the page-sized shapes and the two blobs joined through a corner
    for name in ("spiral", "serpentine", "diagonal_blobs"):
        row, s, e = mr.runs_of(inks[name])
        assert len(set(mr.run_roots(row, s, e).tolist())) == 1 and len(found[name]) == 0


def test_a_row_of_72_roots():
    ink = pe.row_of_frames_ink()
    found = _marks_equal_flood_fill(ink)
    assert len(found) == pe.ROW_FRAMES == 72 and set(found[:, 1].tolist()) == {5}
    row, s, e = mr.runs_of(ink)
    assert int((row == 5).sum()) == 72           # more than one wave's worth of runs, every one a root, in one row


@pytest.mark.parametrize("n", [2048, 2049])
def test_capacity_pages(n):
    ink = pe.marks_grid_ink(n)
    assert ink.shape == (700, 700)
    found = _marks_equal_flood_fill(ink)
    assert len(found) == n and len(set(found[:, 1].tolist())) == -(-n // 46)      # 46 frames share every y0
    kw = {k: v for k, v in pe.RULE_PARAMS.items() if k != "max_rules"}
    page = pe.page_of(pe.rules_grid_ink(n))
    _, rh, rv = _timed(tr.table_rules, page, **kw)
    assert (len(rh), len(rv)) == (n, 0) and len(set(rh[:, 1].tolist())) == -(-n // 64) and len(set(rh[:, 0].tolist())) == 64
    _, rh, rv = _timed(tr.table_rules, np.ascontiguousarray(page.transpose(1, 0, 2)), **kw)
    assert (len(rh), len(rv)) == (0, n)
    assert arch.TABLE_PARAMS["max_rules"] <= 2048 and pe.RULE_PARAMS["max_rules"] == 2048


def test_ragged_pages_differ_in_every_count():
    pages = pe.ragged_pages()
    assert pages.shape == (7, 200, 300, 3) and len({p.tobytes() for p in pages}) == 7
    n_marks = [len(_timed(mr.selection_marks, p)[1]) for p in pages]
    assert n_marks == [1, 2, 3, 4, 5, 6, 7]
    rules = [tuple(len(r) for r in _timed(tr.table_rules, p)[1:]) for p in pages]
    assert [r[0] for r in rules] == [i % 4 + 1 for i in range(7)] and all(r[1] == 1 for r in rules)
    assert len({pr.energies(p) for p in pages}) == 7


def test_probability_maps_hold_components_on_the_border():
    from oracle import dbpost
    maps = pe.long_prob_maps()
    bits = arch.f32_to_bf16_bits(maps)
    res = [dbpost.db_postprocess(b, maps.shape[1], maps.shape[2]) for b in bits]
    assert [len(r[0]) for r in res] == [4, 1, 2] and res[1][2] > 64         # (the specks are components, below min_size as boxes)
    for boxes, _, _ in res:                                                   # every map has a box that straddles the border
        assert any(b[0::2].min() < pe.CHUNK < b[0::2].max() for b in boxes)
