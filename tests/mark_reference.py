"""Restatement (test infrastructure, numpy) of the selection-mark extraction that lumina_ocr_selection_marks runs on the device, as a
sequential definition: ink mask -> runs of every row -> 8-connected components of runs -> candidates by bounding box -> frame test and
interior ink on the page mask -> rows in canonical order.  Plus the restated pipeline with marks (oracle.pipeline + this module +
lumina_ocr.utils.marks) the provider is compared with."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from lumina_ocr import arch

from table_reference import ink_mask, pack_mask

P = arch.MARK_PARAMS


def runs_of(ink: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """bool [H,W] -> (row, start, end) of the maximal ink runs, in raster order."""
    z = np.zeros((ink.shape[0], 1), np.int8)
    d = np.diff(np.concatenate([z, ink.astype(np.int8), z], axis=1), axis=1)
    row, s = np.nonzero(d == 1)
    _, e = np.nonzero(d == -1)
    return row.astype(np.int64), s.astype(np.int64), e.astype(np.int64) - 1


def run_roots(row: np.ndarray, s: np.ndarray, e: np.ndarray) -> np.ndarray:
    """-> for every run the smallest run index of its component: runs of adjacent rows belong together when [s - 1, e + 1] of the one
    overlaps [s, e] of the other (8-connectivity).  Min-label propagation over the pairs, with pointer jumping, to the fixed point."""
    n = len(row)
    big = np.int64(1) << 20
    lo = np.searchsorted(row * big + e, (row - 1) * big + s - 1, "left")        # first run of the row above with e' >= s - 1
    hi = np.searchsorted(row * big + s, (row - 1) * big + e + 1, "right")       # past the last run of the row above with s' <= e + 1
    cnt = np.maximum(hi - lo, 0)
    a = np.repeat(np.arange(n), cnt)
    b = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    lab = np.arange(n)
    while len(a):
        la, lb = lab[a], lab[b]
        mn = np.minimum(la, lb)
        new = lab.copy()
        np.minimum.at(new, la, mn)
        np.minimum.at(new, lb, mn)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def mark_of_box(ink: np.ndarray, x0: int, y0: int, x1: int, y1: int) -> Optional[Tuple[int, int, int, int]]:
    """Steps 4 and 5 on the page mask inside the box -> (edge, ink_in, area_in, state), or None when the frame test fails."""
    w, h = x1 - x0 + 1, y1 - y0 + 1
    box = ink[y0:y1 + 1, x0:x1 + 1]
    t = 1 + min(w, h) // 8
    top, bottom = int(box[:t].any(axis=0).sum()), int(box[h - t:].any(axis=0).sum())
    left, right = int(box[:, :t].any(axis=1).sum()), int(box[:, w - t:].any(axis=1).sum())
    if top < w - w // 8 or bottom < w - w // 8 or left < h - h // 8 or right < h - h // 8:
        return None
    inner = box[h // 4:h - h // 4, w // 4:w - w // 4]
    ink_in, area_in = int(inner.sum()), int(inner.size)
    return top + bottom + left + right, ink_in, area_in, int(16 * ink_in >= area_in)


def marks_of_ink(ink: np.ndarray, min_side: int = P["min_side"], max_side: int = P["max_side"]) -> np.ndarray:
    """bool [H,W] -> int32 [m,8]: x0, y0, x1, y1, edge, ink_in, area_in, state, sorted by (y0, x0, y1, x1, root)."""
    row, s, e = runs_of(ink)
    out = []
    if len(row):
        root = run_roots(row, s, e)
        n = len(row)
        x0, x1, y1 = np.full(n, 1 << 30), np.full(n, -1), np.full(n, -1)
        np.minimum.at(x0, root, s)
        np.maximum.at(x1, root, e)
        np.maximum.at(y1, root, row)
        for r in np.nonzero(root == np.arange(n))[0]:
            bx = (int(x0[r]), int(row[r]), int(x1[r]), int(y1[r]))     # (the root is the component's first run: its row is the top)
            w, h = bx[2] - bx[0] + 1, bx[3] - bx[1] + 1
            if not (min_side <= w <= max_side and min_side <= h <= max_side and 4 * abs(w - h) <= min(w, h)):
                continue
            m = mark_of_box(ink, *bx)
            if m is not None:
                out.append((bx[1], bx[0], bx[3], bx[2], int(r)) + m)
    out.sort()
    return np.array([(t[1], t[0], t[3], t[2]) + t[5:] for t in out], np.int32).reshape(-1, 8)


def selection_marks(page: np.ndarray, threshold: int = P["threshold"], min_side: int = P["min_side"], max_side: int = P["max_side"]):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], marks int32 [m,8])."""
    ink = ink_mask(page, threshold)
    return pack_mask(ink), marks_of_ink(ink, min_side, max_side)


def run_pages(det_w, rec_w, pages_u8: np.ndarray, charset, post=None, max_dim: int = 2000, params: dict = None, table_params: dict = None):
    """The restated pipeline with marks: oracle.pipeline.run_pages, then the marks of every PROCESSED page (what the detector sees);
    with table_params (a dict, or True for arch.TABLE_PARAMS) the rules as well.
    -> (per page dict(quads, texts, scores, det_scores, marks[, hrules, vrules]), processed)."""
    from oracle import pipeline as op
    import table_reference as tr
    mp = dict(P if params is None else params)
    out, processed = op.run_pages(det_w, rec_w, pages_u8, charset, post=post, max_dim=max_dim)
    for d, pg in zip(out, processed):
        d["marks"] = selection_marks(pg, mp["threshold"], mp["min_side"], mp["max_side"])[1]
        if table_params:
            tp = dict(arch.TABLE_PARAMS if table_params is True else table_params)
            _, d["hrules"], d["vrules"] = tr.table_rules(pg, tp["threshold"], tp["gap"], tp["min_len"], tp["max_thick"])
    return out, processed


def page_result(d: dict, page_number: int = 1, snap: int = arch.TABLE_PARAMS["snap"], first_table_index: int = 0):
    """One restated page -> (layout_boxes, markdown, marks) the way the provider builds them."""
    from lumina_ocr.utils import layout, marks, tables
    triples = [(d["quads"][i].tolist(), d["texts"][i], float(d["scores"][i])) for i in range(len(d["texts"]))]
    merged, ordered = layout.reading_order(triples)
    tabs = []
    if "hrules" in d:
        tabs = tables.find_tables(d["hrules"], d["vrules"], snap)
        tables.fill_cells(tabs, ordered)
    found = marks.select_marks(d["marks"])
    boxes = (layout.build_layout_boxes(ordered, page_number) + layout.build_mark_boxes(found, page_number)
             + layout.build_table_boxes(tabs, page_number, first_table_index) + layout.build_paragraph_boxes(merged, page_number))
    return boxes, layout.page_markdown(merged, tabs, marks=found), found
