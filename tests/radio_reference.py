"""Restatement (test infrastructure, numpy) of the round selection marks (radio buttons) that lumina_ocr_selection_marks_round finds on
the device, as a sequential definition on the checkboxes' ink mask, runs and 8-connected components (tests/mark_reference.py): a
candidate by the checkboxes' rule that is no frame -> zones of its box by q = u^2 + v^2 in doubled coordinates about the box centre
-> roundness, thin ring, isolation -> rows in the checkboxes' format and order.  Integer arithmetic only; every reduction is a min, max,
add, or, or a count, so the device equals it exactly.  Plus the restated pipeline with both kinds of mark."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from lumina_ocr import arch

import mark_reference as mr
from mark_reference import run_roots, runs_of
from table_reference import ink_mask, pack_mask

P = arch.MARK_PARAMS
R = arch.ROUND_MARK_PARAMS


def zone_bounds(w: int, h: int, ring_div: int) -> Tuple[int, int, int]:
    """-> (outer, inner, core): q <= outer is inside the outer circle, inner < q <= outer the ring zone, core < q <= inner the moat,
    q <= core the core.  D = max(w, h), T = 1 + D // ring_div: outer = (D + 1)^2, core = D^2 // 4, inner = max((D - 2T)^2, core)
    (D - 2T not below 0)."""
    D = max(w, h)
    T = 1 + D // ring_div
    core = D * D // 4
    return (D + 1) ** 2, max(max(D - 2 * T, 0) ** 2, core), core


def band_of(w: int, h: int, rp: dict = R) -> int:
    return rp["band_min"] + min(w, h) // rp["band_div"]


def round_of_box(ink: np.ndarray, x0: int, y0: int, x1: int, y1: int, rp: dict = R) -> Optional[Tuple[int, int, int, int]]:
    """The tests on the page mask -> (edge, ink_in, area_in, state), or None when the box holds no round mark.  A box that passes the
    checkboxes' frame test is never one: the two lists are disjoint by construction."""
    if mr.mark_of_box(ink, x0, y0, x1, y1) is not None:
        return None
    H, W = ink.shape
    w, h = x1 - x0 + 1, y1 - y0 + 1
    box = ink[y0:y1 + 1, x0:x1 + 1]
    u, v = 2 * np.arange(w) - (w - 1), 2 * np.arange(h) - (h - 1)
    q = u[None, :] ** 2 + v[:, None] ** 2
    outer, inner, core = zone_bounds(w, h, rp["ring_div"])
    if int((box & (q > outer)).sum()) > rp["out_max"]:
        return None
    ring = box & (q <= outer) & (q > inner)
    top, bottom = int(ring[v <= 0].any(axis=0).sum()), int(ring[v >= 0].any(axis=0).sum())
    left, right = int(ring[:, u <= 0].any(axis=1).sum()), int(ring[:, u >= 0].any(axis=1).sum())
    if top < w - w // 8 or bottom < w - w // 8 or left < h - h // 8 or right < h - h // 8:
        return None
    if (box & (q <= inner) & (q > core)).any():
        return None
    b = band_of(w, h, rp)
    around = ink[max(0, y0 - b):min(H, y1 + b + 1), max(0, x0 - b):min(W, x1 + b + 1)]
    if int(around.sum()) != int(box.sum()):
        return None
    ink_in, area_in = int((box & (q <= core)).sum()), int((q <= core).sum())
    return top + bottom + left + right, ink_in, area_in, int(16 * ink_in >= area_in)


def rounds_of_ink(ink: np.ndarray, min_side: int = P["min_side"], max_side: int = P["max_side"], rp: dict = R) -> np.ndarray:
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
            bx = (int(x0[r]), int(row[r]), int(x1[r]), int(y1[r]))
            w, h = bx[2] - bx[0] + 1, bx[3] - bx[1] + 1
            if not (min_side <= w <= max_side and min_side <= h <= max_side and 4 * abs(w - h) <= min(w, h)):
                continue
            m = round_of_box(ink, *bx, rp=rp)
            if m is not None:
                out.append((bx[1], bx[0], bx[3], bx[2], int(r)) + m)
    out.sort()
    return np.array([(t[1], t[0], t[3], t[2]) + t[5:] for t in out], np.int32).reshape(-1, 8)


def selection_marks_round(page: np.ndarray, threshold: int = P["threshold"], min_side: int = P["min_side"], max_side: int = P["max_side"],
                          rp: dict = R):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], checkbox rows int32 [m,8], round rows int32 [k,8])."""
    ink = ink_mask(page, threshold)
    return pack_mask(ink), mr.marks_of_ink(ink, min_side, max_side), rounds_of_ink(ink, min_side, max_side, rp)


def run_pages(det_w, rec_w, pages_u8: np.ndarray, charset, post=None, max_dim: int = 2000, params: dict = None, table_params: dict = None,
              round_params: dict = None):
    """mark_reference.run_pages, then the round marks of every PROCESSED page as d["round_marks"]."""
    mp = dict(P if params is None else params)
    rp = dict(R if round_params is None else round_params)
    out, processed = mr.run_pages(det_w, rec_w, pages_u8, charset, post=post, max_dim=max_dim, params=params, table_params=table_params)
    for d, pg in zip(out, processed):
        d["round_marks"] = rounds_of_ink(ink_mask(pg, mp["threshold"]), mp["min_side"], mp["max_side"], rp)
    return out, processed


def page_result(d: dict, page_number: int = 1, snap: int = arch.TABLE_PARAMS["snap"], first_table_index: int = 0):
    """One restated page -> (layout_boxes, markdown, marks) the way the provider builds them with LUMINA_OCR_RADIO_BUTTONS=1."""
    from lumina_ocr.utils import layout, marks, tables
    triples = [(d["quads"][i].tolist(), d["texts"][i], float(d["scores"][i])) for i in range(len(d["texts"]))]
    merged, ordered = layout.reading_order(triples)
    tabs = []
    if "hrules" in d:
        tabs = tables.find_tables(d["hrules"], d["vrules"], snap)
        tables.fill_cells(tabs, ordered)
    found = marks.select_marks(d["marks"], d["round_marks"])
    boxes = (layout.build_layout_boxes(ordered, page_number) + layout.build_mark_boxes(found, page_number)
             + layout.build_table_boxes(tabs, page_number, first_table_index) + layout.build_paragraph_boxes(merged, page_number))
    return boxes, layout.page_markdown(merged, tabs, marks=found), found
