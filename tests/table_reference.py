"""Restatement (test infrastructure, numpy) of the rule extraction that lumina_ocr_table_rules runs on the device, as a sequential
definition: ink mask -> per-line runs merged across gaps -> components of runs over adjacent lines -> rules, in canonical order.
Plus the restated pipeline with tables (oracle.pipeline + this module + lumina_ocr.utils.tables) the provider is compared with."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr import arch

P = arch.TABLE_PARAMS


def ink_mask(page: np.ndarray, threshold: int = P["threshold"]) -> np.ndarray:
    """uint8 [H,W,3] -> bool [H,W]: L < threshold with L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's convert('L'))."""
    p = page.astype(np.int64)
    grey = (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16
    return grey < threshold


def pack_mask(ink: np.ndarray) -> np.ndarray:
    """bool [H,W] -> uint64 [H, ceil(W/64)]: bit x % 64 of word x // 64; bits past W are 0."""
    h, w = ink.shape
    nw = (w + 63) // 64
    padded = np.zeros((h, nw * 64), np.uint64)
    padded[:, :w] = ink
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(h, nw, 64) * weights).sum(axis=2, dtype=np.uint64)


def kept_runs(ink: np.ndarray, gap: int, min_len: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """bool [R,C] -> (line, start, end) of the kept runs, in raster order: the maximal ink runs of each line, merged while at most `gap`
    non-ink positions apart, kept when end - start + 1 >= min_len."""
    r, c = ink.shape
    z = np.zeros((r, 1), np.int8)
    d = np.diff(np.concatenate([z, ink.astype(np.int8), z], axis=1), axis=1)
    ls, s = np.nonzero(d == 1)
    le, e = np.nonzero(d == -1)
    e = e - 1
    assert np.array_equal(ls, le)
    if len(s) == 0:
        return ls, s, e
    new = np.ones(len(s), bool)
    new[1:] = (ls[1:] != ls[:-1]) | (s[1:] - e[:-1] - 1 > gap)
    first = np.nonzero(new)[0]
    last = np.append(first[1:], len(s)) - 1
    line, s, e = ls[first], s[first], e[last]
    keep = e - s + 1 >= min_len
    return line[keep], s[keep], e[keep]


def rules_one_direction(ink: np.ndarray, gap: int, min_len: int, max_thick: int) -> List[Tuple[int, int, int, int, int]]:
    """bool [R,C] (lines x positions) -> rules as (line0, pos0, line1, pos1, area), sorted by that tuple (ties: first run in raster order)."""
    line, s, e = kept_runs(ink, gap, min_len)
    n = len(line)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    start_of = {}
    for i in range(n):
        start_of.setdefault(int(line[i]), i)
    for i in range(n):
        j = start_of.get(int(line[i]) - 1)
        if j is None:
            continue
        while j < n and line[j] == line[i] - 1:
            if s[j] <= e[i] and s[i] <= e[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            j += 1
    comps = {}
    for i in range(n):
        r = find(i)
        c = comps.setdefault(r, [int(line[i]), int(s[i]), int(line[i]), int(e[i]), 0])
        c[1] = min(c[1], int(s[i])); c[2] = max(c[2], int(line[i])); c[3] = max(c[3], int(e[i])); c[4] += int(e[i] - s[i] + 1)
    out = []
    for r in sorted(comps):
        l0, p0, l1, p1, area = comps[r]
        length = p1 - p0 + 1
        if length >= min_len and area <= max_thick * length:
            out.append((l0, p0, l1, p1, area, r))
    out.sort()
    return [t[:5] for t in out]


def table_rules(page: np.ndarray, threshold: int = P["threshold"], gap: int = P["gap"], min_len: int = P["min_len"],
                max_thick: int = P["max_thick"]):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], hrules int32 [nh,5], vrules int32 [nv,5]) with rules as x0, y0, x1, y1, area;
    horizontal rules sorted by (y0, x0, y1, x1), vertical ones by (x0, y0, x1, y1)."""
    ink = ink_mask(page, threshold)
    hr = [(p0, l0, p1, l1, a) for l0, p0, l1, p1, a in rules_one_direction(ink, gap, min_len, max_thick)]
    vr = [(l0, p0, l1, p1, a) for l0, p0, l1, p1, a in rules_one_direction(np.ascontiguousarray(ink.T), gap, min_len, max_thick)]
    return pack_mask(ink), np.array(hr, np.int32).reshape(-1, 5), np.array(vr, np.int32).reshape(-1, 5)


def run_pages(det_w, rec_w, pages_u8: np.ndarray, charset, post=None, max_dim: int = 2000, params: dict = None):
    """The restated pipeline with tables: oracle.pipeline.run_pages, then the rules of every PROCESSED page (what the detector sees).
    -> (per page dict(quads, texts, scores, det_scores, hrules, vrules), processed)."""
    from oracle import pipeline as op
    tp = dict(P if params is None else params)
    out, processed = op.run_pages(det_w, rec_w, pages_u8, charset, post=post, max_dim=max_dim)
    for d, pg in zip(out, processed):
        _, d["hrules"], d["vrules"] = table_rules(pg, tp["threshold"], tp["gap"], tp["min_len"], tp["max_thick"])
    return out, processed


def page_result(d: dict, page_number: int = 1, snap: int = P["snap"], first_table_index: int = 0):
    """One restated page -> (layout_boxes, markdown, tables) the way the provider builds them."""
    from lumina_ocr.utils import layout, tables
    triples = [(d["quads"][i].tolist(), d["texts"][i], float(d["scores"][i])) for i in range(len(d["texts"]))]
    merged, ordered = layout.reading_order(triples)
    tabs = tables.find_tables(d["hrules"], d["vrules"], snap)
    tables.fill_cells(tabs, ordered)
    boxes = (layout.build_layout_boxes(ordered, page_number) + layout.build_table_boxes(tabs, page_number, first_table_index)
             + layout.build_paragraph_boxes(merged, page_number))
    return boxes, layout.page_markdown(merged, tabs), tabs
