"""Restatement (test infrastructure, numpy) of the page orientation as a sequential definition:
  * sideways or not: ink profiles of the raw page and the energies of their differences (csrc/orient.hip behind lumina_ocr_page_quarter);
  * the vote of the line classifier (lumina_ocr_page_vote + lumina_ocr/utils/page_orient.py);
  * "oracle pipeline + page orientation": the turn of every page, then tests/cls_reference.py's run_pages on the upright page.
Convention: turn = t means the upright page is np.rot90(input_page, t)."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr import arch

import cls_reference as cr
import table_reference as tr

P = arch.PAGE_ORIENT_PARAMS


def profiles(page: np.ndarray, threshold: int = P["threshold"]) -> Tuple[np.ndarray, np.ndarray]:
    """uint8 [H,W,3] -> (r int64 [H], c int64 [W]): ink pixels of every row and of every column, ink as tb_mask defines it."""
    ink = tr.ink_mask(page, threshold)
    return ink.sum(axis=1, dtype=np.int64), ink.sum(axis=0, dtype=np.int64)


def energy(profile) -> int:
    """sum of the squared differences of neighbouring entries, as a Python integer"""
    return sum(int(d) * int(d) for d in np.diff(np.asarray(profile, np.int64)))


def energies(page: np.ndarray, threshold: int = P["threshold"]) -> Tuple[int, int]:
    r, c = profiles(page, threshold)
    return energy(r), energy(c)


def sideways_from(e_r: int, e_c: int, ratio: int = P["ratio"]) -> bool:
    return int(e_c) > int(ratio) * int(e_r)


def sideways(page: np.ndarray, threshold: int = P["threshold"], ratio: int = P["ratio"]) -> bool:
    return sideways_from(*energies(page, threshold), ratio)


def vote(flips, min_lines: int = P["min_lines"]) -> bool:
    """flip flags of a page's lines -> upside-down: at least min_lines lines, more than half of them flipped."""
    flips = list(flips)
    lines, flipped = len(flips), sum(1 for f in flips if f)
    return lines >= min_lines and 2 * flipped > lines


def vote_counts(flip, page_idx, pages: int) -> np.ndarray:
    """-> int32 [pages, 2]: lines per page, flipped lines per page (entries outside 0..pages-1 are not counted)"""
    out = np.zeros((pages, 2), np.int32)
    for f, p in zip(flip, page_idx):
        if 0 <= p < pages:
            out[p, 0] += 1
            out[p, 1] += 1 if f else 0
    return out


def run_pages(det_w, rec_w, cls_w, pages: List[np.ndarray], charset, post: dict = None, thresh: float = arch.CLS_THRESH, params: dict = None):
    """Every page on its own: quarter turn from the profiles, cls_reference.run_pages on the result, the vote on its flips, and for a
    page voted upside-down cls_reference.run_pages once more on the raw page turned by its total.
    -> list per page of dict(turn, quads, texts, scores, labels, cls_scores, flips, processed)."""
    pp = dict(P if params is None else params)
    out = []
    for page in pages:
        t = 1 if sideways(page, pp["threshold"], pp["ratio"]) else 0
        up = np.ascontiguousarray(np.rot90(page, t))
        res, processed = cr.run_pages(det_w, rec_w, cls_w, up[None], charset, post=post, thresh=thresh)
        if vote(res[0]["flips"], pp["min_lines"]):
            t += 2
            up = np.ascontiguousarray(np.rot90(page, t))
            res, processed = cr.run_pages(det_w, rec_w, cls_w, up[None], charset, post=post, thresh=thresh)
        out.append(dict(res[0], turn=t, processed=processed[0]))
    return out


def page_kinds():
    """The project's synthetic page kinds the statistic is stated for: name -> upright page uint8 [H,W,3]."""
    from lumina_ocr import synth
    h, w = synth.A4_200DPI
    return {
        "text_a4": synth.synth_page(h, w, 11)[0],
        "text_small": synth.synth_page(640, 896, 5, n_lines=12)[0],
        "text_3_lines": synth.synth_page(640, 896, 6, n_lines=3)[0],
        "ruled_a4": synth.synth_page(h, w, 12, ruled=True)[0],
        "ruled_small": synth.synth_page(640, 896, 3, n_lines=10, ruled=True)[0],
        "form": synth.synth_form_page(0)[0],
        "table_1": synth.synth_table_page(2, n_tables=1)[0],
        "table_2": synth.synth_table_page(3, h=1400, n_tables=2)[0],
        "marks": synth.synth_marks_page(1)[0],
        "text_landscape": synth.synth_page(w, h, 13, n_lines=40)[0],
    }
