"""Page builders (test infrastructure, numpy) for the regimes of the page-analysis entries that ordinary pages never enter: sides past
4096 pixels (a row of more than 64 mask words: the run kernels walk it in chunks of 64 words and carry one bit across each chunk
border), page groups with a remainder, components that stress the union-find and the accumulation at the root, and lists exactly at
and one past their capacity.  Shared by tests/test_page_analysis_edge_inputs.py (CPU: the restatements on these pages) and
tests/test_gpu_page_analysis_edges.py (GPU: the device against the restatements).

Everything is built as a bool ink array first (what the constructed counts are stated on) and turned into a page by page_of."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from lumina_ocr import synth

CHUNK = 4096                       # pixels in 64 mask words: the border a run kernel's chunk loop crosses
LONG_SHAPES = [(24, 4097), (24, 4160), (40, 8191), (12, 65535)]      # (short, long); every shape is also used transposed
FRAME_OFFSETS = (0, 1, 31, 63)     # a frame's left edge sits at CHUNK - k


def page_of(ink: np.ndarray, ink_value: int = 10) -> np.ndarray:
    """bool [..., H, W] -> uint8 [..., H, W, 3]: ink_value where ink, white elsewhere"""
    return np.repeat(np.where(ink[..., None], ink_value, 255).astype(np.uint8), 3, axis=-1)


def transposed(pages: np.ndarray) -> np.ndarray:
    """[n, H, W, ...] -> [n, W, H, ...], contiguous"""
    return np.ascontiguousarray(np.swapaxes(pages, 1, 2))


def draw_frame(ink: np.ndarray, x0: int, y0: int, side: int, stroke: int = 1) -> None:
    """a square frame with its first pixel at (x0, y0), cut by the page edges"""
    fr = np.zeros((side, side), bool)
    fr[:stroke], fr[-stroke:], fr[:, :stroke], fr[:, -stroke:] = True, True, True, True
    h, w = ink.shape
    ya, xa, yb, xb = max(0, y0), max(0, x0), min(h, y0 + side), min(w, x0 + side)
    if yb > ya and xb > xa:
        ink[ya:yb, xa:xb] |= fr[ya - y0:yb - y0, xa - x0:xb - x0]


# ---- long sides --------------------------------------------------------------------------------------------------------------------
def long_borders(w: int) -> List[int]:
    """the chunk borders a page of width w carries its features on: the first one, and on the longest page one in the middle and the last"""
    return [b for b in (CHUNK, 8 * CHUNK, 15 * CHUNK) if b < w]


def frame_side(h: int) -> int:
    """the frames of a long page: 20-30 pixels where the short side has room, the whole short side (12 = min_side) where it has not"""
    return 30 if h >= 40 else 20 if h >= 20 else h


def _row_features(w: int) -> List[np.ndarray]:
    """bool [w] rows, one feature each, the feature repeated at every border of long_borders(w) (clipped to the page)"""
    def row(spans):
        r = np.zeros(w, bool)
        for b in long_borders(w):
            for lo, hi, step in spans:
                r[max(0, b + lo):min(w, b + hi + 1):step] = True
        return r
    rows = [row([(-96, -1, 1)]),                  # a run ending at 4095
            row([(0, 103, 1)]),                   # a run starting at 4096
            row([(-6, 5, 1)]),                    # a run spanning 4090..4101
            row([(-1, -1, 1)]),                   # single pixels at 4095 ...
            row([(0, 0, 1)]),                     # ... at 4096 ...
            np.zeros(w, bool),                    # ... and at W - 1 (with one at 0)
            np.ones(w, bool),                     # a full row: one run of W pixels
            row([(-32, 32, 2)]),                  # alternating pixels across the border, even phase
            row([(-31, 33, 2)]),                  # and odd phase
            row([(-96, 103, 1)]),                 # a rule >= min_len crossing the border
            row([(-64, -1, 1), (1, 64, 1)]),      # two runs one blank pixel (4096) apart: merged by a gap >= 1, ends at 4095, starts at 4097
            row([(-64, -2, 1), (0, 64, 1)])]      # the blank pixel at 4095
    rows[5][[0, w - 1]] = True
    rows.append(np.zeros(w, bool))
    rows[-1][max(0, w - 80):] = True              # a rule ending at W - 1
    return rows


def long_inks(h: int, w: int) -> Tuple[np.ndarray, List[Tuple[int, int, int, int, int]]]:
    """-> (bool [n, h, w], frames): the run features on every other row (as many pages as that takes), then one page per frame offset
    k with frames of frame_side(h) at border - k for every border, then a page with a frame ending at W - 1.
    frames lists (page, x0, y0, x1, y1) of every frame that lies whole on its page."""
    feats = _row_features(w)
    per_page = h // 2
    pages = []
    for i0 in range(0, len(feats), per_page):
        ink = np.zeros((h, w), bool)
        for j, r in enumerate(feats[i0:i0 + per_page]):
            ink[2 * j] = r
        pages.append(ink)
    s = frame_side(h)
    frames = []
    for k in FRAME_OFFSETS + (None,):
        ink = np.zeros((h, w), bool)
        for x0 in ([b - k for b in long_borders(w)] if k is not None else [w - s]):
            draw_frame(ink, x0, 0, s)
            if x0 + s <= w:
                frames.append((len(pages), x0, 0, x0 + s - 1, s - 1))
        if h >= s + 4:                            # room under the frames: a 2-pixel rule across every border, one blank row below them
            for b in long_borders(w):
                ink[s + 1:s + 3, b - 70:min(w, b + 70)] = True
        pages.append(ink)
    return np.stack(pages), frames


def long_prob_maps(hp: int = 32, wp: int = 4160) -> np.ndarray:
    """float32 [n, hp, wp] probability maps with blobs ending at, starting at and spanning the 4095 / 4096 border, specks on both
    sides of it, a full-width band and an alternating row (one map each side of the threshold: 0.9 in the blobs, 0.1 around them)"""
    feats = _row_features(wp)
    maps = []
    a = np.zeros((hp, wp), bool)                  # blobs 4 rows high
    for j, f in enumerate((feats[0], feats[1], feats[2], feats[9])):
        a[1 + 7 * j:5 + 7 * j] = f
    maps.append(a)
    b = np.zeros((hp, wp), bool)                  # 1-row features, two blank rows between them, and a 6-row full-width band
    for j, f in enumerate((feats[3], feats[4], feats[5], feats[7], feats[8], feats[10], feats[11])):
        b[3 * j] = f
    b[24:30] = True
    maps.append(b)
    c = np.zeros((hp, wp), bool)                  # blobs that touch only across the border, through a corner
    c[2:8, CHUNK - 40:CHUNK] = True
    c[8:14, CHUNK:CHUNK + 40] = True
    c[16:24, CHUNK - 2:CHUNK + 2] = True          # a 4-pixel-wide bar on the border
    c[26:31, wp - 30:wp] = True                   # and a blob ending at Wp - 1
    maps.append(c)
    return np.where(np.stack(maps), np.float32(0.9), np.float32(0.1))


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def ragged_pages(n: int = 7, h: int = 200, w: int = 300) -> np.ndarray:
    """uint8 [n, h, w, 3]: n different small pages with text, noise, rules of both directions and frames; page i carries i + 1 frames
    and i % 4 + 1 horizontal rules, so no two pages share their counts"""
    pages = []
    for i in range(n):
        pg = synth.synth_page(h, w, 50 + i, n_lines=2, noise=3.0)[0].copy()
        rng = np.random.default_rng(900 + i)
        ink = np.zeros((h, w), bool)
        for k in range(i + 1):                                                  # frames, on a row of their own at the bottom
            draw_frame(ink, 6 + 34 * k, h - 40 - (k & 1) * 3, 14 + 2 * k, 1 + (k & 1))
        for k in range(i % 4 + 1):                                              # horizontal rules
            ink[100 + 9 * k:102 + 9 * k + (k & 1), 20 + 5 * i:20 + 5 * i + 80 + 30 * k] = True
        ink[60:150, w - 12 - 3 * i:w - 10 - 3 * i] = True                       # a vertical rule
        dots = rng.integers(0, [h, w], (150, 2))
        ink[dots[:, 0], dots[:, 1]] = True
        pg[ink] = 20
        pages.append(pg)
    return np.stack(pages)


# ---- hard components ---------------------------------------------------------------------------------------------------------------
def spiral(h: int, w: int) -> np.ndarray:
    """bool [h, w]: a rectangular spiral, stroke 1 and gap 1, from the top-left corner inwards (one 8-connected component)"""
    ink = np.zeros((h, w), bool)
    y, x, dy, dx = 0, 0, 0, 1
    ink[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx             # the cell after the next one must be free too (gap of one)
            ok = 0 <= ny < h and 0 <= nx < w and not ink[ny, nx] and not (0 <= ay < h and 0 <= ax < w and ink[ay, ax])
            if ok:
                y, x = ny, nx
                ink[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy                      # turn right
        if not moved:
            break
    return ink


def serpentine(h: int, w: int) -> np.ndarray:
    """bool [h, w]: full rows two apart, joined at the right and the left end in turn (one component, a chain of h / 2 unions)"""
    ink = np.zeros((h, w), bool)
    ink[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        ink[y, w - 1 if k % 2 == 0 else 0] = True
    return ink


def comb(h: int, w: int, teeth: int) -> np.ndarray:
    """bool [h, w]: `teeth` teeth one blank column apart, joined by the last row only"""
    ink = np.zeros((h, w), bool)
    edges = np.linspace(0, w + 1, teeth + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        ink[:, a:b - 1] = True
    ink[h - 1] = True
    return ink


HARD_H, HARD_W = 160, 200
NESTED_AT, NESTED_SIDES = (20, 30), (40, 36, 32, 28, 24)      # five frames, each 2 pixels inside the one before
COMB_AT, COMB_SIDE, COMB_TEETH = (120, 90), 40, 6             # 5 blank columns of 40: the top strip still counts 35 = w - w // 8
ROW_FRAMES, ROW_FRAME_SIDE = 72, 12


def hard_inks() -> Dict[str, np.ndarray]:
    """name -> bool [HARD_H, HARD_W]"""
    out = {}
    out["spiral"] = np.zeros((HARD_H, HARD_W), bool)
    out["spiral"][3:154, 4:195] = spiral(151, 191)
    sm = np.zeros((HARD_H, HARD_W), bool)                     # spirals at marks scale, one per bit offset class, and mirrored ones
    sm[5:46, 10:51] = spiral(41, 41)
    sm[60:93, 50:83] = spiral(33, 33)[::-1]                   # (upside down: the first run is the spiral's END, the root moves late)
    sm[100:149, 120:169] = spiral(49, 49)[:, ::-1]
    out["small_spirals"] = sm
    out["serpentine"] = np.zeros((HARD_H, HARD_W), bool)
    out["serpentine"][2:155, 5:190] = serpentine(153, 185)
    sp = np.zeros((HARD_H, HARD_W), bool)
    sp[10:51, 100:141] = serpentine(41, 41)                   # marks scale, and its transpose (vertical strokes: 21 roots in the top row)
    sp[80:121, 30:71] = serpentine(41, 41).T
    out["small_serpentines"] = sp
    nest = np.zeros((HARD_H, HARD_W), bool)
    for k, s in enumerate(NESTED_SIDES):
        draw_frame(nest, NESTED_AT[0] + 2 * k, NESTED_AT[1] + 2 * k, s)
    out["nested"] = nest
    blobs = np.zeros((HARD_H, HARD_W), bool)
    blobs[10:70, HARD_W - 60:HARD_W] = True                   # reaches the page's right edge
    blobs[70:130, HARD_W - 120:HARD_W - 60] = True            # its top-right pixel touches the first blob's bottom-left one
    out["diagonal_blobs"] = blobs
    cb = np.zeros((HARD_H, HARD_W), bool)
    cb[COMB_AT[1]:COMB_AT[1] + COMB_SIDE, COMB_AT[0]:COMB_AT[0] + COMB_SIDE] = comb(COMB_SIDE, COMB_SIDE, COMB_TEETH)
    cb[10:50, 10:50] = comb(40, 40, 20)                       # 1-pixel teeth: a candidate whose top strip fails the frame test
    out["combs"] = cb
    return out


def row_of_frames_ink(n: int = ROW_FRAMES, side: int = ROW_FRAME_SIDE, w: int = 1200, h: int = 40) -> np.ndarray:
    """bool [h, w]: n frames whose tops share row 5 (n roots in one row of the run list)"""
    ink = np.zeros((h, w), bool)
    for k in range(n):
        draw_frame(ink, 8 + 16 * k, 5, side)
    assert 8 + 16 * (n - 1) + side <= w
    return ink


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
def marks_grid_ink(n: int, side: int = 12, pitch: int = 15, size: int = 700) -> np.ndarray:
    """bool [size, size]: n frames of `side` on a `pitch` grid, filled in raster order (46 of them share every y0)"""
    per_row = (size - 5) // pitch
    assert n <= per_row * per_row
    ink = np.zeros((size, size), bool)
    for k in range(n):
        draw_frame(ink, 3 + pitch * (k % per_row), 3 + pitch * (k // per_row), side)
    return ink


RULE_PARAMS = dict(threshold=128, gap=0, min_len=8, max_thick=2, max_rules=2048)


def rules_grid_ink(n: int, length: int = 8, per_row: int = 64) -> np.ndarray:
    """bool [H, 650]: n horizontal rules of `length` x 1 on a grid of 10 x 2 pixels, filled in raster order: 64 rules share every y0
    and a column of them shares every x0.  Under RULE_PARAMS (gap 0) the columns hold runs of 1 only, so there are no vertical rules."""
    rows = (n + per_row - 1) // per_row
    ink = np.zeros((2 * rows + 3, per_row * 10 + 10), bool)
    for k in range(n):
        y, x = 1 + 2 * (k // per_row), 3 + 10 * (k % per_row)
        ink[y, x:x + length] = True
    return ink
