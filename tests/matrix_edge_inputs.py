"""Page builders (test infrastructure, numpy and Pillow) for the regimes of the Data Matrix and Aztec passes that their own test files
never enter: sides past 4096 pixels (mask words past 63 in az_at and dm_sample, a centre row of many runs, extremes packed from
coordinates up to 65534, the largest symbol of either pass flush against column 65534), Reed-Solomon blocks with more wrong codewords
than the code corrects (the nearly empty 11-layer Aztec symbol whose locator spans three 64-lane chunks; either block of the two-block
52 x 52 Data Matrix), lists exactly at and one past their capacity (64 finders, 64 codes, 1024 candidates), ragged page groups, flat
pages, block noise, widths around the 64-bit mask word with a symbol on either edge, and module widths that are no whole pixels.
Shared by tests/test_matrix_edge_inputs.py (CPU: the restatements on these pages) and tests/test_gpu_matrix_code_edges.py (GPU: the
device against the restatements).

Every builder returns its pages with what was planted on them: {box: text} as the `found` helpers of tests/test_gpu_aztec.py and
tests/test_gpu_datamatrix.py return it."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm

import aztec_pages as AP
import code_edge_inputs as ce
import dm_pages as DP
from code_edge_inputs import BORDERS, EDGE_WIDTHS, RESCALE_FACTORS, blank, flat_pages, rescaled, rot90_box  # noqa: F401  (re-exported for the two test files)

Box = Tuple[int, int, int, int]


def turned(page: np.ndarray, want: Dict[Box, str]) -> Tuple[np.ndarray, Dict[Box, str]]:
    """the page and its boxes a quarter turn counter-clockwise (np.rot90): the long side becomes H.  (A transposed symbol is its mirror
    image and does not read.)"""
    w = page.shape[1]
    return np.ascontiguousarray(np.rot90(page)), {rot90_box(b, w): t for b, t in want.items()}


# ---- long sides --------------------------------------------------------------------------------------------------------------------
LONG_SHAPES = [(96, 8191), (200, 65535)]          # (short, long); each is also used turned
AZ_LARGEST, DM_LARGEST = (False, 11), 14          # 61 x 61 modules, 52 x 52 modules: at 3 px 183 and 156 pixels
AZ_TICK_ROWS = (26, 31)                           # rows 26 .. 30: row 28 is the centre row of the core of the symbol drawn at y = 6


def aztec_long_page(h: int, w: int) -> Tuple[np.ndarray, Dict[Box, str]]:
    """-> (page [h,w,3], {box: text}): a compact 1-layer symbol across x = 4096; on the longest page also a compact 2-layer one across
    32768, a full 1-layer one across 61440 and the largest symbol (full, 11 layers) turned 180 degrees with its last column the page's,
    65534.  Every symbol has its own text and rotation.  On the longest page the centre row of the first symbol's core is a long row:
    about 8000 ticks left and right of the symbol, so that the finder kernel's binary search for the core's run takes 13 steps."""
    page, want = blank(h, w), {}
    want[AP.put(page, BORDERS[0] - 20, 6, "AZ 4096", True, 1, 3, 1)] = "AZ 4096"
    if w > BORDERS[2]:
        want[AP.put(page, BORDERS[1] - 20, 100, "Aztec, mid 32768", True, 2, 3, 3)] = "Aztec, mid 32768"
        want[AP.put(page, BORDERS[2] - 30, 40, "61440 full", False, 1, 3, 0)] = "61440 full"
        text = AP.payload(*AZ_LARGEST, "FAR EDGE ")
        want[AP.put(page, w - AP.side_px(*AZ_LARGEST), 2, text, *AZ_LARGEST, 3, 2)] = text
        for x in range(100, 32000, 4):                       # ticks of 2 x 5 px (too thin for a core) on the first symbol's centre row
            if not BORDERS[0] - 32 <= x < BORDERS[0] + 40:
                page[AZ_TICK_ROWS[0]:AZ_TICK_ROWS[1], x:x + 2] = 0
    assert all(b[0] < c <= b[2] for b, c in zip(want, BORDERS))
    return page, want


def dm_long_page(h: int, w: int) -> Tuple[np.ndarray, Dict[Box, str]]:
    """-> (page [h,w,3], {box: text}): an 18 x 18 symbol across x = 4096; on the longest page also a 12 x 26 one across 32768, a
    20 x 20 one across 61440 and the largest symbol (52 x 52) turned 180 degrees, so that its elbow is its top right corner, with its
    last column the page's, 65534: the largest term of dm_sample.  Every symbol has its own text and rotation."""
    page, want = blank(h, w), {}
    want[DP.put(page, BORDERS[0] - 20, 20, "DM ACROSS 4096", 4, 3, 1)] = "DM ACROSS 4096"
    if w > BORDERS[2]:
        want[DP.put(page, BORDERS[1] - 33, 120, "rect 32768", 17, 3, 0)] = "rect 32768"
        want[DP.put(page, BORDERS[2] - 7, 60, "twenty at 61440", 5, 3, 3)] = "twenty at 61440"
        text = DP.payload(DM_LARGEST, "FAR EDGE ")
        want[DP.put(page, w - 3 * dm.SIZES[DM_LARGEST][1], 2, text, DM_LARGEST, 3, 2)] = text
    assert all(b[0] < c <= b[2] for b, c in zip(want, BORDERS))
    return page, want


# ---- Reed-Solomon beyond the capacity ----------------------------------------------------------------------------------------------
RS_EXTRA, RS_SEEDS = ce.RS_EXTRA, ce.RS_SEEDS     # t - 1, t, t + 1, t + 2, t + 4 wrong codewords; six seeded patterns of each
# (compact, layers, text): the smallest and the largest symbol of every codeword width three quarters full, and three nearly empty
# symbols with the shortest text the encoder accepts: t = 156 (the locator spans three chunks of 64 lanes), 118 and 37
AZ_RS_SYMBOLS = [(c, n, AP.payload(c, n)) for c, n in AP.WIDTH_ENDS] + [(False, 11, "SHORT"), (False, 8, "SHORT"), (True, 4, "S")]


def az_rs_id(symbol) -> str:
    return "%s%d_%s" % ("compact" if symbol[0] else "full", symbol[1], "short" if len(symbol[2]) <= 5 else "filled")


def az_rs_pages(compact: bool, layers: int, text: str) -> Tuple[np.ndarray, List[int], int]:
    """-> (pages [30, side, side + 3, 3], wrong codewords of every page, t): the symbol at 3 px with t - 1 .. t + 4 of its codewords
    destroyed by aztec_pages.corrupted, seeds 0 .. 5, every seed its own rotation"""
    t = AP.capacity(compact, layers, text)
    s = AP.side_px(compact, layers) + 16
    pages, wrong = [], []
    for extra in RS_EXTRA:
        for seed in range(RS_SEEDS):
            page = blank(s, s + 3)
            AP.put(page, 9, 8, "", compact, layers, 3, seed % 4, matrix=AP.corrupted(text, compact, layers, t + extra, seed))
            pages.append(page)
            wrong.append(t + extra)
    return np.stack(pages), wrong, t


# (size, the block whose count varies, text): 10 x 10 (t = 2), 26 x 26, 48 x 48 (t = 34, the largest ec), 52 x 52 (two blocks of
# t = 21; the other block has exactly t wrong) and the 16 x 48 rectangle
DM_RS_SYMBOLS = [(0, 0, "1234"), (8, 0, DP.payload(8)), (13, 0, DP.payload(13)), (14, 0, DP.payload(14)), (14, 1, DP.payload(14)), (20, 0, DP.payload(20))]


def dm_rs_id(symbol) -> str:
    return "%dx%d_block%d" % (dm.SIZES[symbol[0]][:2] + (symbol[1],))


def dm_corrupted(text: str, size: int, wrong: Tuple[int, ...], seed: int) -> np.ndarray:
    """the symbol with wrong[b] codewords of block b (data and check codewords alike) at seeded positions changed by seeded non-zero
    values"""
    cw = synth.dm_interleave(synth.dm_data_codewords(text, size), size)
    ndata, ncheck, nb = dm.SIZES[size][2], dm.SIZES[size][3], dm.SIZES[size][6]
    assert len(wrong) == nb
    rng = np.random.default_rng([size, seed] + list(wrong))
    for b, n in enumerate(wrong):
        at = list(range(b, ndata, nb)) + list(range(ndata + b, ndata + ncheck, nb))
        for p in rng.choice(len(at), n, replace=False):
            cw[at[int(p)]] ^= int(rng.integers(1, 256))
    return synth.dm_matrix(cw, size)


def dm_rs_pages(size: int, block: int, text: str) -> Tuple[np.ndarray, List[int], int]:
    """-> (pages [30, ...], wrong codewords of `block` on every page, t): the symbol at 3 px with t - 1 .. t + 4 wrong codewords in
    `block` and, in a two-block size, exactly t in the other block; seeds 0 .. 5, every seed its own rotation"""
    rows, cols, _, ncheck, _, _, nb = dm.SIZES[size]
    t = ncheck // nb // 2
    s = 3 * max(rows, cols) + 26
    pages, wrong = [], []
    for extra in RS_EXTRA:
        for seed in range(RS_SEEDS):
            page = blank(s, s + 5)
            counts = tuple(t + extra if b == block else t for b in range(nb))
            DP.put(page, 13, 13, "", size, 3, seed % 4, sym=dm_corrupted(text, size, counts, seed))
            pages.append(page)
            wrong.append(t + extra)
    return np.stack(pages), wrong, t


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
AZ_GRID_SHAPE, DM_GRID_SHAPE, DM_SQUARES_SHAPE = (424, 484), (328, 378), (998, 938)


def aztec_grid_page(lone: int = 0) -> Tuple[np.ndarray, Dict[Box, str]]:
    """424 x 484: 64 compact 1-layer symbols at 3 px on an 8 x 8 grid of pitch 60 x 53, rotations cycling, and `lone` bullseyes of
    five modules (a core and one ring: a finder and no symbol) in the margin right of the grid -> (page, {box: text}).
    64 + lone finders."""
    page, want = blank(*AZ_GRID_SHAPE), {}
    for k in range(64):
        text = "Cell %02d" % k
        want[AP.put(page, 2 + 60 * (k % 8), 2 + 53 * (k // 8), text, True, 1, 3, (k + k // 8) % 4)] = text
    for k in range(lone):
        AP.bullseye(page, 468, 10 + 53 * k, 2, 3)
    return page, want


def dm_grid_page() -> Tuple[np.ndarray, Dict[Box, str]]:
    """328 x 378: 64 symbols of 10 x 10 at 3 px on an 8 x 8 grid of pitch 47 x 41, rotations cycling -> (page, {box: text})"""
    page, want = blank(*DM_GRID_SHAPE), {}
    for k in range(64):
        text = "%c%02d" % (65 + k % 26, k)
        want[DP.put(page, 2 + 47 * (k % 8), 2 + 41 * (k // 8), text, 0, 3, (k + k // 8) % 4)] = text
    return page, want


DM_SQUARES_TEXT = "BEHIND 1023"


def dm_squares_page(squares: int) -> Tuple[np.ndarray, Dict[Box, str]]:
    """998 x 938: `squares` solid squares of 24 px, 29 a row on a pitch of 32 x 26, above one 16 x 16 symbol -> (page, {box: text}).
    Every square is a candidate and so is the symbol: squares + 1 candidates, the symbol's the last root of the page."""
    page = blank(*DM_SQUARES_SHAPE)
    for i in range(squares):
        y, x = 5 + 26 * (i // 29), 8 + 32 * (i % 29)
        page[y:y + 24, x:x + 24] = 0
    assert 5 + 26 * ((squares - 1) // 29) + 24 < 942
    return page, {DP.put(page, 150, 945, DM_SQUARES_TEXT, 3, 3): DM_SQUARES_TEXT}


DM_MANY_SHAPE, DM_MANY_SYMBOLS, DM_MANY_SQUARES = (1192, 1156), 600, 423


def dm_many_symbols_page(extra: int = 0) -> np.ndarray:
    """1192 x 1156, cells of 36 px, 32 a row: 600 symbols of 10 x 10 at 3 px (601 candidates: one symbol is two components), then
    423 + extra solid squares of 24 px: 1024 + extra candidates of which more than half read.  The slot a candidate gets in the device's list is the scheduler's
    choice, so a decode that served only a part of the 1024 slots could still reach the one symbol of dm_squares_page; here it
    cannot reach all 600, and the count shows it (600 symbols overflow every list: the count is all that is reported)."""
    page = blank(*DM_MANY_SHAPE)
    for k in range(DM_MANY_SYMBOLS + DM_MANY_SQUARES + extra):
        x, y = 3 + 36 * (k % 32), 3 + 36 * (k // 32)
        if k < DM_MANY_SYMBOLS:
            DP.put(page, x, y, "%03d" % k, 0, 3, 0)
        else:
            page[y:y + 24, x:x + 24] = 0
    return page


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
RAGGED_H, RAGGED_W = 150, 331


def ragged_pages(n: int = 7) -> Tuple[np.ndarray, List[Dict[Box, str]], List[Dict[Box, str]]]:
    """-> (pages [n,150,331,3], Aztec symbols planted per page, Data Matrix symbols planted per page): every page its own texts, sizes
    and positions, page 3 blank, page 5 with three symbols of either kind (the most), every other page one of each."""
    pages, azs, dms = np.stack([blank(RAGGED_H, RAGGED_W) for _ in range(n)]), [], []
    for i, page in enumerate(pages):
        a, d = {}, {}
        if i != 3:
            a[AP.put(page, 8 + 5 * i, 6 + 2 * i, "AZ PAGE %d" % i, i % 2 == 0, 1 + i % 2, 3, i % 4)] = "AZ PAGE %d" % i
            d[DP.put(page, 90 + 4 * i, 80 + i, "DM PAGE %d" % i, 3 + i % 3, 3, (i + 1) % 4)] = "DM PAGE %d" % i
        if i == 5:
            a[AP.put(page, 120, 4, "second on five", True, 2, 3, 2)] = "second on five"
            a[AP.put(page, 200, 8, "3RD", False, 1, 3, 3)] = "3RD"
            d[DP.put(page, 200, 90, "five-two", 3, 3)] = "five-two"
            d[DP.put(page, 270, 70, "55555", 15, 3, 1)] = "55555"
        azs.append(a)
        dms.append(d)
    return pages, azs, dms


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
NOISE_CELLS = [(3, 0.2), (3, 0.5), (5, 0.2), (5, 0.5), (8, 0.2), (8, 0.5)]      # (cell side in pixels, density)
NOISE_H, NOISE_W = 200, 333


def block_noise_ink(cell: int, density: float, seed: int) -> np.ndarray:
    """bool [200,333]: cells of cell x cell pixels, each ink with probability `density` (seeded).  (Pixel noise gives neither pass a
    candidate: every component is too small or too sparse.)"""
    rng = np.random.default_rng(9000 + seed)
    cells = rng.random((-(-NOISE_H // cell), -(-NOISE_W // cell))) < density
    return np.kron(cells, np.ones((cell, cell), bool))[:NOISE_H, :NOISE_W]


def block_noise_pages() -> np.ndarray:
    """[6,200,333,3]: one page for every (cell, density) of NOISE_CELLS"""
    return ce.page_of(np.stack([block_noise_ink(c, d, k) for k, (c, d) in enumerate(NOISE_CELLS)]))


NOISY_BULLSEYES = 5


def noisy_bullseye_page() -> np.ndarray:
    """[200,333,3]: block noise of 3 px cells at density 0.2 and on it a row of five compact bullseyes at 3 px whose core and first
    three rings are clean (so the finder is found) while noise lies over the outer ring, the mode message and everything beyond."""
    ink = block_noise_ink(3, 0.2, 20)
    page = ce.page_of(ink)
    for k in range(NOISY_BULLSEYES):
        x, y = 21 + 63 * k, 60 + 6 * k
        page[y + 3:y + 24, x + 3:x + 24] = 255                                # distances 0 .. 3 are the bullseye's alone
        AP.bullseye(page, x, y, 4, 3)
    return page


def edge_width_pages(w: int, h: int = 100) -> Tuple[np.ndarray, List[Dict[Box, str]], List[Dict[Box, str]]]:
    """-> (pages [2,h,w,3], Aztec symbols planted per page, Data Matrix symbols planted per page).  Compact 1-layer Aztec (45 px) and
    12 x 12 Data Matrix (36 px) at 3 px: page 0 has the Aztec symbol that starts at column 0 and the Data Matrix symbol whose last
    column is w - 1, page 1 the other way round."""
    pages = np.stack([blank(h, w), blank(h, w)])
    azs = [{AP.put(pages[0], 0, 2, "LEFT %d" % w, True, 1, 3, w % 4): "LEFT %d" % w},
           {AP.put(pages[1], w - 45, 50, "RIGHT %d" % w, True, 1, 3, (w + 1) % 4): "RIGHT %d" % w}]
    dms = [{DP.put(pages[0], w - 36, 58, "R%d" % w, 1, 3, (w + 2) % 4): "R%d" % w},
           {DP.put(pages[1], 0, 4, "L%d" % w, 1, 3, (w + 3) % 4): "L%d" % w}]
    return pages, azs, dms


# module widths that are no whole pixels: (text, compact, layers) and (text, size)
RESCALE_AZ = [("rescaled compact 2", True, 2), ("Rescaled Aztec, full 3 layers.", False, 3)]
RESCALE_DM = [("rescaled 18 x 18", 4), ("rescaled 12 x 26", 17)]


def rescale_sources() -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """-> (Aztec pages, Data Matrix pages), one symbol each at 8 px a module: both sides of every page are multiples of 8, so that every
    factor gives a whole page size"""
    azs, dms = [], []
    for k, (text, compact, layers) in enumerate(RESCALE_AZ):
        page = blank(320, 320)
        AP.put(page, 48, 56, text, compact, layers, 8, 1 + k)
        azs.append(page)
    for k, (text, size) in enumerate(RESCALE_DM):
        page = blank(240, 320)
        DP.put(page, 56, 48, text, size, 8, 2 * k)
        dms.append(page)
    return azs, dms
