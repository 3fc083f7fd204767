"""Page builders (test infrastructure, numpy and Pillow) for the regimes of the barcode and QR passes that their own test files never
enter: sides past 4096 pixels (more than 64 mask words a row, run coordinates up to 65534 in the 16-bit run slots, QR modules sampled
at mask words past 64), page groups with a remainder, lists exactly at and one past their capacity (256 barcodes, 64 finders), pages
that are blank, all ink, grey at the threshold or noise, widths around the 64-pixel mask word with a symbol on either edge, and damaged
symbols: a pixel column of a barcode inverted, module widths that are no whole number of pixels, QR blocks with more wrong codewords
than the code corrects.  Shared by tests/test_code_edge_inputs.py (CPU: the restatements on these pages) and
tests/test_gpu_code_edges.py (GPU: the device against the restatements).

Every builder returns its pages with what was planted on them: {box: ...} as the `found` helpers of tests/test_gpu_barcodes.py and
tests/test_gpu_qrcodes.py return it."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

from page_edge_inputs import CHUNK, page_of, transposed  # noqa: F401  (transposed: re-exported for the two test files)

Box = Tuple[int, int, int, int]
BORDERS = (CHUNK, 8 * CHUNK, 15 * CHUNK)      # 4096, 32768, 61440: the chunk borders the long pages carry their symbols on


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def put_bar(page, x, y, text, kind="Code128", m=2, height=20, **kw) -> Box:
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    return synth.render_barcode(page, x, y, syms, kind, m, height, **kw)


def put_qr(page, x, y, text, version, level=1, mask=0, module=3, rotation=0, sym=None) -> Box:
    return synth.draw_qr(page, x, y, synth.qr_encode(text, version, level, mask) if sym is None else sym, module, rotation)


def turned_box(box: Box) -> Box:
    """a box of a page -> the box on the transposed page"""
    return box[1], box[0], box[3], box[2]


def rot90_box(box: Box, w: int) -> Box:
    """a box of a page of width w -> the box on np.rot90(page) (a quarter turn counter-clockwise: column x becomes row w - 1 - x)"""
    return box[1], w - 1 - box[2], box[3], w - 1 - box[0]


# ---- long sides --------------------------------------------------------------------------------------------------------------------
BARCODE_LONG_SHAPES = [(40, 8191), (12, 65535)]      # (short, long); each is also used transposed


def barcode_long_page(h: int, w: int) -> Tuple[np.ndarray, Dict[Box, Tuple[str, int]]]:
    """-> (page [h,w,3], {box: (text, flags)}).  40 rows: a Code 128 read forwards in rows 10..29 and a reversed Code 39 in rows 0..8,
    both across x = 4096.  12 rows hold one strip of min_rows rows: a Code 128 across 4096, a reversed Code 39 across 32768, a reversed
    Code 128 across 61440 and a Code 128 that ends 164 pixels before the far edge (four reads: all the slots a row has)."""
    page, want = blank(h, w), {}
    if h >= 40:
        want[put_bar(page, 4000, 10, "BORDER-4096")] = ("BORDER-4096", 0)
        want[put_bar(page, 3900, 0, "C39-4096", "Code39", height=9, reversed=True)] = ("C39-4096", 1)
    else:
        want[put_bar(page, 4000, 1, "BORDER-4096", height=10)] = ("BORDER-4096", 0)
    if w > BORDERS[2]:
        y, ht = (10, 20) if h >= 40 else (1, 10)
        want[put_bar(page, BORDERS[1] - 101, y, "MID-32768", "Code39", height=ht, reversed=True)] = ("MID-32768", 1)
        want[put_bar(page, BORDERS[2] - 77, y, "Last-61440", m=3, height=ht, reversed=True)] = ("Last-61440", 1)
        want[put_bar(page, w - 300, y, "END", height=ht)] = ("END", 0)
    assert all(b[0] < c <= b[2] for b, c in zip(want, (CHUNK, CHUNK) if h >= 40 else BORDERS))
    return page, want


QR_LONG_V1 = [(BORDERS[0] - 30, "LEFT 4096", 0, 1, 1), (BORDERS[1] - 11, "mid 32768", 1, 6, 2), (BORDERS[2] - 50, "61440", 3, 3, 3)]   # x, text, level, mask, rotation


def qr_long_page(h: int, w: int) -> Tuple[np.ndarray, Dict[Box, str]]:
    """-> (page [h,w,3], {box: text}): version 1 symbols at 3 px across every chunk border of the page, one more whose last column is
    w - 2 (so its quiet zone leaves the page), each with a level, mask and rotation of its own."""
    page, want = blank(h, w), {}
    for (x, text, level, mask, rot), border in zip(QR_LONG_V1, BORDERS):
        if border < w:
            want[put_qr(page, x, 15, text, 1, level, mask, 3, rot)] = text
    want[put_qr(page, w - 1 - 63, 15, "far edge", 1, 2, 4, 3, 0)] = "far edge"
    return page, want


def qr_tall_v10_page() -> Tuple[np.ndarray, Dict[Box, str]]:
    """200 x 8191 (a version 10 symbol at 3 px is 171 rows high and does not fit the 96 rows of the other long pages): the symbol across
    x = 4096, nothing else on the page's first chunk border"""
    page, want = blank(200, 8191), {}
    text = "version ten across the border / " * 4
    want[put_qr(page, CHUNK - 80, 14, text, 10, 1, 2, 3, 1)] = text
    want[put_qr(page, 8191 - 1 - 63, 100, "far edge", 1, 2, 4, 3, 2)] = "far edge"
    return page, want


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
RAGGED_H, RAGGED_W = 262, 331


def ragged_pages(n: int = 7) -> Tuple[np.ndarray, List[Dict[Box, Tuple[str, int]]], List[Dict[Box, str]]]:
    """-> (pages [n,262,331,3], barcodes planted per page, QR symbols planted per page): every page its own texts and positions, page 3
    blank, page 5 with three barcodes and three QR symbols (the most), every other page one of each."""
    pages, bars, qrs = np.stack([blank(RAGGED_H, RAGGED_W) for _ in range(n)]), [], []
    for i, page in enumerate(pages):
        b, q = {}, {}
        if i != 3:
            q[put_qr(page, 12 + 9 * i, 10 + 2 * i, "QR PAGE %d" % i, 1 + i % 2, i % 4, i, 3, i % 4)] = "QR PAGE %d" % i
            b[put_bar(page, 15 + 4 * i, 200 + 3 * i, "BAR-%d" % i, "Code39" if i % 3 == 2 else "Code128", height=12 + i, reversed=bool(i & 1))] = \
                ("BAR-%d" % i, i & 1)
        if i == 5:
            q[put_qr(page, 150, 8, "second on five", 2, 2, 7, 3, 2)] = "second on five"
            q[put_qr(page, 245, 10, "3RD", 1, 3, 0, 4, 3)] = "3RD"
            b[put_bar(page, 20, 110, "five-two", height=14)] = ("five-two", 0)
            b[put_bar(page, 20, 140, "55555", "Code39", height=20)] = ("55555", 0)
        bars.append(b)
        qrs.append(q)
    return pages, bars, qrs


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
BAR_GRID_W, BAR_GRID_PITCH = 328, (80, 13)


def barcode_grid_page(n: int) -> Tuple[np.ndarray, Dict[Box, Tuple[str, int]]]:
    """n one-character Code 128 strips, module 1 px (46 px long), 10 rows high, four a row on a pitch of 80 x 13, filled in raster
    order -> (page [13 rows + 6, 328, 3], {box: (text, 0)}).  256 strips make a page of 838 x 328, 257 one of 851 x 328; every row of
    the page that reads holds four reads, as many as a row has slots."""
    rows = -(-n // 4)
    page, want = blank(13 * rows + 6, BAR_GRID_W), {}
    for k in range(n):
        text = chr(33 + k % 90)
        want[put_bar(page, 4 + BAR_GRID_PITCH[0] * (k % 4), 3 + BAR_GRID_PITCH[1] * (k // 4), text, m=1, height=10)] = (text, 0)
    return page, want


QR_GRID_SIDE, QR_GRID_SYMBOLS = 470, 21


def qr_grid_page(lone_finders: int) -> Tuple[np.ndarray, Dict[Box, str]]:
    """470 x 470: 21 version 1 symbols at 3 px on a 5 x 5 grid of pitch 90, masks, levels and rotations mixed, and lone finder
    patterns in the cells behind them -> (page, {box: text}).  63 + lone_finders finders."""
    page, want = blank(QR_GRID_SIDE, QR_GRID_SIDE), {}
    for k in range(QR_GRID_SYMBOLS):
        text = "CELL %02d" % k
        want[put_qr(page, 10 + 90 * (k % 5), 10 + 90 * (k // 5), text, 1, k % 4, 3 * k % 8, 3, k // 5 % 4)] = text
    for k in range(QR_GRID_SYMBOLS, QR_GRID_SYMBOLS + lone_finders):
        synth.qr_finder(page, 10 + 90 * (k % 5) + 21, 10 + 90 * (k // 5) + 21, 3)
    return page, want


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
def flat_pages(h: int = 100, w: int = 200) -> np.ndarray:
    """[4,h,w,3]: blank, all ink, grey 127 (ink at the threshold of 128) and grey 128 (not ink)"""
    return np.stack([np.full((h, w, 3), v, np.uint8) for v in (255, 0, 127, 128)])


NOISE_DENSITIES = (0.02, 0.2, 0.5)


def noise_pages(h: int = 200, w: int = 333) -> np.ndarray:
    """[3,h,w,3]: every pixel ink with probability 0.02, 0.2, 0.5 (seeded)"""
    return page_of(np.stack([np.random.default_rng(7000 + k).random((h, w)) < d for k, d in enumerate(NOISE_DENSITIES)]))


EDGE_WIDTHS = (63, 64, 65, 127, 128, 129, 191)


def edge_width_pages(w: int, h: int = 100) -> Tuple[np.ndarray, List[Dict[Box, Tuple[str, int]]], List[Dict[Box, str]]]:
    """-> (pages [2,h,w,3], barcodes planted per page, QR symbols planted per page).  A version 1 symbol at 3 px is 63 pixels high, so
    a page of 100 rows holds one: page 0 has the symbol that starts at column 0 and a Code 128 whose last bar is column w - 1, page 1
    the symbol whose last module is column w - 1 and a (reversed) Code 128 that starts at column 0."""
    pages = np.stack([blank(h, w), blank(h, w)])
    qrs = [{put_qr(pages[0], 0, 2, "LEFT %d" % w, 1, 1, w % 8, 3, 0): "LEFT %d" % w},
           {put_qr(pages[1], w - 63, 30, "RIGHT %d" % w, 1, 2, (w + 3) % 8, 3, 3): "RIGHT %d" % w}]
    bars = [{put_bar(pages[0], w - 46, 74, "R", m=1, height=16): ("R", 0)},
            {put_bar(pages[1], 0, 4, "L", m=1, height=16, reversed=True): ("L", 1)}]
    return pages, bars, qrs


# ---- damage ------------------------------------------------------------------------------------------------------------------------
DAMAGE_STRIPS = [("Lumina-128", "Code128", 2), ("12345678", "Code128", 2), ("C39-X", "Code39", 2), ("AB12cd", "Code128", 3)]
STRIP_MARGIN, STRIP_ROWS = 15, 10


def strip_ink(text: str, kind: str, m: int) -> Tuple[np.ndarray, int, int]:
    """-> (bool [STRIP_ROWS, length + 30]: the strip with 15 blank pixels either side, over the page's full height; its first column;
    its length)"""
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    length = synth.barcode_length(syms, kind, m)
    page = blank(STRIP_ROWS, length + 2 * STRIP_MARGIN)
    synth.render_barcode(page, STRIP_MARGIN, 0, syms, kind, m, STRIP_ROWS)
    return page[:, :, 0] < 128, STRIP_MARGIN, length


def column_flips(ink: np.ndarray, x0: int, length: int, width: int = 1, step: int = 1) -> np.ndarray:
    """-> bool [n, H, W]: copy k has the `width` columns from x0 + k * step * width inverted over the full height"""
    starts = range(x0, x0 + length - width + 1, step * width)
    out = np.repeat(ink[None], len(starts), axis=0)
    for k, x in enumerate(starts):
        out[k, :, x:x + width] ^= True
    return out


RESCALE_FACTORS = (0.75, 0.625, 0.5)


def rescaled(page: np.ndarray, factor: float) -> np.ndarray:
    """the page reduced by `factor` with Lanczos: grey edges, module widths that are no whole number of pixels"""
    h, w = page.shape[:2]
    return np.array(Image.fromarray(page).resize((int(round(w * factor)), int(round(h * factor))), Image.LANCZOS), np.uint8)


RESCALE_BAR_TEXT, RESCALE_QR_TEXT = "Lumina-128", "rescaled QR 2-M"


def rescale_sources() -> Tuple[np.ndarray, np.ndarray]:
    """-> (a Code 128 at 4 px a module on 96 x 720, a 2-M symbol at 8 px a module on 320 x 320): both sides multiples of 8, so that every
    factor gives a whole page size"""
    bar, sym = blank(96, 720), blank(320, 320)
    put_bar(bar, 64, 24, RESCALE_BAR_TEXT, m=4, height=48)
    put_qr(sym, 56, 64, RESCALE_QR_TEXT, 2, 1, 2, 8, 0)
    return bar, sym


# the blocks that get more wrong codewords than they correct: (version, level, block, text)
RS_SYMBOLS = [(1, 0, 0, "one-L"), (1, 3, 0, "one-H"), (2, 1, 0, "two-M block"), (5, 2, 1, "five-Q corrected " * 3),
              (10, 3, 7, "ten-H " + "error correction " * 5)]
RS_EXTRA = (-1, 0, 1, 2, 4)        # wrong codewords relative to t = ec // 2
RS_SEEDS = 6


def rs_corrupted(text: str, version: int, level: int, mask: int, block: int, wrong: int, seed: int) -> np.ndarray:
    """the symbol with `wrong` codewords of one block (data and check codewords alike) at seeded positions changed by seeded non-zero
    values, as corrupted() of tests/test_gpu_qrcodes.py changes the block's first ones"""
    cw = synth.qr_interleave(synth.qr_data_codewords(text, version, level), version, level)
    nb, short, dlen, ec = qr.block_structure(version, level)
    ndata = nb * dlen + (nb - short)
    at = [i * nb + block for i in range(dlen)] + ([dlen * nb + block - short] if block >= short else []) + [ndata + i * nb + block for i in range(ec)]
    rng = np.random.default_rng([version, level, wrong, seed])
    for p in rng.choice(len(at), wrong, replace=False):
        cw[at[int(p)]] ^= int(rng.integers(1, 256))
    return synth.qr_matrix(cw, version, level, mask)


def rs_pages(version: int, level: int, block: int, text: str) -> Tuple[np.ndarray, List[int], int]:
    """-> (pages [30, side, side + 5, 3], wrong codewords of every page, t): the symbol at 3 px with t - 1, t, t + 1, t + 2 and t + 4
    wrong codewords in `block`, six seeded patterns of each, on pages that hold it with 13 pixels around"""
    t = qr.block_structure(version, level)[3] // 2
    side = 3 * qr.dimension(version) + 26
    pages, wrong = [], []
    for extra in RS_EXTRA:
        for seed in range(RS_SEEDS):
            page = blank(side, side + 5)
            put_qr(page, 13, 13, "", version, module=3, rotation=seed % 4, sym=rs_corrupted(text, version, level, (seed + extra) % 8, block, t + extra, seed))
            pages.append(page)
            wrong.append(t + extra)
    return np.stack(pages), wrong, t
