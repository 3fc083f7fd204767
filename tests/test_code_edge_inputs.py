"""CPU: the restatements (tests/barcode_reference.py, tests/qr_reference.py) on the pages of tests/code_edge_inputs.py — inputs neither
had seen: sides past 4096, page groups, lists at their capacity, hard pages, damaged symbols.  The GPU file
(tests/test_gpu_code_edges.py) asserts that the device EQUALS the restatements on these pages; this file states what every page was
built to contain and shows that the restatements find exactly that, and it holds the property that matters most for a reader: a
damaged symbol reads as what was printed or not at all, never as something else."""
import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import qrcodes as qr

import barcode_reference as br
import code_edge_inputs as ce
import qr_reference as R

BP, QP = arch.BARCODE_PARAMS, arch.QR_PARAMS


def bars_of(page: np.ndarray, **kw):
    """-> {box: (text, flags)} of the barcode restatement"""
    _, rc, rs = br.barcodes(page, **kw)
    assert len({tuple(c[:4]) for c in rc.tolist()}) == len(rc)
    return {tuple(int(v) for v in c[:4]): (t, int(c[7])) for c, t in zip(rc, br.decoded(rc, rs))}


def qrs_of(page: np.ndarray, **kw):
    """-> ({box: text}, finders) of the QR restatement"""
    _, rc, rd, rf = R.qrcodes(page, **kw)
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}, rf


# ---- long sides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ce.BARCODE_LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_barcode_pages(shape):
    h, w = shape
    page, want = ce.barcode_long_page(h, w)
    assert bars_of(page) == want
    assert sum(b[0] < ce.CHUNK <= b[2] for b in want) == (2 if h >= 40 else 1) and {f for _, f in want.values()} == {0, 1}
    if h >= 40:
        assert want[(4000, 10, 4289, 29)] == ("BORDER-4096", 0)
    else:                                                   # a strip across every chunk border, and one 164 pixels before the far edge
        assert [any(b[0] < c <= b[2] for b in want) for c in ce.BORDERS] == [True] * 3
        assert max(want) == (65235, 1, 65370, 10) and want[max(want)] == ("END", 0) and w - 1 - 65370 < 200
    turned = ce.transposed(page[None])[0]                   # the codes are vertical: read from the transposed mask, H + W rows of slots
    assert turned.shape[:2] == (w, h)
    assert bars_of(turned) == {ce.turned_box(b): (t, f | 2) for b, (t, f) in want.items()}


def test_long_qr_pages():
    page, want = ce.qr_long_page(96, 65535)
    got, finders = qrs_of(page)
    assert got == want and finders == 12 and len(want) == 4 and max(want) == (65471, 15, 65533, 77)
    assert [b[0] < c <= b[2] for b, c in zip(sorted(want), ce.BORDERS)] == [True] * 3
    _, rc, _, _ = R.qrcodes(page)
    assert sorted(tuple(c[5:7]) + (c[9],) for c in rc.tolist()) == sorted([(lv, m, r) for _, _, lv, m, r in ce.QR_LONG_V1] + [(2, 4, 0)])
    got, finders = qrs_of(np.ascontiguousarray(np.rot90(page)))           # (a transposed symbol is its mirror image and does not read)
    assert got == {ce.rot90_box(b, 65535): t for b, t in want.items()} and finders == 12
    page, want = ce.qr_long_page(96, 8191)
    assert qrs_of(page) == (want, 6) and qrs_of(np.ascontiguousarray(np.rot90(page))) == ({ce.rot90_box(b, 8191): t for b, t in want.items()}, 6)


def test_version_ten_across_the_chunk_border():
    page, want = ce.qr_tall_v10_page()
    got, finders = qrs_of(page)
    assert got == want and finders == 6
    box = next(b for b, t in want.items() if t.startswith("version ten"))
    assert box[0] < ce.CHUNK < box[2] and box[2] - box[0] + 1 == 3 * 57 == box[3] - box[1] + 1    # all 57 rows of modules cross x = 4096
    assert qrs_of(np.ascontiguousarray(np.rot90(page)))[0] == {ce.rot90_box(b, 8191): t for b, t in want.items()}


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def test_ragged_pages_differ_and_hold_what_was_planted():
    pages, bars, qrs = ce.ragged_pages()
    assert pages.shape == (7, 262, 331, 3) and len({p.tobytes() for p in pages}) == 7
    for i, page in enumerate(pages):
        assert bars_of(page) == bars[i] and qrs_of(page) == (qrs[i], 3 * len(qrs[i])), i
    assert [len(b) for b in bars] == [len(q) for q in qrs] == [1, 1, 1, 0, 1, 3, 1]
    texts = [t for b in bars for t, _ in b.values()] + [t for q in qrs for t in q.values()]
    assert len(set(texts)) == len(texts) == 16


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_barcode_grid_pages(n):
    page, want = ce.barcode_grid_page(n)
    assert page.shape[:2] == {64: (214, 328), 65: (227, 328), 256: (838, 328), 257: (851, 328)}[n]
    assert bars_of(page) == want and len(want) == n
    assert BP["max_codes"] == 64 and br.ROW_READS == 4                    # (256, the other capacity, is the entry's own limit: max_codes 257 is refused)


@pytest.mark.parametrize("lone", [1, 2])
def test_qr_grid_pages(lone):
    page, want = ce.qr_grid_page(lone)
    assert page.shape[:2] == (470, 470) and len(want) == 21 and QP["max_finders"] == 64
    got, finders = qrs_of(page)
    assert finders == 63 + lone
    if lone == 1:
        assert got == want
    else:                                                                 # 65 finders: the page is not read; with room for 65 it is
        assert got == {}
        _, rc, rd, _ = R.qrcodes(page, max_finders=65)
        assert R.texts(rc, rd) == list(want.values())
        assert len({tuple(c[5:7]) + (c[9],) for c in rc.tolist()}) >= 16  # levels, masks and rotations are mixed


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
def test_flat_pages_hold_nothing():
    pages = ce.flat_pages()
    assert [int(p[0, 0, 0]) for p in pages] == [255, 0, 127, 128] and BP["threshold"] == QP["threshold"] == 128
    ink = [bool(br.ink_mask(p, 128).all()) for p in pages]
    assert ink == [False, True, True, False] and not any(br.ink_mask(p, 128).any() for p in pages[[0, 3]])
    for p in pages:
        assert bars_of(p) == {} and qrs_of(p) == ({}, 0)


def test_noise_pages_read_as_nothing():
    pages = ce.noise_pages()
    assert pages.shape == (3, 200, 333, 3)
    for page, density in zip(pages, ce.NOISE_DENSITIES):
        ink = br.ink_mask(page, 128)
        assert abs(float(ink.mean()) - density) < 0.01
        assert bars_of(page) == {} and qrs_of(page)[0] == {}
    runs = [max(len(br.row_runs(r)) for r in br.ink_mask(p, 128)) for p in pages]
    assert runs[1] > 40 and runs[2] > 64                                  # rows of more runs than a wave has lanes


@pytest.mark.parametrize("w", ce.EDGE_WIDTHS)
def test_edge_width_pages(w):
    pages, bars, qrs = ce.edge_width_pages(w)
    assert pages.shape == (2, 100, w, 3)
    for page, b, q in zip(pages, bars, qrs):
        assert bars_of(page) == b and qrs_of(page) == (q, 3)
    assert [b[0] for b in qrs[0]] == [0] and [b[2] for b in qrs[1]] == [w - 1]
    assert [b[2] for b in bars[0]] == [w - 1] and [b[0] for b in bars[1]] == [0]


# ---- damage ------------------------------------------------------------------------------------------------------------------------
def _row_texts(row: np.ndarray):
    return [bc.symbols_text(kind, list(vals)) for _, _, kind, _, vals in br.row_reads(row, BP["quiet"], BP["max_dist"])]


@pytest.mark.parametrize("strip", ce.DAMAGE_STRIPS, ids=lambda s: s[0])
def test_a_strip_with_one_column_inverted_reads_as_printed_or_not_at_all(strip):
    """Every pixel column of the strip in turn, and every whole module: the read is the printed text or nothing, never another text.
    Every row of such a page is the same row, so the page reads what its row reads (asserted on every fourth column, the GPU test's
    pages); the sweep itself runs on the row.  Both classes hold at least a quarter of the columns, so neither statement is vacuous:
    "Lumina-128" 156 read / 134 not, "12345678" 84 / 74, "C39-X" 138 / 84, "AB12cd" 110 / 193.  No whole-module flip reads."""
    text, kind, m = strip
    ink, x0, length = ce.strip_ink(text, kind, m)
    assert _row_texts(ink[0]) == [text] and ink.shape == (ce.STRIP_ROWS, length + 30) and ink[:, x0].all() and ink[:, x0 + length - 1].all()
    flips = ce.column_flips(ink, x0, length)
    assert len(flips) == length and all((f != ink).sum() == ce.STRIP_ROWS for f in flips[::17])
    got = [_row_texts(f[0]) for f in flips]
    other = [(k, g) for k, g in enumerate(got) if g not in ([text], [])]
    assert other == []
    reads = sum(g == [text] for g in got)
    assert (reads, length - reads) == {"Lumina-128": (156, 134), "12345678": (84, 74), "C39-X": (138, 84), "AB12cd": (110, 193)}[text]
    assert 4 * reads >= length and 4 * (length - reads) >= length
    for k in range(0, length, 4):
        rc, rs = br.codes_of_ink(flips[k])
        assert br.decoded(rc, rs) == got[k], k
    modules = ce.column_flips(ink, x0, length, width=m)
    assert len(modules) == length // m and [_row_texts(f[0]) for f in modules] == [[]] * len(modules)


def test_module_widths_that_are_no_whole_pixels():
    """Rendered at 4 px (Code 128) and 8 px (QR) and reduced with Lanczos: at 3.0 and 2.0 px a module the barcode reads, at 2.5 px it
    does NOT read today (the reader's tolerance is what it is); the QR symbol reads at 6, 5 and 4 px."""
    bar, sym = ce.rescale_sources()
    assert list(bars_of(bar).values()) == [(ce.RESCALE_BAR_TEXT, 0)] and list(qrs_of(sym)[0].values()) == [ce.RESCALE_QR_TEXT]
    read = []
    for f in ce.RESCALE_FACTORS:
        small = ce.rescaled(bar, f)
        assert small.shape == (int(96 * f), int(720 * f), 3) and len(np.unique(small)) > 2          # grey edges
        read.append([t for t, _ in bars_of(small).values()])
        assert list(qrs_of(ce.rescaled(sym, f))[0].values()) == [ce.RESCALE_QR_TEXT], f
    assert read == [[ce.RESCALE_BAR_TEXT], [], [ce.RESCALE_BAR_TEXT]]


@pytest.mark.parametrize("symbol", ce.RS_SYMBOLS, ids=lambda s: "%d-%s" % (s[0], qr.LEVELS[s[1]]))
def test_a_block_beyond_the_correction_capacity_does_not_read(symbol):
    """t - 1, t, t + 1, t + 2 and t + 4 wrong codewords in one block, six seeded patterns each: up to t the symbol reads what was
    printed and reports the errors it corrected; from t + 1 it does not read.  None of the 150 symbols decodes to other data."""
    version, level, block, text = symbol
    pages, wrong, t = ce.rs_pages(version, level, block, text)
    nb, _, _, ec = qr.block_structure(version, level)
    assert t == ec // 2 and block < nb and len(pages) == 30 and sorted(set(wrong)) == [t - 1, t, t + 1, t + 2, t + 4]
    for i, (page, n) in enumerate(zip(pages, wrong)):
        _, rc, rd, rf = R.qrcodes(page)
        assert rf == 3, i
        if n <= t:
            assert R.texts(rc, rd) == [text] and tuple(rc[0][4:6]) == (version, level) and int(rc[0][8]) == n, (i, n)
        else:
            assert len(rc) == 0, (i, n, R.texts(rc, rd))
