"""GPU: lumina_ocr_barcodes and lumina_ocr_qrcodes in the regimes their own test files never enter, on the pages of
tests/code_edge_inputs.py: sides past 4096 pixels (more than 64 mask words a row and, turned, a line of the transposed mask; run
coordinates up to 65534 in the 16-bit run slots; QR modules sampled at mask words past 64), page groups with a remainder (3 + 3 + 1
and 2 + 2 + 1, with and without mask_in), lists exactly at and one past their capacity (256 barcodes, 64 finders), blank, all-ink,
grey and noise pages, widths around the mask word with a symbol on either edge, and damaged symbols: barcodes with a pixel column
inverted, module widths that are no whole pixels, QR blocks with more wrong codewords than the code corrects (the exits of the decode
behind the Berlekamp-Massey step).  Every device result EQUALS the restatement (barcode_reference, qr_reference): mask, rows, values,
counts and finder counts, through the check helpers of the passes' own test files; the definitions are integer, there is no tolerance.
tests/test_code_edge_inputs.py checks the restatements themselves on the same pages, on the CPU."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch
from lumina_ocr.utils import qrcodes as qr

import barcode_reference as br
import code_edge_inputs as ce
import qr_reference as R
from test_gpu_barcodes import check as check_bars, found as found_bars
from test_gpu_qrcodes import check as check_qrs, found as found_qrs

pytestmark = pytest.mark.gpu

BP, QP = arch.BARCODE_PARAMS, arch.QR_PARAMS


# ---- long sides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turned", [False, True], ids=["long_w", "long_h"])
@pytest.mark.parametrize("shape", ce.BARCODE_LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_sides_barcodes(engine, shape, turned):
    """strips across the 4095 / 4096 border of a row's 64-word chunks (and, on the longest page, across 32768 and 61440 and up to
    x = 65370), read forwards and backwards; turned: the codes are vertical, the run list is the transposed mask's and a page has
    H + W rows of slots"""
    page, want = ce.barcode_long_page(*shape)
    pages = page[None]
    if turned:
        pages, want = ce.transposed(pages), {ce.turned_box(b): (t, f | 2) for b, (t, f) in want.items()}
    (rc, rs), = check_bars(engine, pages)
    assert found_bars(rc, rs) == want


@pytest.mark.parametrize("turned", [False, True], ids=["long_w", "long_h"])
@pytest.mark.parametrize("which", ["96x65535", "96x8191", "200x8191"])
def test_long_sides_qrcodes(engine, which, turned):
    """version 1 symbols across every chunk border and one whose quiet zone leaves the page at column 65534, each with its own level,
    mask and rotation; a version 10 symbol whose 57 rows of modules all cross x = 4096; turned by np.rot90 (a transposed symbol is its
    mirror image and does not read): the long side is H"""
    w = int(which.split("x")[1])
    page, want = ce.qr_tall_v10_page() if which == "200x8191" else ce.qr_long_page(96, w)
    if turned:
        page, want = np.ascontiguousarray(np.rot90(page)), {ce.rot90_box(b, w): t for b, t in want.items()}
    (rc, rd, rf), = check_qrs(engine, page[None])
    assert found_qrs(rc, rd) == want and rf == 3 * len(want)


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def _bars(engine, pages: np.ndarray, **kw):
    out = engine.barcodes(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), debug=True, **kw)
    torch.cuda.synchronize()
    return out


def _qrs(engine, pages: np.ndarray, **kw):
    out = engine.qrcodes(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), debug=True, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, "output %d" % k)


@pytest.mark.parametrize("group,first", [(3, 0), (2, 2)], ids=["7_pages_by_3", "5_pages_by_2"])
def test_ragged_page_groups(engine, group, first):
    """seven pages in groups of 3 + 3 + 1 and five in groups of 2 + 2 + 1: every pointer the two entries offset per group (pages, rows,
    values or data, counts, finder counts, mask_in, mask_out) with a group size that does not divide the batch.  Every page has its own
    texts (a wrong offset shows), page 3 is blank and page 5 has the most codes.  The split call equals the restatement, the same call
    with the first call's mask as mask_in, the call in one group, and every page decoded alone."""
    pages, bars, qrs = ce.ragged_pages()
    pages, bars, qrs = pages[first:], bars[first:], qrs[first:]
    assert len(pages) % group == 1 and len(pages) > 2 * group
    engine.set_option("post_group", group)
    try:
        res_b, res_q = check_bars(engine, pages), check_qrs(engine, pages)
        split_b, split_q = _bars(engine, pages), _qrs(engine, pages)
        _same(_bars(engine, pages, mask_in=split_b[3]), split_b, "barcodes with mask_in")
        _same(_qrs(engine, pages, mask_in=split_q[3]), split_q, "qrcodes with mask_in")
    finally:
        engine.set_option("post_group", 64)
    assert [found_bars(*r) for r in res_b] == bars and [found_qrs(*r[:2]) for r in res_q] == qrs
    assert [r[2] for r in res_q] == [3 * len(q) for q in qrs]
    whole_b, whole_q = _bars(engine, pages), _qrs(engine, pages)
    _same(split_b, whole_b, "barcodes in one group")
    _same(split_q, whole_q, "qrcodes in one group")
    _same(_bars(engine, pages, mask_in=whole_b[3]), whole_b, "barcodes in one group with mask_in")
    _same(_qrs(engine, pages, mask_in=whole_q[3]), whole_q, "qrcodes in one group with mask_in")
    for i in range(len(pages)):
        _same(_bars(engine, pages[i:i + 1]), [t[i:i + 1] for t in whole_b], "barcodes of page %d alone" % i)
        _same(_qrs(engine, pages[i:i + 1]), [t[i:i + 1] for t in whole_q], "qrcodes of page %d alone" % i)


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(64, 64), (65, 64), (256, 256), (257, 256)])
def test_barcodes_at_and_one_past_the_capacity(engine, n, cap):
    """exactly max_codes codes, four in every row that reads: a full list, sorted (at 256 one full round of the merge kernel's rank sort
    and a full key array); one more: the count, and no row is written (check asserts both)"""
    page, want = ce.barcode_grid_page(n)
    assert cap == (BP["max_codes"] if cap == 64 else 256)
    (rc, rs), = check_bars(engine, page[None], max_codes=cap)
    assert len(rc) == n and found_bars(rc, rs) == want


def test_qrcodes_at_and_one_past_the_capacity(engine):
    """64 finders with room for 64: 21 symbols into a list of 21; into a list of 20: the count is 21 and no row is written; 65
    finders: the finder count is 65 and the page is not read"""
    full, want = ce.qr_grid_page(1)
    over, _ = ce.qr_grid_page(2)
    (rc, rd, rf), (rc2, _, rf2) = check_qrs(engine, np.stack([full, over]), max_codes=21)
    assert found_qrs(rc, rd) == want and len(rc) == 21 and rf == 64 == QP["max_finders"]
    assert len(rc2) == 0 and rf2 == 65
    (rc, _, rf), = check_qrs(engine, full[None], max_codes=20)
    assert len(rc) == 21 and rf == 64


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
def test_flat_pages(engine):
    """blank, all ink, grey 127 and grey 128: the two sides of the threshold"""
    pages = ce.flat_pages()
    assert all(len(rc) == 0 for rc, _ in check_bars(engine, pages))
    assert all(len(rc) == 0 and rf == 0 for rc, _, rf in check_qrs(engine, pages))


@pytest.mark.parametrize("k", [0, 1, 2], ids=["density_%s" % d for d in ce.NOISE_DENSITIES])
def test_noise_pages(engine, k):
    """many components for the union-find and the accumulation at the roots; rows of more than 64 runs full of near-start patterns"""
    page = ce.noise_pages()[k]
    (rc, _), = check_bars(engine, page[None])
    (qc, _, _), = check_qrs(engine, page[None])
    assert len(rc) == 0 and len(qc) == 0


@pytest.mark.parametrize("w", ce.EDGE_WIDTHS)
def test_widths_with_a_symbol_on_either_edge(engine, w):
    pages, bars, qrs = ce.edge_width_pages(w)
    assert [found_bars(*r) for r in check_bars(engine, pages)] == bars
    res = check_qrs(engine, pages)
    assert [found_qrs(*r[:2]) for r in res] == qrs and [r[2] for r in res] == [3, 3]


# ---- damage ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip", ce.DAMAGE_STRIPS, ids=lambda s: s[0])
def test_strips_with_one_column_inverted(engine, strip):
    """every fourth pixel column of the strip inverted over its full height, one batch: the bars are a pixel too wide, too narrow or
    split, and the match distance lies either side of max_dist S M / 256; the device reads what the restatement reads, which is the
    printed text or nothing (tests/test_code_edge_inputs.py has the whole sweep)"""
    text, kind, m = strip
    ink, x0, length = ce.strip_ink(text, kind, m)
    pages = ce.page_of(ce.column_flips(ink, x0, length, step=4))
    assert len(pages) == -(-length // 4)
    got = [br.decoded(rc, rs) for rc, rs in check_bars(engine, pages)]
    assert all(g in ([text], []) for g in got) and [text] in got and [] in got


def test_module_widths_that_are_no_whole_pixels(engine):
    """rendered at 4 px (Code 128) and 8 px (QR) and reduced with Lanczos to 3.0, 2.5, 2.0 and 6, 5, 4 px a module: the device equals
    the restatement whatever that says.  Today the barcode reads at 3.0 and 2.0 px and does NOT read at 2.5 px; the QR symbol reads at
    all three."""
    bar, sym = ce.rescale_sources()
    for f in ce.RESCALE_FACTORS:
        (rc, rs), = check_bars(engine, ce.rescaled(bar, f)[None])
        assert br.decoded(rc, rs) == ([] if f == 0.625 else [ce.RESCALE_BAR_TEXT]), f
        (qc, qd, _), = check_qrs(engine, ce.rescaled(sym, f)[None])
        assert R.texts(qc, qd) == [ce.RESCALE_QR_TEXT], f


@pytest.mark.parametrize("version", sorted({s[0] for s in ce.RS_SYMBOLS}))
def test_blocks_beyond_the_correction_capacity(engine, version):
    """t - 1, t, t + 1, t + 2 and t + 4 wrong codewords in one block (1-L, 1-H, 2-M, 5-Q block 1, 10-H block 7), six seeded patterns
    each, one batch a version: beyond t the decode leaves through its exits behind the Berlekamp-Massey step (too long a locator, fewer
    roots than its degree, a zero derivative, syndromes that remain) and the device, as the restatement, reads nothing"""
    symbols = [s for s in ce.RS_SYMBOLS if s[0] == version]
    built = [ce.rs_pages(*s) for s in symbols]
    res = check_qrs(engine, np.concatenate([b[0] for b in built]))
    assert len(res) == 30 * len(symbols)
    for k, ((_, level, _, text), (_, wrong, t)) in enumerate(zip(symbols, built)):
        for (rc, rd, rf), n in zip(res[30 * k:30 * k + 30], wrong):
            assert rf == 3
            if n <= t:
                assert R.texts(rc, rd) == [text] and int(rc[0][8]) == n and tuple(rc[0][4:6]) == (version, level)
            else:
                assert len(rc) == 0, (qr.LEVELS[level], n)
