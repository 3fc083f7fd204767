"""CPU: the restatements (tests/aztec_reference.py, tests/dm_reference.py) on the pages of tests/matrix_edge_inputs.py — inputs neither
had seen: sides past 4096, Reed-Solomon blocks beyond their capacity, lists at their capacity, ragged page groups, flat and noise
pages, symbols on either edge of widths around the mask word, module widths that are no whole pixels.  The GPU file
(tests/test_gpu_matrix_code_edges.py) asserts that the device EQUALS the restatements on these pages; this file states what every page
was built to show and that the restatements find exactly that: which symbols read and with how many errors, how many finders or
candidates there are, which pages read nothing — so that a page that stopped entering its regime would be noticed here."""
import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.utils import aztec as az
from lumina_ocr.utils import datamatrix as dm

import aztec_pages as AP
import aztec_reference as AR
import dm_reference as DR
import matrix_edge_inputs as me

AZP, DMP = arch.AZTEC_PARAMS, arch.DM_PARAMS


def az_of(page: np.ndarray, **kw):
    """-> ({box: text}, finders, rows) of the Aztec restatement"""
    _, rc, rd, rf = AR.aztec(page, **kw)
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, AR.texts(rc, rd))}, rf, rc


def dm_of(page: np.ndarray, **kw):
    """-> ({box: text}, candidates, rows) of the Data Matrix restatement"""
    _, rc, rd, rn = DR.datamatrix(page, **kw)
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, DR.texts(rc, rd))}, rn, rc


# ---- long sides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", me.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_aztec_pages(shape):
    h, w = shape
    page, want = me.aztec_long_page(h, w)
    got, finders, rc = az_of(page)
    assert got == want and finders == len(want) == (4 if w == 65535 else 1)
    assert [b[0] < c <= b[2] for b, c in zip(sorted(want), me.BORDERS)] == [True] * (3 if w == 65535 else 1)
    assert len({int(c[9]) for c in rc}) == len(rc) and len(set(want.values())) == len(want)          # every symbol its own rotation and text
    if w == 65535:                                           # the largest symbol, its last column the page's
        assert max(want) == (65352, 2, 65534, 184) and tuple(int(v) for v in rc[0][4:6]) == (11, 0) and int(rc[0][9]) == 2
        # the centre row of the first symbol's core holds more than 2^12 runs, the core's run in their middle: a deep binary search
        row = AR.ink_mask(page, AZP["threshold"])[28]
        starts = np.flatnonzero(row & ~np.r_[False, row[:-1]])
        box = min(want)
        assert (box[1] + box[3]) // 2 == 28 and me.AZ_TICK_ROWS[0] <= 28 < me.AZ_TICK_ROWS[1] and len(starts) > 4096
        assert int((starts < box[0]).sum()) > 900 and int((starts > box[2]).sum()) > 4096
    page, want = me.turned(page, want)                       # the long side is H
    assert page.shape[:2] == (w, h)
    got, finders, _ = az_of(page)
    assert got == want and finders == len(want)


@pytest.mark.parametrize("shape", me.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_datamatrix_pages(shape):
    h, w = shape
    page, want = me.dm_long_page(h, w)
    got, cands, rc = dm_of(page)
    assert got == want and cands == len(want) == (4 if w == 65535 else 1)
    assert [b[0] < c <= b[2] for b, c in zip(sorted(want), me.BORDERS)] == [True] * (3 if w == 65535 else 1)
    assert len({int(c[8]) for c in rc}) == len(rc) and len(set(want.values())) == len(want)
    if w == 65535:
        assert max(want) == (65379, 2, 65534, 157) and tuple(int(v) for v in rc[0][4:6]) == (52, 52) and int(rc[0][8]) == 2
        # the elbow O of the 52 x 52 symbol as the decode takes it (P[(k + 3) % 4], doubled pixels): its x is the largest the pass can
        # meet, so dm_sample's largest term, ox * 2 * R * C, is the one exercised
        ink = DR.ink_mask(page, DMP["threshold"])
        corners = [c for _, c in DR.find_candidates(ink, DMP["min_module"], DMP["max_module"]) if c[3][0] // 2 >= 65379]
        assert len(corners) == 1
        ox, oy = corners[0][(2 + 3) % 4]
        assert ox // 2 > 65300 and (ox, oy) == (2 * 65535, 2 * 2) and ox * 2 * 52 * 52 > 7.0e8
    page, want = me.turned(page, want)
    assert page.shape[:2] == (w, h)
    got, cands, _ = dm_of(page)
    assert got == want and cands == len(want)


# ---- Reed-Solomon beyond the capacity ----------------------------------------------------------------------------------------------
def test_the_nearly_empty_symbols_have_the_capacities_they_were_chosen_for():
    t = {me.az_rs_id(s): AP.capacity(*s) for s in me.AZ_RS_SYMBOLS}
    assert t["full11_short"] >= 150 and t["full11_short"] > 2 * 64          # the locator spans three chunks of 64 lanes
    assert (t["full11_short"], t["full8_short"], t["compact4_short"]) == (156, 118, 37) and t["full11_filled"] == 47
    assert t["full11_short"] <= 318 // 2 and 318 // 2 - t["full11_short"] <= 3   # within three of the Chien / Forney loop's bound
    assert len(t) == len(me.AZ_RS_SYMBOLS) == 9
    assert [dm.SIZES[s][:2] for s, _, _ in me.DM_RS_SYMBOLS] == [(10, 10), (26, 26), (48, 48), (52, 52), (52, 52), (16, 48)]
    assert [dm.SIZES[s][3] // dm.SIZES[s][6] // 2 for s, _, _ in me.DM_RS_SYMBOLS] == [2, 14, 34, 21, 21, 14] and dm.SIZES[14][6] == 2


@pytest.mark.parametrize("symbol", me.AZ_RS_SYMBOLS, ids=me.az_rs_id)
def test_an_aztec_block_beyond_the_correction_capacity(symbol):
    """t - 1, t, t + 1, t + 2 and t + 4 wrong codewords, six seeded patterns each: up to t the symbol reads what was printed and
    reports the errors it corrected.  Beyond t a decoder may land on another valid codeword: of the 30 pages of a symbol at most one
    beyond t reads anything (today exactly one of all 270 does: compact 1 layer, t + 1, seed 3 reads another text)."""
    compact, layers, text = symbol
    pages, wrong, t = me.az_rs_pages(*symbol)
    assert len(pages) == 30 and sorted(set(wrong)) == [t - 1, t, t + 1, t + 2, t + 4] and t == AP.capacity(*symbol)
    beyond = []
    for i, (page, n) in enumerate(zip(pages, wrong)):
        _, rc, rd, rf = AR.aztec(page)
        assert rf == 1, i
        if n <= t:
            assert AR.texts(rc, rd) == [text] and int(rc[0][8]) == n and (int(rc[0][4]), bool(rc[0][5])) == (layers, compact), (i, n)
        elif len(rc):
            beyond.append((i, n, AR.texts(rc, rd)))
    assert len(beyond) <= 1, beyond
    assert (len(beyond) == 1) == (me.az_rs_id(symbol) == "compact1_filled"), beyond


@pytest.mark.parametrize("symbol", me.DM_RS_SYMBOLS, ids=me.dm_rs_id)
def test_a_datamatrix_block_beyond_the_correction_capacity(symbol):
    """the same for Data Matrix; in the two-block 52 x 52 the other block has exactly t wrong codewords, so the error column is the sum
    and, with block 1 varied, the decode fails after block 0 has been corrected.  None of the 180 pages reads beyond t."""
    size, block, text = symbol
    pages, wrong, t = me.dm_rs_pages(*symbol)
    nb = dm.SIZES[size][6]
    assert len(pages) == 30 and sorted(set(wrong)) == [t - 1, t, t + 1, t + 2, t + 4] and block < nb
    for i, (page, n) in enumerate(zip(pages, wrong)):
        _, rc, rd, rn = DR.datamatrix(page)
        assert rn >= 1, i                                                 # (damage may split a second candidate off the symbol)
        if n <= t:
            assert DR.texts(rc, rd) == [text] and int(rc[0][7]) == n + (nb - 1) * t and tuple(rc[0][4:6]) == dm.SIZES[size][:2], (i, n)
        else:
            assert len(rc) == 0, (i, n, DR.texts(rc, rd))


def test_dm_corrupted_changes_what_it_says():
    from lumina_ocr import synth
    clean = synth.dm_interleave(synth.dm_data_codewords(me.DM_RS_SYMBOLS[3][2], 14), 14)
    place = dm.placement_of(14)
    for counts in ((0, 0), (3, 0), (0, 22), (20, 25)):
        m = me.dm_corrupted(me.DM_RS_SYMBOLS[3][2], 14, counts, 1)
        got = [sum(int(m[place[8 * i + b]]) << (7 - b) for b in range(8)) for i in range(len(clean))]
        diff = [i for i, (a, b) in enumerate(zip(got, clean)) if a != b]
        assert (sum(i % 2 == 0 for i in diff), sum(i % 2 == 1 for i in diff)) == counts       # (204 data codewords: the parity is the block's in both parts)


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
def test_aztec_grid_pages():
    page, want = me.aztec_grid_page()
    assert page.shape[:2] == me.AZ_GRID_SHAPE and len(want) == len(set(want.values())) == 64 == AZP["max_finders"]
    got, finders, rc = az_of(page)
    assert got == want and finders == 64 and sorted({int(c[9]) for c in rc}) == [0, 1, 2, 3]
    over, _ = me.aztec_grid_page(1)
    got, finders, _ = az_of(over)                                         # 65 finders: the page is not read; with room for 65 it is
    assert got == {} and finders == 65


def test_datamatrix_grid_and_squares_pages():
    page, want = me.dm_grid_page()
    assert page.shape[:2] == me.DM_GRID_SHAPE and len(want) == len(set(want.values())) == 64
    got, cands, rc = dm_of(page)
    assert got == want and 64 <= cands <= DMP["max_candidates"] and sorted({int(c[8]) for c in rc}) == [0, 1, 2, 3]
    page, want = me.dm_squares_page(1023)
    assert page.shape[:2] == me.DM_SQUARES_SHAPE
    assert dm_of(page, max_candidates=1024)[:2] == (want, 1024) and dm_of(page, max_candidates=1023)[:2] == ({}, 1024)
    over, _ = me.dm_squares_page(1024)
    assert dm_of(over, max_candidates=1024)[:2] == ({}, 1025)


def test_datamatrix_page_of_many_symbols():
    """1024 candidates, 600 of them symbols that read: more than any half of the candidate slots holds"""
    page = me.dm_many_symbols_page()
    assert page.shape[:2] == me.DM_MANY_SHAPE
    got, cands, rc = dm_of(page, max_candidates=1024)
    assert cands == 1024 and len(rc) == me.DM_MANY_SYMBOLS == 600 and sorted(got.values()) == ["%03d" % k for k in range(600)]
    assert dm_of(me.dm_many_symbols_page(1), max_candidates=1024)[:2] == ({}, 1025)


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def test_ragged_pages_differ_and_hold_what_was_planted():
    pages, azs, dms = me.ragged_pages()
    assert pages.shape == (7, me.RAGGED_H, me.RAGGED_W, 3) and len({p.tobytes() for p in pages}) == 7
    for i, page in enumerate(pages):
        got, finders, _ = az_of(page)
        assert got == azs[i] and finders == len(azs[i]), i
        assert dm_of(page)[0] == dms[i], i
    assert [len(a) for a in azs] == [len(d) for d in dms] == [1, 1, 1, 0, 1, 3, 1]
    texts = [t for a in azs for t in a.values()] + [t for d in dms for t in d.values()]
    assert len(set(texts)) == len(texts) == 16


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
def test_flat_pages_hold_nothing():
    pages = me.flat_pages()
    assert [int(p[0, 0, 0]) for p in pages] == [255, 0, 127, 128] and AZP["threshold"] == DMP["threshold"] == 128
    for p in pages:
        assert az_of(p)[:2] == ({}, 0) and dm_of(p)[0] == {}
    assert [dm_of(p)[1] for p in pages] == [0, 1, 1, 0]                   # an all-ink page is one solid component: a candidate


def test_block_noise_pages_read_as_nothing():
    pages = me.block_noise_pages()
    assert pages.shape == (6, me.NOISE_H, me.NOISE_W, 3)
    cands = []
    for page, (cell, density) in zip(pages, me.NOISE_CELLS):
        assert abs(float(DR.ink_mask(page, 128).mean()) - density) < 0.03
        assert az_of(page)[:2] == ({}, 0)
        got, n, _ = dm_of(page)
        assert got == {}
        cands.append(n)
    assert max(cands) >= 10 and cands[me.NOISE_CELLS.index((8, 0.2))] >= 10 and all(c >= 1 for c in cands)
    page = me.noisy_bullseye_page()                                       # finders whose decode is rejected
    got, finders, _ = az_of(page)
    assert got == {} and finders >= 3 and finders == me.NOISY_BULLSEYES and dm_of(page)[0] == {}


@pytest.mark.parametrize("w", me.EDGE_WIDTHS)
def test_edge_width_pages(w):
    pages, azs, dms = me.edge_width_pages(w)
    assert pages.shape == (2, 100, w, 3)
    for page, a, d in zip(pages, azs, dms):
        assert az_of(page)[:2] == (a, 1) and dm_of(page)[0] == d
    assert [b[0] for b in azs[0]] == [0] and [b[2] for b in azs[1]] == [w - 1]
    assert [b[2] for b in dms[0]] == [w - 1] and [b[0] for b in dms[1]] == [0]


def test_module_widths_that_are_no_whole_pixels():
    """Rendered at 8 px a module and reduced with Lanczos to 6, 5 and 4 px: every symbol reads at every factor."""
    azs, dms = me.rescale_sources()
    for f in me.RESCALE_FACTORS:
        for page, (text, compact, layers) in zip(azs, me.RESCALE_AZ):
            small = me.rescaled(page, f)
            assert small.shape == (int(320 * f), int(320 * f), 3) and len(np.unique(small)) > 2          # grey edges
            got, _, rc = az_of(small)
            assert list(got.values()) == [text] and (int(rc[0][4]), bool(rc[0][5])) == (layers, compact), f
            assert rc[0][2] - rc[0][0] + 1 == pytest.approx(az.modules(compact, layers) * 8 * f, abs=2)
        for page, (text, size) in zip(dms, me.RESCALE_DM):
            got, _, rc = dm_of(me.rescaled(page, f))
            assert list(got.values()) == [text] and tuple(rc[0][4:6]) == dm.SIZES[size][:2], f
