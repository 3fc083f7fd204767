"""GPU: lumina_ocr_aztec and lumina_ocr_datamatrix in the regimes their own test files never enter, on the pages of
tests/matrix_edge_inputs.py: sides past 4096 pixels (mask words past 63 in az_at and dm_sample, extremes packed from coordinates up
to 65534, the largest symbol of either pass against column 65534, H + 1 run offsets of a tall page), Reed-Solomon blocks with more
wrong codewords than the code corrects (the exits behind the locator; a locator of 156 coefficients over three chunks of lanes; the
second block of a 52 x 52 failing after the first was written), lists exactly at and one past their capacity (64 finders, 64 codes,
1024 candidates), ragged page groups (3 + 3 + 1 and 2 + 2 + 1, with and without mask_in), flat pages, block noise, widths around the
mask word with a symbol on either edge, and module widths that are no whole pixels.  Every device result EQUALS the restatement
(aztec_reference, dm_reference): mask, rows, data codewords, counts and finder or candidate counts, through the check helpers of the
passes' own test files; the definitions are integer, there is no tolerance.  tests/test_matrix_edge_inputs.py checks the restatements
themselves on the same pages, on the CPU."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch
from lumina_ocr.utils import datamatrix as dm

import aztec_reference as AR
import dm_reference as DR
import matrix_edge_inputs as me
from test_gpu_aztec import check as check_az, found as found_az
from test_gpu_datamatrix import check as check_dm, found as found_dm

pytestmark = pytest.mark.gpu

AZP, DMP = arch.AZTEC_PARAMS, arch.DM_PARAMS


# ---- long sides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turned", [False, True], ids=["long_w", "long_h"])
@pytest.mark.parametrize("shape", me.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_sides_aztec(engine, shape, turned):
    """a symbol across x = 4096 and, on the longest page, across 32768 and 61440 and the 11-layer symbol whose last column is 65534:
    az_at at mask words up to 1023; the first symbol's core lies in a row of 8000 runs, 990 of them before it: the finders' binary
    search at its depth; turned by np.rot90: the long side is H, H + 1 run offsets"""
    page, want = me.aztec_long_page(*shape)
    if turned:
        page, want = me.turned(page, want)
    (rc, rd, rf), = check_az(engine, page[None])
    assert found_az(rc, rd) == want and rf == len(want)


@pytest.mark.parametrize("turned", [False, True], ids=["long_w", "long_h"])
@pytest.mark.parametrize("shape", me.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_sides_datamatrix(engine, shape, turned):
    """the same for Data Matrix; the 52 x 52 symbol's elbow is at x = 65535 (doubled 131070): run_extremes' keys and dm_sample's
    largest term, ox * 2 * R * C = 7.1e8"""
    page, want = me.dm_long_page(*shape)
    if turned:
        page, want = me.turned(page, want)
    (rc, rd, rn), = check_dm(engine, page[None])
    assert found_dm(rc, rd) == want and rn == len(want)


# ---- Reed-Solomon beyond the capacity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol", me.AZ_RS_SYMBOLS, ids=me.az_rs_id)
def test_aztec_blocks_beyond_the_correction_capacity(engine, symbol):
    """t - 1, t, t + 1, t + 2 and t + 4 wrong codewords, six seeded patterns each, one batch: up to t the text reads and the error
    column is the count; beyond t the decode leaves through the exits behind the locator (too long a locator, fewer roots than its
    degree, a zero derivative, syndromes that remain) and the device, as the restatement, reads nothing — or, where the restatement
    lands on another codeword (compact 1 layer, t + 1, seed 3), the same wrong codewords: check demands equality there too."""
    compact, layers, text = symbol
    pages, wrong, t = me.az_rs_pages(*symbol)
    res = check_az(engine, pages)
    assert len(res) == 30
    beyond = 0
    for (rc, rd, rf), n in zip(res, wrong):
        assert rf == 1
        if n <= t:
            assert AR.texts(rc, rd) == [text] and int(rc[0][8]) == n and (int(rc[0][4]), bool(rc[0][5])) == (layers, compact)
        else:
            beyond += len(rc)
    assert beyond <= 1


@pytest.mark.parametrize("symbol", me.DM_RS_SYMBOLS, ids=me.dm_rs_id)
def test_datamatrix_blocks_beyond_the_correction_capacity(engine, symbol):
    """the same for rs_correct_block of rs.h on one- and two-block sizes; 52 x 52 with block 0 varied and block 1 at t, and
    with block 0 at t and block 1 varied: there the decode returns after block 0's codewords have been written"""
    size, block, text = symbol
    pages, wrong, t = me.dm_rs_pages(*symbol)
    nb = dm.SIZES[size][6]
    res = check_dm(engine, pages)
    assert len(res) == 30
    for (rc, rd, rn), n in zip(res, wrong):
        assert rn >= 1
        if n <= t:
            assert DR.texts(rc, rd) == [text] and int(rc[0][7]) == n + (nb - 1) * t and tuple(rc[0][4:6]) == dm.SIZES[size][:2]
        else:
            assert len(rc) == 0, n


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [64, 63])
def test_aztec_at_and_one_past_the_capacity(engine, cap):
    """64 finders with room for 64 and 64 symbols into a list of 64 (a full rank sort); into a list of 63: the count is 64 and no row
    is written (check asserts both)"""
    page, want = me.aztec_grid_page()
    (rc, rd, rf), = check_az(engine, page[None], max_codes=cap)
    assert found_az(rc, rd) == want and len(rc) == 64 and rf == 64 == AZP["max_finders"]


def test_aztec_one_finder_too_many(engine):
    """65 finders: the finder count is 65 and the page is not read"""
    page, _ = me.aztec_grid_page(1)
    (rc, _, rf), = check_az(engine, page[None], max_codes=64)
    assert len(rc) == 0 and rf == 65


@pytest.mark.parametrize("cap", [64, 63])
def test_datamatrix_codes_at_and_one_past_the_capacity(engine, cap):
    page, want = me.dm_grid_page()
    (rc, rd, rn), = check_dm(engine, page[None], max_codes=cap)
    assert found_dm(rc, rd) == want and len(rc) == 64 and 64 <= rn <= DMP["max_candidates"]


@pytest.mark.parametrize("squares", [1023, 1024])
def test_datamatrix_candidates_at_and_one_past_the_capacity(engine, squares):
    """1024 candidates with room for 1024, the symbol's the last of them: it is read; 1025: the count, and the page is not read"""
    page, want = me.dm_squares_page(squares)
    (rc, rd, rn), = check_dm(engine, page[None], max_candidates=1024)
    assert rn == squares + 1 and found_dm(rc, rd) == (want if squares == 1023 else {})


@pytest.mark.parametrize("extra", [0, 1])
def test_datamatrix_every_candidate_slot_is_decoded(engine, extra):
    """1024 candidates of which 600 are symbols: whichever slots the candidates fall into, every one of the 1024 is decoded, and the
    count says so (600 overflow the list: no row is written); with one candidate more the page is not read"""
    page = me.dm_many_symbols_page(extra)
    (rc, _, rn), = check_dm(engine, page[None], max_candidates=1024, max_codes=64)
    assert rn == 1024 + extra and len(rc) == (0 if extra else me.DM_MANY_SYMBOLS)


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def _az(engine, pages: np.ndarray, **kw):
    out = engine.aztec(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), debug=True, **kw)
    torch.cuda.synchronize()
    return out


def _dm(engine, pages: np.ndarray, **kw):
    out = engine.datamatrix(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), debug=True, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, "output %d" % k)


@pytest.mark.parametrize("group,first", [(3, 0), (2, 2)], ids=["7_pages_by_3", "5_pages_by_2"])
def test_ragged_page_groups(engine, group, first):
    """seven pages in groups of 3 + 3 + 1 and five in groups of 2 + 2 + 1: every pointer the two entries offset per group (pages, rows,
    data, counts, finder or candidate counts, mask_in, mask_out) with a group size that does not divide the batch.  Every page has its
    own texts (a wrong offset shows), page 3 is blank and page 5 has the most symbols.  The split call equals the restatement, the same
    call with the first call's mask as mask_in, the call in one group, and every page decoded alone."""
    pages, azs, dms = me.ragged_pages()
    pages, azs, dms = pages[first:], azs[first:], dms[first:]
    assert len(pages) % group == 1 and len(pages) > 2 * group
    engine.set_option("post_group", group)
    try:
        res_a, res_d = check_az(engine, pages), check_dm(engine, pages)
        split_a, split_d = _az(engine, pages), _dm(engine, pages)
        _same(_az(engine, pages, mask_in=split_a[3]), split_a, "aztec with mask_in")
        _same(_dm(engine, pages, mask_in=split_d[3]), split_d, "datamatrix with mask_in")
        _same(_dm(engine, pages, mask_in=split_a[3]), split_d, "datamatrix with the Aztec pass's mask")
    finally:
        engine.set_option("post_group", 64)
    assert [found_az(*r[:2]) for r in res_a] == azs and [found_dm(*r[:2]) for r in res_d] == dms
    assert [r[2] for r in res_a] == [len(a) for a in azs]
    whole_a, whole_d = _az(engine, pages), _dm(engine, pages)
    _same(split_a, whole_a, "aztec in one group")
    _same(split_d, whole_d, "datamatrix in one group")
    _same(_az(engine, pages, mask_in=whole_a[3]), whole_a, "aztec in one group with mask_in")
    _same(_dm(engine, pages, mask_in=whole_d[3]), whole_d, "datamatrix in one group with mask_in")
    for i in range(len(pages)):
        _same(_az(engine, pages[i:i + 1]), [t[i:i + 1] for t in whole_a], "aztec of page %d alone" % i)
        _same(_dm(engine, pages[i:i + 1]), [t[i:i + 1] for t in whole_d], "datamatrix of page %d alone" % i)


# ---- hard pages --------------------------------------------------------------------------------------------------------------------
def test_flat_pages(engine):
    """blank, all ink, grey 127 and grey 128: the two sides of the threshold (an all-ink page is one candidate)"""
    pages = me.flat_pages()
    assert all(len(rc) == 0 and rf == 0 for rc, _, rf in check_az(engine, pages))
    res = check_dm(engine, pages)
    assert all(len(rc) == 0 for rc, _, _ in res) and [rn for _, _, rn in res] == [0, 1, 1, 0]


def test_block_noise_pages(engine):
    """cells of 3, 5 and 8 px at densities 0.2 and 0.5: components of every shape for the extremes and the candidate filter, up to 15
    candidates a page whose every try is scored and dropped; a row of bullseyes under noise: finders whose decode is rejected"""
    pages = me.block_noise_pages()
    assert all(len(rc) == 0 and rf == 0 for rc, _, rf in check_az(engine, pages))
    res = check_dm(engine, pages)
    assert all(len(rc) == 0 for rc, _, _ in res) and max(rn for _, _, rn in res) >= 10
    page = me.noisy_bullseye_page()
    (rc, _, rf), = check_az(engine, page[None])
    assert len(rc) == 0 and rf == me.NOISY_BULLSEYES >= 3
    (rc, _, _), = check_dm(engine, page[None])
    assert len(rc) == 0


@pytest.mark.parametrize("w", me.EDGE_WIDTHS)
def test_widths_with_a_symbol_on_either_edge(engine, w):
    pages, azs, dms = me.edge_width_pages(w)
    res = check_az(engine, pages)
    assert [found_az(*r[:2]) for r in res] == azs and [r[2] for r in res] == [1, 1]
    assert [found_dm(*r[:2]) for r in check_dm(engine, pages)] == dms


def test_module_widths_that_are_no_whole_pixels(engine):
    """rendered at 8 px a module and reduced with Lanczos to 6, 5 and 4 px: the device equals the restatement, and both read the text"""
    azs, dms = me.rescale_sources()
    for f in me.RESCALE_FACTORS:
        res = check_az(engine, np.stack([me.rescaled(p, f) for p in azs]))
        assert [AR.texts(*r[:2]) for r in res] == [[text] for text, _, _ in me.RESCALE_AZ], f
        res = check_dm(engine, np.stack([me.rescaled(p, f) for p in dms]))
        assert [DR.texts(*r[:2]) for r in res] == [[text] for text, _ in me.RESCALE_DM], f
