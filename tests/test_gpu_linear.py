"""GPU: lumina_ocr_barcodes_kinds through the C ABI against the restatement (tests/linear_reference.py): the ink mask, the rows, the symbol
values and the counts are EQUAL for every kind set (integer arithmetic in a canonical order: no tolerance), the decoded strings are
what was rendered, and lumina_ocr_barcodes and kinds = 3 are what tests/barcode_reference.py says on pages that hold EAN and ITF."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch
from lumina_ocr.engine import EngineError

import linear_pages as lp
import linear_reference as lr

pytestmark = pytest.mark.gpu

P = arch.BARCODE_PARAMS
ALL = lr.ALL_KINDS


def run(engine, pages: np.ndarray, kinds, **kw):
    out = engine.barcodes(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), debug=True, kinds=kinds, **kw)
    torch.cuda.synchronize()
    codes, syms, cnt, mask = (t.cpu().numpy() for t in out)
    return codes, syms, cnt, mask.view(np.uint64)


def equal(got, refs, cap=P["max_codes"]):
    """device (codes, syms, counts, mask) of a batch against the per-page (mask, codes, syms) of a restatement"""
    codes, syms, cnt, mask = got
    for i, (rmask, rc, rs) in enumerate(refs):
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s\n%s" % (i, cnt[i], len(rc), codes[i, :int(cnt[i])], rc)
        n = len(rc) if len(rc) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(syms[i, :n], rs[:n]), "page %d: symbols differ" % i
        assert not codes[i, n:].any() and not syms[i, n:].any(), "page %d: rows past the count were written" % i


@pytest.mark.parametrize("kinds", [ALL, 4, 8, 16, 32], ids=["all", "ean13", "ean8", "upce", "itf"])
def test_device_equals_restatement_on_the_regime_pages(engine, kinds):
    """three 420 x 640 pages in one call: module widths 2-4, ITF ratios 2 / 2.5 / 3, upside down, vertical, neighbours, page edges,
    filled quiet zones, failing checks, a start from the second 64-run chunk of its row, text"""
    pages, wants = lp.regime_pages()
    refs = [lp.reference(("regime", i), pages[i], kinds) for i in range(len(pages))]
    got = run(engine, pages, kinds)
    equal(got, refs)
    for i in range(len(pages)):
        n = int(got[2][i])
        assert lp.found(got[0][i, :n], got[1][i, :n]) == lp.only(wants[i], kinds)
    assert int(got[2].sum()) >= (3 if kinds != ALL else 31)


def test_kind_names_and_mixed_sets(engine):
    pages, wants = lp.regime_pages()
    for kinds, names in ((1 | 4 | 32, ("code128", "ean13", "itf")), (2 | 8 | 16, "code39,ean8,upce")):
        refs = [lp.reference(("regime", i), pages[i], kinds) for i in range(1, 3)]
        equal(run(engine, pages[1:], kinds), refs)
        equal(run(engine, pages[1:], names), refs)


def test_the_old_entry_and_kinds_3_are_unchanged_on_pages_with_ean_and_itf(engine):
    pages, _ = lp.regime_pages()
    refs = [lp.old_reference(("regime", i), pages[i]) for i in range(len(pages))]
    assert sum(len(r[1]) for r in refs) == 3                   # the two Code 128 and the Code 39, none of the other strips
    equal(run(engine, pages, None), refs)
    equal(run(engine, pages, 3), refs)
    for i, page in enumerate(lp.reference_pages()):            # the pages of tests/test_barcode_reference.py with EAN and ITF strips added
        ref = [lp.old_reference(("reference", i), page)]
        equal(run(engine, page[None], None), ref)
        equal(run(engine, page[None], 3), ref)


def test_itf_of_sixty_four_digits_uses_every_lane_pair(engine):
    digits = "".join(str((7 * k + k // 10) % 10) for k in range(64))
    page = lp.blank(40, 1000)
    want = {}
    lp.put(page, want, 40, 4, "ITF", digits, m=2, height=12)
    lp.put(page, want, 40, 22, "ITF", digits + "12", m=2, height=12, read=False)      # 66 digits: not read
    ref = lp.reference("itf64", page, ALL)
    got = run(engine, page[None], ALL)
    equal(got, [ref])
    assert lp.found(ref[1], ref[2]) == want and int(ref[1][0][5]) == 64


def test_overflowing_list_is_counted_and_not_written(engine):
    page = lp.blank(100, 300)
    for y, (kind, digits) in zip((4, 36, 68), (("EAN13", lp.EAN13_A), ("EAN8", lp.EAN8), ("ITF", lp.ITF6))):
        lp.put(page, {}, 20, y, kind, digits, height=16)
    ref = lp.reference("overflow", page, ALL)
    assert len(ref[1]) == 3
    got = run(engine, page[None], ALL, max_codes=2)
    equal(got, [ref], cap=2)
    assert int(got[2][0]) == 3 and not got[0].any()
    equal(run(engine, page[None], ALL, max_codes=3), [ref], cap=3)


def test_mask_in_gives_the_same_rows_and_mask_out_is_the_ink_mask(engine):
    pages, _ = lp.regime_pages()
    dev = torch.from_numpy(pages[:2]).cuda()
    codes, syms, cnt, mask = engine.barcodes(dev, debug=True, kinds=ALL)
    again = engine.barcodes(dev, mask_in=mask, debug=True, kinds=ALL)
    torch.cuda.synchronize()
    assert int(cnt.sum()) >= 20
    assert all(torch.equal(a, b) for a, b in zip((codes, syms, cnt, mask), again))
    for i in range(2):
        assert np.array_equal(mask[i].cpu().numpy().view(np.uint64), lp.reference(("regime", i), pages[i], ALL)[0])


def test_bad_kinds_return_a_status_and_write_nothing(engine):
    pages = torch.from_numpy(lp.blank(64, 200)[None]).cuda()
    for bad in (0, 64, 3 | 64, -1, 1 << 20):
        codes = torch.full((1, 4, 8), -7, dtype=torch.int32, device="cuda")
        syms = torch.full((1, 4, 64), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_barcodes_kinds(engine._h, pages.data_ptr(), 1, 64, 200, P["threshold"], P["quiet"], P["max_dist"], P["min_rows"], P["row_gap"],
                                                  4, codes.data_ptr(), syms.data_ptr(), counts.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream, bad)
        torch.cuda.synchronize()
        assert rc != 0 and b"barcodes_kinds" in engine.lib.lumina_ocr_last_error(engine._h) and b"kinds" in engine.lib.lumina_ocr_last_error(engine._h), bad
        assert bool((codes == -7).all()) and bool((syms == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError):
            engine.barcodes(pages, kinds=bad)
    with pytest.raises(ValueError):
        engine.barcodes(pages, kinds=("ean13", "codabar"))
    codes = torch.full((1, 4, 8), -7, dtype=torch.int32, device="cuda")
    rc = engine.lib.lumina_ocr_barcodes_kinds(engine._h, pages.data_ptr(), 1, 64, 200, P["threshold"], P["quiet"], 257, P["min_rows"], P["row_gap"], 4,
                                              codes.data_ptr(), codes.data_ptr(), codes.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream, ALL)
    assert rc != 0 and bool((codes == -7).all())
