"""GPU: lumina_ocr_barcodes through the C ABI against the restatement (tests/barcode_reference.py): the ink mask (parity hook), the
rows, the symbol values and the counts are EQUAL — the definition is integer arithmetic with a canonical order, so there is no
tolerance — and the decoded strings are what was rendered."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError

import barcode_reference as br
import table_reference as tr

pytestmark = pytest.mark.gpu

P = arch.BARCODE_PARAMS


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, syms) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in ("quiet", "max_dist", "min_rows", "row_gap")}
    cap = params.get("max_codes", P["max_codes"])
    codes, syms, cnt, mask = engine.barcodes(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    codes, syms, cnt, mask = codes.cpu().numpy(), syms.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rs = br.barcodes(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rc), rc)
        n = len(rc) if len(rc) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(syms[i, :n], rs[:n]), "page %d: symbols differ" % i
        assert not codes[i, n:].any() and not syms[i, n:].any(), "page %d: rows past the count were written" % i
        out.append((rc, rs))
    return out


def found(rc, rs):
    """-> {(x0, y0, x1, y1): (text, flags)}"""
    return {tuple(int(v) for v in c[:4]): (t, int(c[7])) for c, t in zip(rc, br.decoded(rc, rs))}


def put(page, x, y, text, kind="Code128", m=2, height=20, **kw):
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    return synth.render_barcode(page, x, y, syms, kind, m, height, **kw)


def test_three_pages_empty_single_and_four_codes(engine):
    """192 x 520: W is no multiple of 64 and every code crosses word boundaries"""
    pages = np.stack([blank(192, 520) for _ in range(3)])
    want1 = {put(pages[1], 37, 20, "Lumina-128"): ("Lumina-128", 0)}
    want2 = {put(pages[2], 13, 8, "AB12cd", m=2, height=24): ("AB12cd", 0),
             put(pages[2], 300, 10, "C39", "Code39", m=2, height=18): ("C39", 0),
             put(pages[2], 60, 60, "123456", m=3, height=30, reversed=True): ("123456", 1),
             put(pages[2], 400, 50, "77", m=2, height=40, vertical=True): ("77", 2)}
    res = check(engine, pages)
    assert found(*res[0]) == {} and found(*res[1]) == want1 and found(*res[2]) == want2


def test_vertical_code_longer_than_the_page_is_wide(engine):
    page = blank(520, 192)
    box = put(page, 50, 7, "Taller than wide", m=2, height=33, vertical=True)
    box2 = put(page, 120, 100, "UPSIDE", "Code39", m=2, height=21, vertical=True, reversed=True)
    assert box[3] - box[1] + 1 > 192
    (rc, rs), = check(engine, page[None])
    assert found(rc, rs) == {box: ("Taller than wide", 2), box2: ("UPSIDE", 3)}


def test_sixty_five_rows_the_last_work_group_has_one_row(engine):
    page = blank(65, 200)
    box = put(page, 10, 65 - 9, "Z", height=9)          # rows 56..64: the last row reads too
    (rc, rs), = check(engine, page[None])
    assert found(rc, rs) == {box: ("Z", 0)} and int(rc[0][6]) == 9


@pytest.mark.parametrize("kind", ["Code128", "Code39"])
def test_sixty_four_symbols_are_read_and_sixty_five_are_not(engine, kind):
    if kind == "Code128":
        t64, t65 = "12" * 61, "12" * 62                 # set C: start, 61 / 62 pairs, check, stop
        assert len(synth.code128_symbols(t64)) == 64 and len(synth.code128_symbols(t65)) == 65
    else:
        t64, t65 = "LUMINA-39." * 6 + "AB", "LUMINA-39." * 6 + "ABC"
        assert len(synth.code39_symbols(t64)) == 64
    page = blank(44, 2200)
    box = put(page, 5, 2, t64, kind, height=12)
    put(page, 5, 24, t65, kind, height=12)
    (rc, rs), = check(engine, page[None])
    assert found(rc, rs) == {box: (t64, 0)} and int(rc[0][5]) == 64


def test_overflowing_list_is_counted_and_not_written(engine):
    page = blank(100, 300)
    for y in (4, 36, 68):
        put(page, 20, y, "OVER", height=16)
    check(engine, page[None], max_codes=2)
    (rc, _), = check(engine, page[None], max_codes=3)
    assert len(rc) == 3


def test_five_codes_side_by_side_the_four_leftmost_are_the_rows(engine):
    page = blank(30, 640)
    boxes = [put(page, 14 + 122 * k, 5, "ab"[k % 2], height=14, reversed=k == 1) for k in range(5)]
    (rc, rs), = check(engine, page[None])
    assert found(rc, rs) == {b: ("ab"[k % 2], int(k == 1)) for k, b in enumerate(boxes[:4])}


def test_decoys_and_text_yield_nothing(engine):
    page, gt = synth.synth_barcode_decoys()
    assert len(gt) == 7
    (rc, _), = check(engine, page[None])
    assert len(rc) == 0
    (rc, _), = check(engine, synth.synth_page(300, 520, 5, n_lines=8)[0][None])
    assert len(rc) == 0


def test_synthetic_pages_decode_to_what_was_rendered(engine):
    pages, gts = zip(*[synth.synth_barcode_page(s, h=360, w=900, text_lines=3) for s in (1, 2)])
    for (rc, rs), gt in zip(check(engine, np.stack(pages)), gts):
        assert len(gt) >= 2
        assert found(rc, rs) == {g["box"]: (g["text"], int(g["reversed"]) | 2 * int(g["vertical"])) for g in gt}


def test_mask_in_gives_the_same_rows_and_mask_out_is_the_ink_mask(engine):
    pages = np.stack([synth.synth_barcode_page(s, h=192, w=520, text_lines=0, n_codes=2)[0] for s in (3, 4)])
    dev = torch.from_numpy(pages).cuda()
    codes, syms, cnt, mask = engine.barcodes(dev, debug=True)
    again = engine.barcodes(dev, mask_in=mask, debug=True)
    torch.cuda.synchronize()
    assert int(cnt.sum()) >= 2
    assert all(torch.equal(a, b) for a, b in zip((codes, syms, cnt, mask), again))
    for i, page in enumerate(pages):
        assert np.array_equal(mask[i].cpu().numpy().view(np.uint64), tr.pack_mask(tr.ink_mask(page, P["threshold"])))


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(blank(64, 200)[None]).cuda()
    good = dict(threshold=P["threshold"], quiet=P["quiet"], max_dist=P["max_dist"], min_rows=P["min_rows"], row_gap=P["row_gap"], max_codes=4)
    for bad in (dict(max_codes=0), dict(max_codes=257), dict(row_gap=0), dict(row_gap=17), dict(quiet=-1), dict(max_dist=257), dict(min_rows=0)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 8), -7, dtype=torch.int32, device="cuda")
        syms = torch.full((1, max(kw["max_codes"], 1), 64), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_barcodes(engine._h, pages.data_ptr(), 1, 64, 200, kw["threshold"], kw["quiet"], kw["max_dist"], kw["min_rows"], kw["row_gap"],
                                            kw["max_codes"], codes.data_ptr(), syms.data_ptr(), counts.data_ptr(), None, None,
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc != 0 and b"barcodes" in engine.lib.lumina_ocr_last_error(engine._h), bad
        assert bool((codes == -7).all()) and bool((syms == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError):
            engine.barcodes(pages, **kw)
    codes = torch.zeros((1, 4, 8), dtype=torch.int32, device="cuda")
    for args in ((None, codes.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_barcodes(engine._h, args[0], 1, 64, 200, 128, 5, 24, 8, 2, 4, args[1], None, None, None, None,
                                            torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and b"barcodes" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_barcodes(engine._h, pages.data_ptr(), 1, 0, 200, 128, 5, 24, 8, 2, 4, codes.data_ptr(), codes.data_ptr(), codes.data_ptr(),
                                        None, None, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
