"""GPU: lumina_ocr_datamatrix through the C ABI against the restatement (tests/dm_reference.py): the ink mask (parity hook), the rows,
the data codewords, the counts and the candidate counts are EQUAL — the definition is integer arithmetic with a canonical order, so
there is no tolerance — and the decoded strings are what was rendered.  Pages are 200 x 243: the smallest that hold a 52 x 52 symbol
at 3 px a module with its quiet zone; W is no multiple of 64."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import datamatrix as dm

import dm_reference as R
import table_reference as tr
from dm_pages import H, W, blank, corrupted, payload, put

pytestmark = pytest.mark.gpu

P = arch.DM_PARAMS
KEYS = ("min_module", "max_module", "quiet", "timing_max", "solid_max", "max_candidates")
ORDER = ("threshold", "min_module", "max_module", "quiet", "timing_max", "solid_max", "max_candidates", "max_codes")


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, candidates) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    codes, data, cnt, mask, nc = engine.datamatrix(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    codes, data, cnt, mask, nc = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64), nc.cpu().numpy()
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rd, rn = R.datamatrix(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nc[i]) == rn, "page %d: %d candidates, restatement %d" % (i, nc[i], rn)
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rc), rc)
        n = len(rc) if len(rc) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(data[i, :n], rd[:n]), "page %d: data codewords differ" % i
        assert not codes[i, n:].any() and not data[i, n:].any(), "page %d: rows past the count were written" % i
        out.append((rc, rd, rn))
    return out


def found(rc, rd):
    """-> {(x0, y0, x1, y1): text}"""
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}


def test_empty_page_and_every_size_reads(engine):
    """all 21 sizes, five or six a batch behind an empty page, each with its own rotation and module of 3 or 4 px"""
    for first in (0, 5, 10, 15):
        sizes = list(range(first, min(first + 5, dm.NUM_SIZES))) + ([20] if first == 15 else [])
        pages = np.stack([blank() for _ in range(len(sizes) + 1)])
        want = [{}]
        for i, s in enumerate(sizes):
            text = "1234" if s == 0 else payload(s)
            m = 3 if max(dm.SIZES[s][:2]) > 44 else 4
            want.append({put(pages[i + 1], 11 + i, 9 + 2 * i, text, s, m, (s + i) % 4): text})
        res = check(engine, pages)
        assert [found(*r[:2]) for r in res] == want, first
        assert [tuple(int(v) for v in r[0][0][4:7]) for r in res[1:]] == [dm.SIZES[s][:3] for s in sizes]


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_every_rotation_at_module_three_and_seven_square_and_rectangle(engine, rotation):
    pages = np.stack([blank(), blank()])
    a = put(pages[0], 41, 23, "ROT %d m3" % rotation, 3, 3, rotation)
    r = put(pages[0], 130, 60, "RECT %d" % rotation, 16, 3, rotation)
    b = put(pages[1], 50, 20, "ROT %d m7" % rotation, 4, 7, rotation, scheme="c40")
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: "ROT %d m3" % rotation, r: "RECT %d" % rotation} and found(*res[1][:2]) == {b: "ROT %d m7" % rotation}
    assert [int(c[8]) for c in res[0][0]] == [rotation, rotation] and int(res[1][0][0][8]) == rotation


def test_most_errors_each_block_corrects_and_one_more(engine):
    """52 x 52 with both blocks at 21 errors, 48 x 48 with 34 (the largest ec), 10 x 10 with 2; one more each -> the restatement's drop"""
    cases = ((14, 21, payload(14)), (13, 34, payload(13)), (0, 2, "1234"))
    pages = np.stack([blank() for _ in range(6)])
    boxes = []
    for i, (s, t, text) in enumerate(cases):
        boxes.append(put(pages[2 * i], 30, 20, "", s, sym=corrupted(text, s, t)))
        put(pages[2 * i + 1], 30, 20, "", s, sym=corrupted(text, s, t + 1))
    res = check(engine, pages)
    for i, (s, t, text) in enumerate(cases):
        assert found(*res[2 * i][:2]) == {boxes[i]: text} and int(res[2 * i][0][0][7]) == t * dm.SIZES[s][6], s
        assert len(res[2 * i + 1][0]) == 0 and res[2 * i + 1][2] == 1, s
    assert dm.SIZES[13][3] // 2 == 34 and dm.block_lengths(14) == [(102, 42), (102, 42)]


def test_word_boundary_page_edges_and_schemes(engine):
    pages = np.stack([blank(), blank()])
    a = put(pages[0], 40, 30, "ACROSS X = 64", 4, 3)                     # 18 x 18 at 3 px: x 40 .. 93
    assert a[0] < 64 < a[2]
    b = put(pages[0], 120, 100, "EDIFACT 42", 5, 4, 1, scheme="edifact")
    c = put(pages[1], 0, 0, "TOP LEFT", 3, 4, 1, scheme="x12")           # symbols whose edges are the page's
    d = put(pages[1], W - 22 * 4, H - 22 * 4, "bottom right é", 6, 4, 2, scheme="base256")
    e = put(pages[1], W - 36 * 3, 0, "top right", 18, 3, 0, scheme="text")
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: "ACROSS X = 64", b: "EDIFACT 42"}
    assert found(*res[1][:2]) == {c: "TOP LEFT", d: "bottom right é", e: "top right"}


def test_tilted_pages_equal_the_restatement(engine):
    """one and two degrees of residual skew: stairs on every edge, the grid is affine"""
    from PIL import Image
    pages = np.stack([blank(), blank()])
    put(pages[0], 60, 40, "TILT ONE", 6, 4)
    put(pages[1], 30, 20, payload(14, "TILT TWO "), 14, 3)
    pages = np.stack([np.asarray(Image.fromarray(p).rotate(a, resample=Image.BICUBIC, fillcolor=(255, 255, 255))) for p, a in zip(pages, (1.0, 2.0))])
    res = check(engine, pages)
    assert R.texts(*res[0][:2]) == ["TILT ONE"] and R.texts(*res[1][:2]) == [payload(14, "TILT TWO ")]


def test_decoys_and_text_yield_nothing(engine):
    page, gt = synth.synth_dm_decoys(h=H)
    text = synth.synth_page(page.shape[0], page.shape[1], 5, n_lines=7)[0]
    res = check(engine, np.stack([page, text]))
    assert len(gt) == 8 and len(res[0][0]) == 0 and res[0][2] >= 6 and len(res[1][0]) == 0


def test_overflowing_lists_are_counted_and_not_written(engine):
    page = blank()
    put(page, 20, 20, "ONE", 1, 4)
    put(page, 120, 100, "TWO", 2, 4)
    (rc, _, rn), = check(engine, page[None], max_codes=1)              # two symbols, room for one: the count is 2, no rows
    assert len(rc) == 2 and rn == 2
    (rc, _, rn), = check(engine, page[None], max_candidates=1)         # two candidates, room for one: the page is not read
    assert len(rc) == 0 and rn == 2
    (rc, rd, _), = check(engine, page[None], max_candidates=2, max_codes=2)
    assert sorted(R.texts(rc, rd)) == ["ONE", "TWO"]


def test_a_symbol_behind_more_than_sixty_four_candidates_is_read(engine):
    """108 solid squares of 24 px above the symbol: every one is a candidate, the symbol's component is the last root of the page"""
    page = blank(330, 400)
    for i in range(108):
        y, x = 5 + 29 * (i // 12), 8 + 32 * (i % 12)
        page[y:y + 24, x:x + 24] = 0
    box = put(page, 150, 270, "BEHIND 108 SQUARES", 4, 3)
    (rc, rd, rn), = check(engine, page[None])
    assert rn >= 109 > 64 and found(rc, rd) == {box: "BEHIND 108 SQUARES"}
    (rc, rd, rn), = check(engine, page[None], max_candidates=64)
    assert rn >= 109 and len(rc) == 0


def test_mask_in_gives_the_same_rows_and_mask_out_is_the_ink_mask(engine):
    pages = np.stack([synth.synth_dm_page(s, h=H, w=W, n_codes=2, text_lines=0, module_px=3)[0] for s in (3, 4)])
    dev = torch.from_numpy(pages).cuda()
    first = engine.datamatrix(dev, debug=True)
    again = engine.datamatrix(dev, mask_in=first[3], debug=True)
    torch.cuda.synchronize()
    assert int(first[2].sum()) >= 2
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i, page in enumerate(pages):
        assert np.array_equal(first[3][i].cpu().numpy().view(np.uint64), tr.pack_mask(tr.ink_mask(page, P["threshold"])))


def test_long_side_page_and_ragged_groups(engine):
    """one 2000 x 260 page with a symbol at either end; then n = 1 and n = 5 with the engine's page group at 2"""
    long_page = blank(260, 2000)
    a = put(long_page, 8, 30, "LEFT END", 3, 5)
    b = put(long_page, 2000 - 8 - 36 * 4, 100, "RIGHT END, LONG SIDE", 18, 4, 2)
    (rc, rd, _), = check(engine, long_page[None])
    assert found(rc, rd) == {a: "LEFT END", b: "RIGHT END, LONG SIDE"}
    pages = np.stack([blank() for _ in range(5)])
    want = [{put(pages[i], 10 + 9 * i, 12 + 5 * i, "PAGE %d" % i, 2 + i, 4, i % 4): "PAGE %d" % i} for i in range(5)]
    engine.set_option("post_group", 2)                                  # five pages leave in groups of 2 + 2 + 1
    try:
        res1 = check(engine, pages[:1])
        res5 = check(engine, pages)
    finally:
        engine.set_option("post_group", 64)
    assert [found(*r[:2]) for r in res1] == want[:1] and [found(*r[:2]) for r in res5] == want


def test_synthetic_pages_decode_to_what_was_rendered(engine):
    pages, gts = zip(*[synth.synth_dm_page(s, h=330, w=520, n_codes=2, text_lines=3) for s in (1, 2)])
    for (rc, rd, _), gt in zip(check(engine, np.stack(pages)), gts):
        assert len(gt) == 2 and found(rc, rd) == {g["box"]: g["text"] for g in gt}
        assert {tuple(int(v) for v in c[:4]): (int(c[4]), int(c[5]), int(c[8])) for c in rc} == {g["box"]: (g["rows"], g["cols"], g["rotation"]) for g in gt}


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(blank(64, 200)[None]).cuda()
    good = dict(P, max_codes=4)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_codes=0), dict(max_codes=65), dict(max_candidates=0), dict(max_candidates=1025), dict(quiet=-1), dict(quiet=5), dict(min_module=0),
                dict(max_module=2), dict(max_module=65), dict(timing_max=-1), dict(timing_max=129), dict(solid_max=-1), dict(solid_max=129)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), dm.MAX_DATA), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_datamatrix(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in ORDER], codes.data_ptr(), data.data_ptr(),
                                              counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        err = engine.lib.lumina_ocr_last_error(engine._h)
        assert rc != 0 and b"datamatrix" in err and b"max_candidates 1..1024" in err, bad
        assert bool((codes == -7).all()) and bool((data == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError, match="datamatrix"):
            engine.datamatrix(pages, **kw)
    codes = torch.zeros((1, 4, dm.MAX_DATA), dtype=torch.int32, device="cuda")
    for args in ((None, codes.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_datamatrix(engine._h, args[0], 1, 64, 200, *[good[k] for k in ORDER], args[1], codes.data_ptr(), codes.data_ptr(), None, None, None, st)
        assert rc != 0 and b"datamatrix: bad arguments" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_datamatrix(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in ORDER], codes.data_ptr(), codes.data_ptr(), codes.data_ptr(),
                                          None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    with pytest.raises(TypeError):
        engine.datamatrix(pages, ring_tol=3)


def test_pipeline_datamatrix_equals_the_stand_alone_call_whichever_pass_hands_the_mask_over(engine):
    from lumina_ocr.pipeline import OcrPipeline
    import qr_reference as QR
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    form = synth.synth_dm_page(5, h=460, w=620, n_codes=2, text_lines=3, module_px=4)[0]
    synth.draw_qr(form, 480, 330, synth.qr_encode("QR BESIDE", 2, 1, 3), 4)
    synth.render_barcode(form, 40, 430, synth.code128_symbols("WITH-DM"), "Code128", 2, 25)
    pages = torch.from_numpy(np.stack([form, blank(460, 620)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, empty), processed = OcrPipeline(engine, datamatrix=True, **kw).run(pages)
    (off, _), _ = OcrPipeline(engine, **kw).run(pages)
    _, rc, rd, _ = R.datamatrix(processed[0].cpu().numpy())
    assert len(rc) == 2 and np.array_equal(on.datamatrix, rc) and np.array_equal(on.dm_data, rd) and on.datamatrix.dtype == np.int32
    assert empty.datamatrix.shape == (0, 12) and empty.dm_data.shape == (0, dm.MAX_DATA)
    assert off.datamatrix is None and off.dm_data is None and off.texts == on.texts and np.array_equal(off.quads, on.quads)
    assert P["threshold"] == arch.QR_PARAMS["threshold"] == arch.BARCODE_PARAMS["threshold"]
    _, qc, qd, _ = QR.qrcodes(processed[0].cpu().numpy())
    for opts in (dict(marks=True), dict(tables=True), dict(barcodes=True), dict(qrcodes=True), dict(barcodes=True, qrcodes=True),
                 dict(marks=True, tables=True, qrcodes=True), dict(qrcodes=True, qr_params=dict(arch.QR_PARAMS, threshold=127))):
        (a, _), _ = OcrPipeline(engine, datamatrix=True, **opts, **kw).run(pages)
        (b, _), _ = OcrPipeline(engine, **opts, **kw).run(pages)
        assert np.array_equal(a.datamatrix, rc) and np.array_equal(a.dm_data, rd), opts
        for name in ("marks", "hrules", "vrules", "barcodes", "barcode_syms", "qrcodes", "qr_data"):
            va, vb = getattr(a, name), getattr(b, name)
            assert (va is None and vb is None) or np.array_equal(va, vb), (opts, name)
        assert a.texts == on.texts
        if opts.get("qrcodes") and "qr_params" not in opts:
            assert len(qc) == 1 and np.array_equal(a.qrcodes, qc) and np.array_equal(a.qr_data, qd)
    (few, _), _ = OcrPipeline(engine, datamatrix=True, dm_params=dict(P, max_codes=1), **kw).run(pages)
    assert few.datamatrix.shape == (0, 12)                                          # an overflowing page reports none
