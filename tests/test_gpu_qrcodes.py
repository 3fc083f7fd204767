"""GPU: lumina_ocr_qrcodes through the C ABI against the restatement (tests/qr_reference.py): the ink mask (parity hook), the rows, the
data codewords, the counts and the finder counts are EQUAL — the definition is integer arithmetic with a canonical order, so there is
no tolerance — and the decoded strings are what was rendered.  Pages are about 260 x 330: the smallest that hold a version 10 symbol
at 3 px a module with its quiet zone; W is no multiple of 64.  (The longest-block case uses the 560 x 587 pages of the all-versions tests.)"""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import qrcodes as qr

import qr_reference as R
import table_reference as tr

pytestmark = pytest.mark.gpu

P = arch.QR_PARAMS
H, W = 262, 331
KEYS = ("min_module", "max_module", "quiet", "centre_tol", "ring_tol", "timing_max", "max_finders")


def blank(h: int = H, w: int = W) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, finders) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    codes, data, cnt, mask, nf = engine.qrcodes(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    codes, data, cnt, mask, nf = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64), nf.cpu().numpy()
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rd, rf = R.qrcodes(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nf[i]) == rf, "page %d: %d finders, restatement %d" % (i, nf[i], rf)
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rc), rc)
        n = len(rc) if len(rc) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(data[i, :n], rd[:n]), "page %d: data codewords differ" % i
        assert not codes[i, n:].any() and not data[i, n:].any(), "page %d: rows past the count were written" % i
        out.append((rc, rd, rf))
    return out


def found(rc, rd):
    """-> {(x0, y0, x1, y1): text}"""
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}


def put(page, x, y, text, version, level=1, mask=0, module=3, rotation=0, sym=None):
    return synth.draw_qr(page, x, y, synth.qr_encode(text, version, level, mask) if sym is None else sym, module, rotation)


def corrupted(text, version, level, mask, block, wrong):
    cw = synth.qr_interleave(synth.qr_data_codewords(text, version, level), version, level)
    nb = qr.block_structure(version, level)[0]
    for i in range(wrong):
        cw[i * nb + block] ^= (0xFF, 0x5A, 0x01, 0x80)[i % 4]
    return synth.qr_matrix(cw, version, level, mask)


def test_empty_page_two_symbols_and_version_ten(engine):
    """v1 at 3 px and at 7 px turned by 90 degrees on one page; v10 at 3 px turned by 180 degrees on the next"""
    pages = np.stack([blank() for _ in range(3)])
    want1 = {put(pages[1], 20, 30, "V1 M3", 1, 1, 0, 3): "V1 M3", put(pages[1], 150, 60, "v1 seven", 1, 2, 5, 7, 1): "v1 seven"}
    long_text = "https://lumina.example/documents/2024/invoice?id=4242&sig=" + "0123456789abcdef" * 4
    want2 = {put(pages[2], 77, 40, long_text, 10, 1, 3, 3, 2): long_text}
    res = check(engine, pages)
    assert found(*res[0][:2]) == {} and found(*res[1][:2]) == want1 and found(*res[2][:2]) == want2
    assert [int(c[4]) for c in res[1][0]] == [1, 1] and sorted(int(c[9]) for c in res[1][0]) == [0, 1] and tuple(res[2][0][0][4:10]) == (10, 1, 3, 216, 0, 2)


def test_corrected_errors_second_format_copy_word_boundary_and_page_edges(engine):
    pages = np.stack([blank() for _ in range(3)])
    # page 0: 10-H at 3 px turned by 270 degrees, its last block with all the errors it can correct
    t10 = qr.block_structure(10, 3)[3] // 2
    text10 = "ten-H " + "error correction " * 5
    box10 = put(pages[0], 60, 50, text10, 10, module=3, rotation=3, sym=corrupted(text10, 10, 3, 6, 7, t10))
    # page 1: 5-Q at 4 px with t errors in block 1; a version 2 symbol across x = 64 whose first format copy is destroyed
    t5 = qr.block_structure(5, 2)[3] // 2
    text5 = "five-Q corrected " * 3
    box5 = put(pages[1], 170, 20, text5, 5, module=4, sym=corrupted(text5, 5, 2, 1, 1, t5))
    true = qr.format_word(0, 7)
    flips = next(f for f in range(1, 1 << 15) if 4 <= bin(f).count("1") <= 6 and min(bin((true ^ f) ^ w).count("1") for w in qr.FORMAT_WORDS) >= 4)
    sym = synth.qr_encode("SECOND COPY", 2, 0, 7)
    for i, (r, c) in enumerate(qr.format_positions(2)[0]):
        if (flips >> i) & 1:
            sym[r, c] = not sym[r, c]
    box2 = put(pages[1], 30, 150, "", 2, module=3, sym=sym)
    assert box2[0] < 64 < box2[2]
    # page 2: symbols whose edges are the page's: left and top, right and bottom
    boxa = put(pages[2], 0, 0, "TOP LEFT", 2, 2, 4, 4, 1)
    boxb = put(pages[2], W - 21 * 7, H - 21 * 7, "bottom right", 1, 0, 2, 7, 2)
    res = check(engine, pages)
    assert found(*res[0][:2]) == {box10: text10} and int(res[0][0][0][8]) == t10 == 14
    assert found(*res[1][:2]) == {box5: text5, box2: "SECOND COPY"}
    by_box = {tuple(int(v) for v in c[:4]): c for c in res[1][0]}
    assert int(by_box[box5][8]) == t5 == 9 and int(by_box[box2][10]) == qr.SECOND_COPY and int(by_box[box5][10]) == 0
    assert found(*res[2][:2]) == {boxa: "TOP LEFT", boxb: "bottom right"}


def longest_block_pages():
    """9-L at 3 px on two 560 x 587 pages: ec = 30 and two blocks of 146 codewords, the longest block and the largest locator (L = 15)
    versions 1-10 ever build.  Page 0 has ec // 2 = 15 errors in the last block, page 1 one more -> pages, the symbol's box, its text"""
    nb, _, _, ec = qr.block_structure(9, 0)
    assert (nb, ec) == (2, 30)
    text = ("9-L " + "the longest block / " * 16)[:qr.data_codewords(9, 0) - 3]
    pages = np.stack([blank(587, 560), blank(587, 560)])
    box = put(pages[0], 90, 120, "", 9, module=3, sym=corrupted(text, 9, 0, 5, nb - 1, ec // 2))
    put(pages[1], 90, 120, "", 9, module=3, sym=corrupted(text, 9, 0, 5, nb - 1, ec // 2 + 1))
    return pages, box, text


def test_the_longest_block_reads_at_its_capacity_and_not_one_error_past_it(engine):
    pages, box, text = longest_block_pages()
    res = check(engine, pages)
    assert found(*res[0][:2]) == {box: text} and int(res[0][0][0][8]) == 15
    assert len(res[1][0]) == 0 and res[1][2] == 3                                  # three finders and no symbol


def test_every_version_and_level_reads(engine):
    """all 40 block structures, 9-L with its two blocks of 146 codewords (the longest) among them: four levels a batch"""
    for version in range(1, 11):
        pages = np.stack([blank() for _ in range(4)])
        want = []
        for level in range(4):
            text = ("v%d%s " % (version, qr.LEVELS[level]) + "block structure / " * 16)[:qr.data_codewords(version, level) - 3]
            want.append({put(pages[level], 30 + 7 * level, 25, text, version, level, (version + level) % 8, 3, level): text})
        res = check(engine, pages)
        assert [found(*r[:2]) for r in res] == want, version
        assert [tuple(int(v) for v in r[0][0][4:6]) for r in res] == [(version, level) for level in range(4)]


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_every_rotation_at_module_three_and_seven(engine, rotation):
    pages = np.stack([blank(), blank()])
    a = put(pages[0], 41, 23, "ROT %d m3" % rotation, 4, 3, 2, 3, rotation)
    b = put(pages[1], 50, 20, "ROT %d m7" % rotation, 3, 0, 6, 7, rotation)
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: "ROT %d m3" % rotation} and found(*res[1][:2]) == {b: "ROT %d m7" % rotation}
    assert int(res[0][0][0][9]) == rotation == int(res[1][0][0][9])


def test_a_corner_crowded_by_a_neighbours_finder_reads_on_a_later_pair(engine):
    page, want = synth.synth_qr_crowded_page()
    (rc, rd, rf), = check(engine, page[None])
    assert found(rc, rd) == want and rf == 6


def test_tilted_pages_equal_the_restatement(engine):
    """half a degree and two degrees of residual skew: stairs on every edge, the grid is affine"""
    from PIL import Image
    pages = np.stack([blank(), blank()])
    put(pages[0], 60, 40, "TILT 5", 5, 1, 2, 4)
    put(pages[1], 70, 40, "TILT 10", 10, 1, 2, 3)
    pages = np.stack([np.asarray(Image.fromarray(p).rotate(a, resample=Image.BICUBIC, fillcolor=(255, 255, 255))) for p, a in zip(pages, (0.5, 2.0))])
    res = check(engine, pages)
    assert R.texts(*res[0][:2]) == ["TILT 5"] and R.texts(*res[1][:2]) == ["TILT 10"]


def test_decoys_and_text_yield_nothing(engine):
    page, gt = synth.synth_qr_decoys()
    text = synth.synth_page(page.shape[0], page.shape[1], 5, n_lines=9)[0]
    res = check(engine, np.stack([page, text]))
    assert len(gt) == 7 and len(res[0][0]) == 0 and res[0][2] >= 9 and len(res[1][0]) == 0


def test_overflowing_lists_are_counted_and_not_written(engine):
    page = blank()
    put(page, 20, 20, "ONE", 1, module=4)
    put(page, 170, 120, "TWO", 2, module=4)
    (rc, _, rf), = check(engine, page[None], max_codes=1)              # two symbols, room for one: the count is 2, no rows
    assert len(rc) == 2 and rf == 6
    (rc, _, rf), = check(engine, page[None], max_finders=5)            # six finders, room for five: the page is not read
    assert len(rc) == 0 and rf == 6
    (rc, rd, _), = check(engine, page[None], max_finders=6, max_codes=2)
    assert sorted(R.texts(rc, rd)) == ["ONE", "TWO"]


def test_mask_in_gives_the_same_rows_and_mask_out_is_the_ink_mask(engine):
    pages = np.stack([synth.synth_qr_page(s, h=H, w=W, n_codes=2, text_lines=0, module_px=3)[0] for s in (3, 4)])
    dev = torch.from_numpy(pages).cuda()
    first = engine.qrcodes(dev, debug=True)
    again = engine.qrcodes(dev, mask_in=first[3], debug=True)
    torch.cuda.synchronize()
    assert int(first[2].sum()) >= 2
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i, page in enumerate(pages):
        assert np.array_equal(first[3][i].cpu().numpy().view(np.uint64), tr.pack_mask(tr.ink_mask(page, P["threshold"])))


def test_synthetic_pages_decode_to_what_was_rendered(engine):
    pages, gts = zip(*[synth.synth_qr_page(s, h=330, w=520, n_codes=2, text_lines=3) for s in (1, 2)])
    for (rc, rd, _), gt in zip(check(engine, np.stack(pages)), gts):
        assert len(gt) == 2 and found(rc, rd) == {g["box"]: g["text"] for g in gt}
        assert {tuple(int(v) for v in c[:4]): (int(c[4]), int(c[5]), int(c[6]), int(c[9])) for c in rc} == \
               {g["box"]: (g["version"], g["level"], g["mask"], g["rotation"]) for g in gt}


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(blank(64, 200)[None]).cuda()
    order = ("threshold", "min_module", "max_module", "quiet", "centre_tol", "ring_tol", "timing_max", "max_finders", "max_codes")
    good = dict(P, max_codes=4)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_codes=0), dict(max_codes=65), dict(max_finders=0), dict(max_finders=65), dict(quiet=-1), dict(quiet=5), dict(min_module=0),
                dict(max_module=2), dict(max_module=65), dict(centre_tol=-1), dict(ring_tol=65), dict(timing_max=-1), dict(timing_max=129)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), qr.MAX_DATA), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_qrcodes(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in order], codes.data_ptr(), data.data_ptr(),
                                           counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        assert rc != 0 and b"qrcodes" in engine.lib.lumina_ocr_last_error(engine._h), bad
        assert bool((codes == -7).all()) and bool((data == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError):
            engine.qrcodes(pages, **kw)
    # the barcode call's codes for the same mistakes
    codes = torch.zeros((1, 4, 12), dtype=torch.int32, device="cuda")
    bp = arch.BARCODE_PARAMS
    rc_bar = engine.lib.lumina_ocr_barcodes(engine._h, pages.data_ptr(), 1, 64, 200, bp["threshold"], bp["quiet"], bp["max_dist"], bp["min_rows"], bp["row_gap"], 0,
                                            codes.data_ptr(), codes.data_ptr(), codes.data_ptr(), None, None, st)
    rc_qr = engine.lib.lumina_ocr_qrcodes(engine._h, pages.data_ptr(), 1, 64, 200, *[dict(good, max_codes=0)[k] for k in order], codes.data_ptr(), codes.data_ptr(),
                                          codes.data_ptr(), None, None, None, st)
    assert rc_bar == rc_qr != 0
    for args in ((None, codes.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_qrcodes(engine._h, args[0], 1, 64, 200, *[good[k] for k in order], args[1], codes.data_ptr(), codes.data_ptr(), None, None, None, st)
        rc_bar = engine.lib.lumina_ocr_barcodes(engine._h, args[0], 1, 64, 200, 128, 5, 24, 8, 2, 4, args[1], codes.data_ptr(), codes.data_ptr(), None, None, st)
        assert rc == rc_bar != 0 and b"barcodes" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_qrcodes(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in order], codes.data_ptr(), codes.data_ptr(), codes.data_ptr(),
                                       None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    with pytest.raises(TypeError):
        engine.qrcodes(pages, max_dist=3)


def test_pipeline_qrcodes_equal_the_stand_alone_call_whichever_pass_hands_the_mask_over(engine):
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    form = synth.synth_qr_page(5, h=460, w=620, n_codes=2, text_lines=3, module_px=4)[0]
    synth.render_barcode(form, 40, 430, synth.code128_symbols("WITH-QR"), "Code128", 2, 25)
    pages = torch.from_numpy(np.stack([form, blank(460, 620)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, empty), processed = OcrPipeline(engine, qrcodes=True, **kw).run(pages)
    (off, _), _ = OcrPipeline(engine, **kw).run(pages)
    codes, data, cnt = (t.cpu().numpy() for t in engine.qrcodes(processed))
    assert int(cnt[0]) == 2 and int(cnt[1]) == 0
    assert np.array_equal(on.qrcodes, codes[0, :2]) and np.array_equal(on.qr_data, data[0, :2]) and on.qrcodes.dtype == np.int32
    _, rc, rd, _ = R.qrcodes(processed[0].cpu().numpy())
    assert np.array_equal(on.qrcodes, rc) and np.array_equal(on.qr_data, rd)
    assert empty.qrcodes.shape == (0, 12) and empty.qr_data.shape == (0, qr.MAX_DATA)
    assert off.qrcodes is None and off.qr_data is None and off.texts == on.texts and np.array_equal(off.quads, on.quads)
    assert P["threshold"] == arch.BARCODE_PARAMS["threshold"] == arch.MARK_PARAMS["threshold"] == arch.TABLE_PARAMS["threshold"]
    for opts in (dict(marks=True), dict(tables=True), dict(barcodes=True), dict(marks=True, tables=True), dict(marks=True, barcodes=True),
                 dict(barcodes=True, barcode_params=dict(arch.BARCODE_PARAMS, threshold=127))):
        (a, _), _ = OcrPipeline(engine, qrcodes=True, **opts, **kw).run(pages)
        (b, _), _ = OcrPipeline(engine, **opts, **kw).run(pages)
        assert np.array_equal(a.qrcodes, rc) and np.array_equal(a.qr_data, rd), opts
        for name in ("marks", "hrules", "vrules", "barcodes", "barcode_syms"):
            va, vb = getattr(a, name), getattr(b, name)
            assert (va is None and vb is None) or np.array_equal(va, vb), (opts, name)
        assert a.texts == on.texts
    (few, _), _ = OcrPipeline(engine, qrcodes=True, qr_params=dict(P, max_codes=1), **kw).run(pages)
    assert few.qrcodes.shape == (0, 12)                                             # an overflowing page reports none
