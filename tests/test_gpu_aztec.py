"""GPU: lumina_ocr_aztec through the C ABI against the restatement (tests/aztec_reference.py): the ink mask (parity hook), the rows, the
data codewords, the counts and the finder counts are EQUAL — the definition is integer arithmetic with a canonical order, so there is
no tolerance — and the decoded strings are what was rendered.  Pages are as small as their symbols allow."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import aztec as az

import aztec_pages as AP
import aztec_reference as R
import table_reference as tr

pytestmark = pytest.mark.gpu

P = arch.AZTEC_PARAMS
KEYS = ("min_module", "max_module", "quiet", "centre_tol", "ring_tol", "mark_max", "max_finders")
ORDER = ("threshold",) + KEYS + ("max_codes",)


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, finders) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    codes, data, cnt, mask, nf = engine.aztec(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    codes, data, cnt, mask, nf = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64), nf.cpu().numpy()
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rd, rn = R.aztec(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nf[i]) == rn, "page %d: %d finders, restatement %d" % (i, nf[i], rn)
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
    """the 15 sizes, several to a page, behind an empty page; W = 430 is no multiple of 64"""
    H, W = 200, 430
    groups = (((True, 1), (True, 2), (True, 3), (True, 4), (False, 1)), ((False, 2), (False, 3), (False, 4), (False, 5)),
              ((False, 6), (False, 7)), ((False, 8), (False, 9)), ((False, 10), (False, 11)))
    pages = np.stack([AP.blank(H, W) for _ in range(len(groups) + 1)])
    want = [{}]
    for g, page in zip(groups, pages[1:]):
        x, w = 7, {}
        for i, (compact, layers) in enumerate(g):
            text = AP.payload(compact, layers)
            w[AP.put(page, x, 5 + 3 * i, text, compact, layers, 3, (layers + i) % 4)] = text
            x += AP.side_px(compact, layers) + 11
        want.append(w)
    res = check(engine, pages)
    assert [found(*r[:2]) for r in res] == want
    assert [[(bool(c[5]), int(c[4])) for c in r[0]] for r in res[1:]] == [list(g) for g in groups]


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_every_rotation_at_module_three_and_seven(engine, rotation):
    pages = np.stack([AP.blank(140, 330), AP.blank(140, 330)])
    a = AP.put(pages[0], 21, 13, "ROT %d m3" % rotation, True, 1, 3, rotation)
    b = AP.put(pages[0], 130, 20, "Full %d, m3." % rotation, False, 3, 3, rotation)
    c = AP.put(pages[1], 12, 6, "ROT %d m7" % rotation, True, 1, 7, rotation)
    d = AP.put(pages[1], 150, 3, "Full %d m7" % rotation, False, 1, 7, rotation)
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: "ROT %d m3" % rotation, b: "Full %d, m3." % rotation}
    assert found(*res[1][:2]) == {c: "ROT %d m7" % rotation, d: "Full %d m7" % rotation}
    assert [int(r[9]) for r in res[0][0]] == [rotation] * 2 and [int(r[9]) for r in res[1][0]] == [rotation] * 2


@pytest.mark.parametrize("compact,layers", AP.WIDTH_ENDS)
def test_most_errors_the_block_corrects_and_one_more(engine, compact, layers):
    """the smallest and the largest symbol of every codeword width with ec // 2 codewords destroyed, and with one more"""
    text = AP.payload(compact, layers)
    t = AP.capacity(compact, layers, text)
    s = AP.side_px(compact, layers) + 16
    pages = np.stack([AP.blank(s, s + 3), AP.blank(s, s + 3)])
    box = AP.put(pages[0], 9, 8, "", compact, layers, matrix=AP.corrupted(text, compact, layers, t))
    AP.put(pages[1], 9, 8, "", compact, layers, matrix=AP.corrupted(text, compact, layers, t + 1))
    res = check(engine, pages)
    assert found(*res[0][:2]) == {box: text} and int(res[0][0][0][8]) == t
    assert len(res[1][0]) == 0 and res[1][2] == 1


def test_mode_message_errors_are_corrected(engine):
    pages = np.stack([AP.blank(110, 230)])
    for x, compact, layers, wrong in ((8, True, 2, 2), (100, False, 4, 3)):
        words, nd = az.symbol_words("MODE %d" % wrong, compact, layers)
        mode = az.mode_words(compact, layers, nd)
        for i in range(wrong):
            mode[2 * i] ^= 9
        AP.put(pages[0], x, 9, "", compact, layers, matrix=az.matrix_of_words(compact, layers, words, nd, mode))
    (rc, rd, _), = check(engine, pages)
    assert R.texts(rc, rd) == ["MODE 2", "MODE 3"] and [int(c[10]) for c in rc] == [2, 3]


def test_word_boundary_and_page_edges(engine):
    """a symbol across x = 64, and symbols whose sides are the page's: the edge counts as quiet"""
    H, W = 150, 200
    pages = np.stack([AP.blank(H, W), AP.blank(H, W)])
    a = AP.put(pages[0], 40, 30, "ACROSS X = 64", True, 1)
    assert a[0] < 64 < a[2]
    c = AP.put(pages[1], 0, 0, "TOP LEFT", True, 2, 3, 1)
    d = AP.put(pages[1], W - 19 * 4, H - 19 * 4, "bottom right \xe9", False, 1, 4, 2)
    e = AP.put(pages[1], W - 45, 0, "top right", True, 1, 3)
    f = AP.put(pages[1], 0, H - 45, "bottom left", True, 1, 3, 3)
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: "ACROSS X = 64"}
    assert found(*res[1][:2]) == {c: "TOP LEFT", d: "bottom right \xe9", e: "top right", f: "bottom left"}


@pytest.mark.parametrize("compact,layers", sorted(AP.TILTS))
def test_tilted_pages_equal_the_restatement_and_read(engine, compact, layers):
    text = AP.payload(compact, layers, "TILT ")
    s = AP.side_px(compact, layers) + 44
    page = AP.blank(s, s + 5)
    AP.put(page, 22, 20, text, compact, layers, 3, layers % 4)
    tilts = AP.TILTS[(compact, layers)]
    res = check(engine, np.stack([AP.tilted(page, a) for a in tilts]))
    assert [R.texts(*r[:2]) for r in res] == [[text]] * len(tilts)


def test_decoys_and_text_yield_nothing(engine):
    page, kinds = AP.decoys()
    text = synth.synth_page(page.shape[0], page.shape[1], 5, n_lines=5)[0]
    res = check(engine, np.stack([page, text]))
    assert len(kinds) == 11 and len(res[0][0]) == 0 and res[0][2] >= 3 and len(res[1][0]) == 0


def test_overflowing_lists_are_counted_and_not_written(engine):
    page = AP.blank(70, 140)
    AP.put(page, 8, 8, "ONE", True, 1)
    AP.put(page, 80, 12, "TWO", True, 1)
    (rc, _, rn), = check(engine, page[None], max_codes=1)              # two symbols, room for one: the count is 2, no rows
    assert len(rc) == 2 and rn == 2
    (rc, _, rn), = check(engine, page[None], max_finders=1)            # two finders, room for one: the page is not read
    assert len(rc) == 0 and rn == 2
    (rc, rd, _), = check(engine, page[None], max_finders=2, max_codes=2)
    assert R.texts(rc, rd) == ["ONE", "TWO"]


def test_mask_in_gives_the_same_rows_and_mask_out_is_the_ink_mask(engine):
    pages = np.stack([AP.blank(100, 150), AP.blank(100, 150)])
    AP.put(pages[0], 20, 10, "mask in", True, 2, 3, 1)
    AP.put(pages[1], 30, 5, "Mask Out 2", False, 2, 3, 2)
    dev = torch.from_numpy(pages).cuda()
    first = engine.aztec(dev, debug=True)
    again = engine.aztec(dev, mask_in=first[3], debug=True)
    torch.cuda.synchronize()
    assert first[2].tolist() == [1, 1]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i, page in enumerate(pages):
        assert np.array_equal(first[3][i].cpu().numpy().view(np.uint64), tr.pack_mask(tr.ink_mask(page, P["threshold"])))


def test_ragged_page_groups(engine):
    """n = 1 and n = 4 with the engine's page group at 3"""
    pages = np.stack([AP.blank(90, 120) for _ in range(4)])
    want = [{AP.put(pages[i], 10 + 9 * i, 6 + 5 * i, "PAGE %d" % i, i % 2 == 0, 1 + i % 2, 3, i % 4): "PAGE %d" % i} for i in range(4)]
    engine.set_option("post_group", 3)
    try:
        res1 = check(engine, pages[:1])
        res4 = check(engine, pages)
    finally:
        engine.set_option("post_group", 64)
    assert [found(*r[:2]) for r in res1] == want[:1] and [found(*r[:2]) for r in res4] == want


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(AP.blank(64, 200)[None]).cuda()
    good = dict(P, max_codes=4)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_codes=0), dict(max_codes=65), dict(max_finders=0), dict(max_finders=65), dict(quiet=-1), dict(quiet=5), dict(min_module=0),
                dict(max_module=2), dict(max_module=65), dict(centre_tol=-1), dict(centre_tol=65), dict(ring_tol=-1), dict(ring_tol=16), dict(mark_max=-1),
                dict(mark_max=65)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), az.MAX_DATA), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_aztec(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in ORDER], codes.data_ptr(), data.data_ptr(),
                                         counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        err = engine.lib.lumina_ocr_last_error(engine._h)
        assert rc != 0 and b"aztec" in err and b"max_finders 1..64" in err, bad
        assert bool((codes == -7).all()) and bool((data == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError, match="aztec"):
            engine.aztec(pages, **kw)
    codes = torch.zeros((1, 4, az.MAX_DATA), dtype=torch.int32, device="cuda")
    for args in ((None, codes.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_aztec(engine._h, args[0], 1, 64, 200, *[good[k] for k in ORDER], args[1], codes.data_ptr(), codes.data_ptr(), None, None, None, st)
        assert rc != 0 and b"aztec: bad arguments" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_aztec(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in ORDER], codes.data_ptr(), codes.data_ptr(), codes.data_ptr(),
                                     None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    assert engine.lib.lumina_ocr_aztec_workspace_bytes(2, 64, 200, 64, 16) > engine.lib.lumina_ocr_aztec_workspace_bytes(1, 64, 200, 64, 16) > 0
    assert engine.lib.lumina_ocr_aztec_workspace_bytes(1, 0, 200, 64, 16) == 0 and engine.lib.lumina_ocr_aztec_workspace_bytes(1, 64, 200, 65, 16) == 0
    with pytest.raises(TypeError):
        engine.aztec(pages, timing_max=3)


def test_pipeline_aztec_equals_the_stand_alone_call_whichever_pass_hands_the_mask_over(engine):
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    form = synth.synth_dm_page(5, h=460, w=620, n_codes=1, text_lines=3, module_px=4)[0]
    synth.draw_qr(form, 480, 330, synth.qr_encode("QR BESIDE", 2, 1, 3), 4)
    AP.put(form, 300, 300, "Aztec on the form, 2024.", False, 2, 4, 1)
    AP.put(form, 400, 200, "COMPACT", True, 1, 4)
    pages = torch.from_numpy(np.stack([form, AP.blank(460, 620)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, empty), processed = OcrPipeline(engine, aztec=True, **kw).run(pages)
    (off, _), _ = OcrPipeline(engine, **kw).run(pages)
    _, rc, rd, _ = R.aztec(processed[0].cpu().numpy())
    assert len(rc) == 2 and np.array_equal(on.aztec, rc) and np.array_equal(on.az_data, rd) and on.aztec.dtype == np.int32
    assert sorted(R.texts(rc, rd)) == ["Aztec on the form, 2024.", "COMPACT"]
    assert empty.aztec.shape == (0, 12) and empty.az_data.shape == (0, az.MAX_DATA)
    assert off.aztec is None and off.az_data is None and off.texts == on.texts and np.array_equal(off.quads, on.quads)
    assert P["threshold"] == arch.DM_PARAMS["threshold"] == arch.QR_PARAMS["threshold"] == arch.BARCODE_PARAMS["threshold"]
    for opts in (dict(marks=True), dict(tables=True), dict(barcodes=True), dict(qrcodes=True), dict(datamatrix=True), dict(barcodes=True, qrcodes=True, datamatrix=True),
                 dict(marks=True, tables=True, datamatrix=True), dict(datamatrix=True, dm_params=dict(arch.DM_PARAMS, threshold=127))):
        (a, _), _ = OcrPipeline(engine, aztec=True, **opts, **kw).run(pages)
        (b, _), _ = OcrPipeline(engine, **opts, **kw).run(pages)
        assert np.array_equal(a.aztec, rc) and np.array_equal(a.az_data, rd), opts
        for name in ("marks", "hrules", "vrules", "barcodes", "barcode_syms", "qrcodes", "qr_data", "datamatrix", "dm_data"):
            va, vb = getattr(a, name), getattr(b, name)
            assert (va is None and vb is None) or np.array_equal(va, vb), (opts, name)
        assert a.texts == on.texts
    (few, _), _ = OcrPipeline(engine, aztec=True, aztec_params=dict(P, max_codes=1), **kw).run(pages)
    assert few.aztec.shape == (0, 12)                                               # an overflowing page reports none
