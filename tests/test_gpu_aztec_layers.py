"""GPU: lumina_ocr_aztec_layers through the C ABI against the restatement (tests/aztec_layers_reference.py): the ink mask, the rows, the
data codewords, the counts and the finder counts are EQUAL (integer arithmetic, a canonical order: no tolerance), and the decoded
strings are what was rendered.  Pages are as small as their symbols allow."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import aztec as az

import aztec_layers_pages as LP
import aztec_layers_reference as R2
import aztec_pages as AP

pytestmark = pytest.mark.gpu

P = arch.AZTEC_PARAMS
KEYS = ("min_module", "max_module", "quiet", "centre_tol", "ring_tol", "mark_max", "max_finders")
ORDER = ("threshold",) + KEYS + ("max_codes",)


def check(engine, pages: np.ndarray, max_layers: int = 32, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, finders) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    codes, data, cnt, mask, nf = engine.aztec_layers(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_layers, max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    codes, data, cnt, mask, nf = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64), nf.cpu().numpy()
    assert data.dtype == np.uint16 and data.shape[1:] == (cap, az.MAX_DATA_ALL)
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rd, rn = LP.reference(page, max_layers, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nf[i]) == rn, "page %d: %d finders, restatement %d" % (i, nf[i], rn)
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rc), rc)
        n = len(rc) if len(rc) <= cap else 0
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(data[i, :n], rd[:n]), "page %d: data codewords differ" % i
        assert not codes[i, n:].any() and not data[i, n:].any(), "page %d: rows past the count were written" % i
        out.append((rc, rd, rn))
    return out


def found(rc, rd):
    """-> {(x0, y0, x1, y1): text}"""
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R2.texts(rc, rd))}


@pytest.mark.parametrize("layers", LP.SIZES)
def test_every_kind_of_size_reads(engine, layers):
    """32 layers is the test that fails without the entry: lumina_ocr_aztec gives that page an empty list"""
    page, box, text = LP.page_of(layers, rotation=layers % 4)
    (rc, rd, rn), = check(engine, page[None])
    assert found(rc, rd) == {box: text} and rn == 1
    assert tuple(rc[0][4:12]) == (layers, 0, az.word_width(layers), az.symbol_words(text, False, layers)[1], 0, layers % 4, 0, 0)
    old = engine.aztec(torch.from_numpy(page[None]).cuda())
    assert int(old[2][0]) == 0


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_every_rotation_at_12_and_27_layers(engine, rotation):
    for layers in (12, 27):
        page, box, text = LP.page_of(layers, rotation=rotation, text="ROT %d of %d layers. " % (rotation, layers) * 9)
        (rc, rd, _), = check(engine, page[None])
        assert found(rc, rd) == {box: text} and int(rc[0][9]) == rotation


@pytest.mark.parametrize("layers,module", [(23, 4), (12, 7)])
def test_other_pitches(engine, layers, module):
    page, box, text = LP.page_of(layers, module, 1, margin=(14, 10))
    (rc, rd, _), = check(engine, page[None])
    assert found(rc, rd) == {box: text}


@pytest.mark.parametrize("layers", [22, 23])
def test_most_errors_the_block_corrects_and_one_more(engine, layers):
    """GF(1024) and GF(4096) with ec // 2 codewords destroyed, and with one more"""
    text = LP.nearly_full(layers)
    t = AP.capacity(False, layers, text)
    good, box, _ = LP.page_of(layers, text=text, matrix=AP.corrupted(text, False, layers, t))
    bad, _, _ = LP.page_of(layers, text=text, matrix=AP.corrupted(text, False, layers, t + 1))
    res = check(engine, np.stack([good, bad]))
    assert found(*res[0][:2]) == {box: text} and int(res[0][0][0][8]) == t and 12 <= t <= 32
    assert len(res[1][0]) == 0 and res[1][2] == 1


def test_mixed_page_is_in_order_and_stage_one_rows_are_the_old_entrys(engine):
    page = AP.blank(300, 560)
    a = AP.put(page, 8, 11, "COMPACT TWO", True, 2)
    b = AP.put(page, 90, 6, LP.payload(11), False, 11, 3, 2)
    c = AP.put(page, 290, 20, LP.payload(16), False, 16, 3, 3)
    (rc, rd, _), = check(engine, page[None])
    assert found(rc, rd) == {a: "COMPACT TWO", b: LP.payload(11), c: LP.payload(16)}
    assert [tuple(r[:4]) for r in rc] == sorted((a, b, c), key=lambda t: (t[1], t[0]))
    dev = torch.from_numpy(page[None]).cuda()
    old, new = engine.aztec(dev), engine.aztec_layers(dev, 32)
    torch.cuda.synchronize()
    assert int(old[2][0]) == 2 and int(new[2][0]) == 3
    keep = [i for i in range(3) if int(new[0][0, i, 4]) <= 11]
    data = new[1].cpu().numpy()[0]
    assert np.array_equal(new[0].cpu().numpy()[0, keep], old[0].cpu().numpy()[0, :2]) and np.array_equal(data[keep, :320], old[1].cpu().numpy()[0, :2])
    assert not data[keep, 320:].any()


def test_stage_one_pages_equal_the_old_entry_at_any_cap(engine):
    """decoys, text and small symbols: the list of lumina_ocr_aztec, with max_layers at 32 and at 11"""
    decoys, _ = AP.decoys(150, 430)
    small = AP.blank(*decoys.shape[:2])
    x = 7
    for i, (compact, layers) in enumerate(((True, 1), (True, 4), (False, 1), (False, 6))):
        AP.put(small, x, 5 + 3 * i, AP.payload(compact, layers), compact, layers, 3, i)
        x += AP.side_px(compact, layers) + 11
    text = synth.synth_page(decoys.shape[0], decoys.shape[1], 5, n_lines=5)[0]
    pages = np.stack([decoys, small, text])
    dev = torch.from_numpy(pages).cuda()
    old = engine.aztec(dev, debug=True)
    for cap in (32, 11):
        res = check(engine, pages, cap)
        new = engine.aztec_layers(dev, cap, debug=True)
        torch.cuda.synchronize()
        assert torch.equal(new[0], old[0]) and torch.equal(new[2], old[2]) and torch.equal(new[4], old[4]) and new[2].tolist() == [0, 4, 0]
        data = new[1].cpu().numpy()
        assert np.array_equal(data[:, :, :320], old[1].cpu().numpy()) and not data[:, :, 320:].any()
        assert len(res[1][0]) == 4


def test_a_symbol_above_the_cap_gives_no_row(engine):
    page, box, text = LP.page_of(23)
    (rc, _, rn), = check(engine, page[None], 20)
    assert len(rc) == 0 and rn == 1
    (rc, rd, _), = check(engine, page[None], 23)
    assert found(rc, rd) == {box: text}


def test_page_edges_count_as_quiet_and_ink_a_module_off_does_not(engine):
    s = AP.side_px(False, 12)
    pages = np.stack([AP.blank(s + 30, s + 40) for _ in range(3)])
    a = AP.put(pages[0], 0, 0, LP.payload(12), False, 12, 3, 1)
    b = AP.put(pages[1], 40, 30, LP.payload(12), False, 12, 3, 2)
    c = AP.put(pages[2], 5, 5, LP.payload(12), False, 12)
    pages[2][c[1] + 40:c[1] + 46, c[2] + 2:c[2] + 4] = 0                   # ink one module off the right side
    res = check(engine, pages, quiet=1)
    assert found(*res[0][:2]) == {a: LP.payload(12)} and found(*res[1][:2]) == {b: LP.payload(12)}
    assert len(res[2][0]) == 0 and res[2][2] == 1
    (rc, rd, _), = check(engine, pages[2:], quiet=0)
    assert found(rc, rd) == {c: LP.payload(12)}


@pytest.mark.parametrize("layers", [12, 22, 32])
def test_tilted_pages_equal_the_restatement_and_read(engine, layers):
    text = LP.payload(layers, "TILT ")
    page, _, _ = LP.page_of(layers, rotation=layers % 3, text=text, margin=(22, 20))
    tilts = [d for l, d in LP.TILTS if l == layers]
    res = check(engine, np.stack([AP.tilted(page, d) for d in tilts]))
    assert [R2.texts(*r[:2]) for r in res] == [[text]] * len(tilts)


def test_ragged_page_groups(engine):
    pages = np.stack([LP.page_of(12, rotation=i, text="PAGE %d of the ragged groups" % i)[0] for i in range(4)])
    engine.set_option("post_group", 3)
    try:
        res = check(engine, pages)
    finally:
        engine.set_option("post_group", 64)
    assert [R2.texts(*r[:2]) for r in res] == [["PAGE %d of the ragged groups" % i] for i in range(4)]


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(AP.blank(64, 200)[None]).cuda()
    good = dict(P, max_codes=4, max_layers=32)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_layers=10), dict(max_layers=33), dict(max_codes=0), dict(max_codes=65), dict(max_finders=0), dict(quiet=5), dict(ring_tol=16)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), az.MAX_DATA_ALL), -7, dtype=torch.int16, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_aztec_layers(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in ORDER], kw["max_layers"], codes.data_ptr(),
                                                data.data_ptr(), counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        err = engine.lib.lumina_ocr_last_error(engine._h)
        assert rc != 0 and b"aztec_layers" in err and b"max_layers 11..32" in err, bad
        assert bool((codes == -7).all()) and bool((data == -7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError, match="aztec_layers"):
            engine.aztec_layers(pages, kw["max_layers"], **{k: kw[k] for k in ORDER})
    buf = torch.zeros((1, 4, az.MAX_DATA_ALL), dtype=torch.int32, device="cuda")
    for args in ((None, buf.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_aztec_layers(engine._h, args[0], 1, 64, 200, *[good[k] for k in ORDER], 32, args[1], buf.data_ptr(), buf.data_ptr(), None, None,
                                                None, st)
        assert rc != 0 and b"aztec_layers: bad arguments" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_aztec_layers(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in ORDER], 32, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                            None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    ws, ws1 = engine.lib.lumina_ocr_aztec_layers_workspace_bytes, engine.lib.lumina_ocr_aztec_workspace_bytes
    assert ws(2, 64, 200, 64, 16) > ws(1, 64, 200, 64, 16) > ws1(1, 64, 200, 64, 16) > 0
    assert ws(1, 0, 200, 64, 16) == 0 and ws(1, 64, 200, 65, 16) == 0 and ws(0, 64, 200, 64, 16) == 0
    with pytest.raises(TypeError):
        engine.aztec_layers(pages, 32, timing_max=3)


def test_pipeline_reads_the_large_symbol_with_the_option_and_not_without(engine):
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    form = AP.blank(540, 620)
    form[:150] = synth.synth_page(150, 620, 3, n_lines=3, noise=0.0)[0]
    big = AP.put(form, 30, 180, LP.payload(16), False, 16, 4, 1)
    AP.put(form, 400, 200, "COMPACT", True, 1, 4)
    pages = torch.from_numpy(np.stack([form, AP.blank(540, 620)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, empty), processed = OcrPipeline(engine, aztec=True, aztec_max_layers=32, **kw).run(pages)
    (default, _), _ = OcrPipeline(engine, aztec=True, **kw).run(pages)
    _, rc, rd, _ = LP.reference(processed[0].cpu().numpy())
    assert np.array_equal(on.aztec, rc) and np.array_equal(on.az_data, rd) and on.az_data.dtype == np.uint16 and on.az_data.shape == (2, az.MAX_DATA_ALL)
    assert sorted(R2.texts(on.aztec, on.az_data)) == sorted(["COMPACT", LP.payload(16)]) and big is not None
    assert empty.aztec.shape == (0, 12) and empty.az_data.shape == (0, az.MAX_DATA_ALL)
    assert [e["content"] for e in az.read_aztec(default.aztec, default.az_data)] == ["COMPACT"] and default.az_data.shape == (1, az.MAX_DATA)
    assert default.texts == on.texts
    for bad in (10, 33):
        with pytest.raises(ValueError, match="aztec_max_layers"):
            OcrPipeline(engine, aztec=True, aztec_max_layers=bad, **kw)
