"""GPU: barcodes through the provider (LUMINA_OCR_BARCODES=1) and OcrPipeline(barcodes=True) on one synthetic form: the entries carry
what was rendered, nothing the recogniser made of the bars is left, the option off is a provider that never heard of barcodes, and
marks and tables are what they are without it."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import layout

import barcode_reference as br

pytestmark = pytest.mark.gpu

H, W = 700, 1000


@pytest.fixture(scope="module")
def form():
    """text lines above; a Code 128, a reversed Code 39 and a vertical Code 128 below"""
    page = np.full((H, W, 3), 255, np.uint8)
    page[:240] = synth.synth_page(240, W, 11, n_lines=5, noise=0.0)[0]
    gt = []
    for x, y, text, kind, m, height, kw in ((60, 300, "INV-2024/0042", "Code128", 2, 60, {}), (480, 320, "LOT 7", "Code39", 3, 50, dict(reversed=True)),
                                            (880, 280, "990017", "Code128", 3, 40, dict(vertical=True))):
        syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
        gt.append(dict(kind=kind, text=text, box=synth.render_barcode(page, x, y, syms, kind, m, height, **kw)))
    return page, gt


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_tables, s._use_marks, s._use_barcodes, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_tables, s._use_marks, s._use_barcodes, s.apply_deskew = saved


def _run(s, image, barcodes: bool, marks: bool = False, tables: bool = False):
    s.cleanup()
    s._use_barcodes, s._use_marks, s._use_tables = barcodes, marks, tables
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_form_through_the_provider(service, form):
    page, gt = form
    image = Image.fromarray(page)
    r = _run(service, image, True)
    assert r.success, r.error
    assert service.get_status()["barcodes"] is True
    got = [b for b in r.layout_boxes if b["type"] == "barcode"]
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)]
    assert sorted((b["kind"], b["content"], b["polygon"]) for b in got) == sorted((g["kind"], g["text"], rect(g["box"])) for g in gt)
    assert all(b["confidence"] == 1.0 for b in got) and r.json_output["barcodes_count"] == len(gt) == 3
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [b["type"] for b in r.layout_boxes]
    assert types == sorted(types, key=["word", "line", "selection_mark", "barcode", "table", "table_cell", "paragraph"].index)
    assert not [b for b in r.layout_boxes if b["type"] in ("word", "line") and any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    rows = r.markdown.split("\n")
    assert all(":barcode: %s" % g["text"] in rows for g in gt) and r.markdown.count(":barcode:") == 3
    lines = [b for b in r.layout_boxes if b["type"] == "line"]
    assert len(lines) >= 3 and rows.index(":barcode: INV-2024/0042") >= 3           # the text above the codes comes first
    # ---- the switch: off is a provider that never heard of barcodes ----
    off = _run(service, image, False)
    assert off.success and "barcodes_count" not in off.json_output and service.get_status()["barcodes"] is False
    assert not [b for b in off.layout_boxes if b["type"] == "barcode"] and ":barcode:" not in off.markdown
    outside = lambda res: [b for b in res.layout_boxes if b["type"] in ("word", "line") and not any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    assert outside(off) == outside(r)
    assert off.markdown == layout.page_markdown(layout.reading_order([(b["polygon"], b["content"], 1.0) for b in off.layout_boxes if b["type"] == "line"])[0])
    assert r.processed_image_bytes == off.processed_image_bytes
    again = _run(service, image, False)
    assert again.layout_boxes == off.layout_boxes and again.markdown == off.markdown and again.json_output == off.json_output


def test_marks_and_tables_are_unchanged_by_the_barcodes(service):
    page, gt = synth.synth_marks_page(1, 640, 896, n_marks=6, stroke=2, max_side=40)       # 6 boxes in the columns, 4 in the table's cells
    page = page.copy()
    box = synth.render_barcode(page, 40, 590, synth.code128_symbols("MIXED-1"), "Code128", 2, 40)
    image = Image.fromarray(page)
    with_codes, without = _run(service, image, True, marks=True, tables=True), _run(service, image, False, marks=True, tables=True)
    assert with_codes.success and without.success
    pick = lambda r, *types: [b for b in r.layout_boxes if b["type"] in types]
    assert pick(with_codes, "selection_mark", "table", "table_cell") == pick(without, "selection_mark", "table", "table_cell")
    assert len(pick(without, "selection_mark")) == len(gt) == 10 and len(pick(without, "table")) == 1
    assert [(b["content"], b["polygon"][:2]) for b in pick(with_codes, "barcode")] == [("MIXED-1", [float(box[0]), float(box[1])])]
    assert {k: v for k, v in with_codes.json_output.items() if k not in ("barcodes_count", "words_count", "lines_count", "paragraphs_count")} == \
           {k: v for k, v in without.json_output.items() if k not in ("words_count", "lines_count", "paragraphs_count")}


def test_pipeline_barcodes_equal_the_restatement_and_off_is_none(engine, form):
    import torch
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    pages = torch.from_numpy(np.stack([form[0], np.full((H, W, 3), 255, np.uint8)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, blank), processed = OcrPipeline(engine, barcodes=True, **kw).run(pages)
    (off, _), _ = OcrPipeline(engine, **kw).run(pages)
    _, rc, rs = br.barcodes(processed[0].cpu().numpy())
    assert np.array_equal(on.barcodes, rc) and np.array_equal(on.barcode_syms, rs) and on.barcodes.dtype == np.int32 and len(rc) == 3
    assert [f["content"] for f in bc.read_barcodes(on.barcodes, on.barcode_syms)] == br.decoded(rc, rs)
    assert blank.barcodes.shape == (0, 8) and blank.barcode_syms.shape == (0, 64)
    assert off.barcodes is None and off.barcode_syms is None and off.texts == on.texts and np.array_equal(off.quads, on.quads)
    # the ink mask handed over by the marks or the tables call (each on its own at the barcodes' threshold), and the joint call, which
    # hands none: the same barcodes, and marks and rules as without them
    assert arch.BARCODE_PARAMS["threshold"] == arch.MARK_PARAMS["threshold"] == arch.TABLE_PARAMS["threshold"]
    for opts in (dict(marks=True), dict(marks=True, round_marks=True), dict(tables=True), dict(marks=True, tables=True),
                 dict(marks=True, mark_params=dict(arch.MARK_PARAMS, threshold=127))):
        (a, _), _ = OcrPipeline(engine, barcodes=True, **opts, **kw).run(pages)
        (b, _), _ = OcrPipeline(engine, **opts, **kw).run(pages)
        assert np.array_equal(a.barcodes, rc) and np.array_equal(a.barcode_syms, rs), opts
        for name in ("marks", "round_marks", "hrules", "vrules"):
            va, vb = getattr(a, name), getattr(b, name)
            assert (va is None and vb is None) or np.array_equal(va, vb), (opts, name)
        assert a.texts == on.texts
    (few, _), _ = OcrPipeline(engine, barcodes=True, barcode_params=dict(arch.BARCODE_PARAMS, max_codes=2), **kw).run(pages)
    assert few.barcodes.shape == (0, 8)                                            # an overflowing page reports none
