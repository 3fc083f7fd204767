"""GPU: ruled tables through the provider (LUMINA_OCR_TABLES=1) and OcrPipeline(tables=True), against the ground truth of
synth.synth_table_page and against the restated pipeline (oracle.pipeline + tests/table_reference.py + lumina_ocr/utils/tables.py).

Text inset: the hand-set detector text path joins a cell's text with the rules around it when they are close.  Measured on the CPU with
the restated pipeline on 640 x 896 pages (seeds 1-5, thickness 2-5, with and without spans): at inset 20, 19 of 46 cell texts were not a
detection of their own (the whole table came back as one line at inset <= 14); at 24, 28, 32 and 40 every one was.  The pages here use 28."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout, tables

import table_reference as tr

pytestmark = pytest.mark.gpu

H, W, INSET = 640, 896, 28
SNAP = arch.TABLE_PARAMS["snap"]


@pytest.fixture(scope="module")
def table_pages():
    """(page, ground truth) x 2: a 4 x 3 table with a header across the columns and a cell across two rows; a page of plain tables"""
    return [synth.synth_table_page(1, H, W, inset=INSET, spans=True, rows=4, cols=3, noise=2.0), synth.synth_table_page(5, H, W, inset=INSET, thickness=2, n_tables=2)]


@pytest.fixture(scope="module")
def restated(table_pages):
    """the provider's seeded synthetic networks (LUMINA_OCR_ALLOW_SYNTHETIC=1) through the restated pipeline, per page"""
    charset = arch.ctc_charset()
    det_w, rec_w = arch.make_det_weights(), arch.make_rec_weights(num_classes=len(charset), code_path=True)
    out, _ = tr.run_pages(det_w, rec_w, np.stack([p for p, _ in table_pages]), charset, post=arch.TEXT_PATH_POST)
    return out


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_tables, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False      # (the restated pipeline has no de-skew step; these pages are upright)
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_tables, s.apply_deskew = saved


def _run(s, on: bool, image):
    s.cleanup()
    s._use_tables = on
    return s.process_image_sync(image)


def _near(poly, want):
    return len(poly) == 8 and all(abs(a - b) <= SNAP for a, b in zip(poly, want))


def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def _comparable(boxes):
    """words without their confidence (the recogniser's fp32 mean on the device, fp64 in the restatement)"""
    return [{k: v for k, v in b.items() if not (b["type"] == "word" and k == "confidence")} for b in boxes]


@pytest.mark.parametrize("which", [0, 1])
def test_table_page_through_the_provider(service, table_pages, restated, which):
    page, gt = table_pages[which]
    r = _run(service, True, Image.fromarray(page))
    assert r.success, r.error
    tabs = [b for b in r.layout_boxes if b["type"] == "table"]
    cells = [b for b in r.layout_boxes if b["type"] == "table_cell"]
    assert len(tabs) == len(gt) >= 1 and r.json_output["tables_count"] == len(gt)
    assert [t["table_index"] for t in tabs] == list(range(len(gt)))
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [b["type"] for b in r.layout_boxes]
    order = ["word", "line", "table", "table_cell", "paragraph"]
    assert [k for k in types if k not in ("table", "table_cell")] == sorted((k for k in types if k not in ("table", "table_cell")), key=order.index)
    assert max(i for i, k in enumerate(types) if k == "line") < types.index("table") and types.index("paragraph") > max(i for i, k in enumerate(types) if k == "table_cell")
    # ---- structure and geometry against the ground truth ----
    ci = 0
    lines = [b for b in r.layout_boxes if b["type"] == "line"]
    for t, g in zip(tabs, gt):
        assert (t["row_count"], t["column_count"]) == (g["row_count"], g["column_count"])
        assert _near(t["polygon"], _rect(g["xs"][0], g["ys"][0], g["xs"][-1], g["ys"][-1]))
        for c in g["cells"]:
            cell = cells[ci]
            ci += 1
            assert (cell["row_index"], cell["column_index"], cell.get("row_span", 1), cell.get("column_span", 1)) == \
                (c["row_index"], c["column_index"], c["row_span"], c["column_span"])
            assert _near(cell["polygon"], _rect(g["xs"][c["column_index"]], g["ys"][c["row_index"]], g["xs"][c["column_index"] + c["column_span"]],
                                                g["ys"][c["row_index"] + c["row_span"]]))
            # the cell's rendered text is one detection of its own (centre inside the text's box), and that line is the cell's content
            bx = c["box"]
            own = [ln for ln in lines if bx[0] - 4 <= tables.quad_centre(ln["polygon"])[0] <= bx[2] + 4 and bx[1] - 4 <= tables.quad_centre(ln["polygon"])[1] <= bx[3] + 4]
            assert len(own) == 1 and own[0]["content"] and cell["content"] == own[0]["content"], (c, own, cell)
    assert ci == len(cells)
    assert r.markdown.count("<table>") == len(gt) == r.markdown.count("</table>") and r.markdown.count("<tr>") == sum(g["row_count"] for g in gt)
    if which == 0:
        assert 'colspan="3"' in r.markdown and 'rowspan="2"' in r.markdown
    assert r.markdown.splitlines()[0] != "<table>"        # the title line stays in the plain flow, before the table
    # ---- boxes, strings and cell contents against the restated pipeline ----
    ref_boxes, ref_md, ref_tabs = tr.page_result(restated[which])
    assert len(ref_tabs) == len(gt) and r.markdown == ref_md
    assert _comparable(r.layout_boxes) == _comparable(ref_boxes)
    # ---- the switch: off is today's provider ----
    off = _run(service, False, Image.fromarray(page))
    assert off.success and off.json_output["tables_count"] == 0 and not any(b["type"] in ("table", "table_cell") for b in off.layout_boxes)
    assert off.layout_boxes == [b for b in r.layout_boxes if b["type"] not in ("table", "table_cell")]
    assert "<table>" not in off.markdown and off.markdown == layout.page_markdown(layout.reading_order(
        [(b["polygon"], b["content"], 1.0) for b in r.layout_boxes if b["type"] == "line"])[0])
    d_on, d_off = r.to_dict(), off.to_dict()
    for d in (d_on, d_off):
        for k in ("processing_time_ms", "markdown", "html", "layout_boxes"):
            d.pop(k)
        d["json_output"] = dict(d["json_output"], tables_count=0)
    assert d_on == d_off and r.processed_image_bytes == off.processed_image_bytes


def test_pipeline_rules_equal_the_restatement_and_off_is_none(engine, table_pages, restated):
    import torch
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    pages = torch.from_numpy(np.stack([p for p, _ in table_pages])).cuda()
    on, _ = OcrPipeline(engine, charset=charset, post=arch.TEXT_PATH_POST, tables=True).run(pages)
    off, _ = OcrPipeline(engine, charset=charset, post=arch.TEXT_PATH_POST).run(pages)
    for d, o, ref in zip(on, off, restated):
        assert np.array_equal(d.hrules, ref["hrules"]) and np.array_equal(d.vrules, ref["vrules"]) and len(d.hrules) >= 2
        assert o.hrules is None and o.vrules is None
        assert d.texts == o.texts == ref["texts"] and np.array_equal(d.quads, o.quads) and np.array_equal(d.quads, ref["quads"])
    blank, _ = OcrPipeline(engine, charset=charset, post=arch.TEXT_PATH_POST, tables=True).run(torch.full((2, 320, 448, 3), 255, dtype=torch.uint8, device="cuda"))
    assert all(len(b.texts) == 0 and b.hrules.shape == (0, 5) and b.vrules.shape == (0, 5) for b in blank)      # pages without a line still report


def test_table_index_runs_over_the_pages_of_a_document(service, table_pages):
    service.cleanup()
    service._use_tables = True
    images = [Image.fromarray(table_pages[k][0]) for k in (0, 1, 0)]
    res = service.process_pages_sync(images)
    assert all(r.success for r in res)
    counts = [len(table_pages[k][1]) for k in (0, 1, 0)]
    assert [r.json_output["tables_count"] for r in res] == counts
    idx = [[b["table_index"] for b in r.layout_boxes if b["type"] == "table"] for r in res]
    flat = [i for page in idx for i in page]
    assert flat == list(range(sum(counts))) and [len(p) for p in idx] == counts
    single = service.process_image_sync(images[1], page_number=2)
    strip = lambda boxes: [dict(b, table_index=0) if b["type"] == "table" else b for b in boxes]
    assert strip(single.layout_boxes) == strip(res[1].layout_boxes) and single.markdown == res[1].markdown
    doc = service._document_from_pages(res, 0.0)
    assert [b["table_index"] for b in doc.combined_layout_boxes if b["type"] == "table"] == flat and doc.combined_markdown.count("<table>") == sum(counts)


def test_environment_switch(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    for env, want in ((None, False), ("0", False), ("1", True), ("true", True)):
        if env is None:
            monkeypatch.delenv("LUMINA_OCR_TABLES", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_TABLES", env)
        s = object.__new__(svc.OCRService)
        s._initialized = False
        svc.OCRService.__init__(s)
        assert s._use_tables is want
