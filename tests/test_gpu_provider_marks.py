"""GPU: selection marks through the provider (LUMINA_OCR_SELECTION_MARKS=1) and OcrPipeline(marks=True), against the restated pipeline
(oracle.pipeline + tests/mark_reference.py + lumina_ocr/utils/marks.py) and the ground truth of synth.synth_marks_page; marks and
tables together; the option off."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout

import mark_reference as mr
import table_reference as tr

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture(scope="module")
def mark_pages():
    """(page, ground truth) x 2: form pages with boxes beside their labels and, on the first, a ruled table with boxes in its cells"""
    return [synth.synth_marks_page(1, H, W, n_marks=6, stroke=2, max_side=40), synth.synth_marks_page(4, H, W, n_marks=10, table=False, noise=2.0, max_side=36)]


@pytest.fixture(scope="module")
def restated(mark_pages):
    """the provider's seeded synthetic networks (LUMINA_OCR_ALLOW_SYNTHETIC=1) through the restated pipeline, per page, rules included"""
    charset = arch.ctc_charset()
    det_w, rec_w = arch.make_det_weights(), arch.make_rec_weights(num_classes=len(charset), code_path=True)
    out, _ = mr.run_pages(det_w, rec_w, np.stack([p for p, _ in mark_pages]), charset, post=arch.TEXT_PATH_POST, table_params=True)
    return out


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_tables, s._use_marks, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False      # (the restated pipeline has no de-skew step; these pages are upright)
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_tables, s._use_marks, s.apply_deskew = saved


def _run(s, marks: bool, tables: bool, image):
    s.cleanup()
    s._use_marks, s._use_tables = marks, tables
    return s.process_image_sync(image)


def _comparable(boxes):
    """words without their confidence (the recogniser's fp32 mean on the device, fp64 in the restatement)"""
    return [{k: v for k, v in b.items() if not (b["type"] == "word" and k == "confidence")} for b in boxes]


def _without(d: dict, *keys):
    return {k: v for k, v in d.items() if k not in keys}


@pytest.mark.parametrize("which", [0, 1])
def test_marks_page_through_the_provider(service, mark_pages, restated, which):
    page, gt = mark_pages[which]
    image = Image.fromarray(page)
    r = _run(service, True, False, image)
    assert r.success, r.error
    got = [b for b in r.layout_boxes if b["type"] == "selection_mark"]
    # ---- the ground truth: every drawn box, with its state, and nothing else (the pages are upright and keep their size) ----
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2], b[1], b[2], b[3], b[0], b[3])]
    assert sorted((m["polygon"], m["state"]) for m in got) == sorted((rect(g["box"]), g["state"]) for g in gt)
    assert r.json_output["selection_marks_count"] == len(gt) and r.json_output["tables_count"] == 0
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [b["type"] for b in r.layout_boxes]
    assert types == sorted(types, key=["word", "line", "selection_mark", "table", "table_cell", "paragraph"].index)
    assert r.markdown.count(":selected:") + r.markdown.count(":unselected:") == len(gt)
    # ---- boxes, strings and counts against the restated pipeline (its rules left aside) ----
    ref_boxes, ref_md, ref_found = mr.page_result(_without(restated[which], "hrules", "vrules"))
    assert len(ref_found) == len(gt) and r.markdown == ref_md
    assert _comparable(r.layout_boxes) == _comparable(ref_boxes)
    # ---- the switch: off is a provider that never heard of marks ----
    off = _run(service, False, False, image)
    assert off.success and "selection_marks_count" not in off.json_output
    assert off.layout_boxes == [b for b in r.layout_boxes if b["type"] != "selection_mark"]
    assert off.markdown == layout.page_markdown(layout.reading_order([(b["polygon"], b["content"], 1.0) for b in r.layout_boxes if b["type"] == "line"])[0])
    d_on, d_off = r.to_dict(), off.to_dict()
    for d in (d_on, d_off):
        for k in ("processing_time_ms", "markdown", "html", "layout_boxes"):
            d.pop(k)
    assert _without(d_on["json_output"], "selection_marks_count") == d_off["json_output"]
    assert _without(d_on, "json_output") == _without(d_off, "json_output") and r.processed_image_bytes == off.processed_image_bytes


def test_marks_and_tables_together_equal_the_restatement_and_their_solo_runs(service, mark_pages, restated):
    page, gt = mark_pages[0]
    image = Image.fromarray(page)
    both = _run(service, True, True, image)
    assert both.success, both.error
    ref_boxes, ref_md, _ = mr.page_result(restated[0])
    assert both.markdown == ref_md and _comparable(both.layout_boxes) == _comparable(ref_boxes)
    assert both.json_output["tables_count"] == 1 and both.json_output["selection_marks_count"] == len(gt)
    assert layout.validate_layout_boxes(both.layout_boxes) == []
    in_cells = sum(g["in_table"] for g in gt)
    assert in_cells == 4 and sum(td.count(":selected:") + td.count(":unselected:") for td in both.markdown.split("<td>")[1:]) >= in_cells
    # each half equals its solo run: the shared mask changes nothing
    marks_only, tables_only = _run(service, True, False, image), _run(service, False, True, image)
    pick = lambda r, *types: [b for b in r.layout_boxes if b["type"] in types]
    assert pick(both, "selection_mark") == pick(marks_only, "selection_mark")
    assert pick(both, "table", "table_cell") == pick(tables_only, "table", "table_cell")
    assert pick(both, "word", "line", "paragraph") == pick(marks_only, "word", "line", "paragraph") == pick(tables_only, "word", "line", "paragraph")
    ref_t_boxes, ref_t_md, _ = tr.page_result(restated[0])
    assert tables_only.markdown == ref_t_md and _comparable(tables_only.layout_boxes) == _comparable(ref_t_boxes)


def test_pipeline_marks_equal_the_restatement_and_off_is_none(engine, mark_pages, restated):
    import torch
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    pages = torch.from_numpy(np.stack([p for p, _ in mark_pages])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    on, _ = OcrPipeline(engine, marks=True, **kw).run(pages)
    both, _ = OcrPipeline(engine, marks=True, tables=True, **kw).run(pages)
    split, _ = OcrPipeline(engine, marks=True, tables=True, table_params=dict(arch.TABLE_PARAMS, threshold=127), **kw).run(pages)   # two thresholds: two masks
    off, _ = OcrPipeline(engine, **kw).run(pages)
    for d, bt, sp, o, ref in zip(on, both, split, off, restated):
        assert np.array_equal(d.marks, ref["marks"]) and len(d.marks) >= 6 and d.marks.dtype == np.int32 and d.hrules is None
        assert np.array_equal(bt.marks, ref["marks"]) and np.array_equal(bt.hrules, ref["hrules"]) and np.array_equal(bt.vrules, ref["vrules"])
        assert np.array_equal(sp.marks, ref["marks"]) and sp.hrules is not None
        assert o.marks is None and o.hrules is None
        assert d.texts == bt.texts == o.texts == ref["texts"] and np.array_equal(d.quads, o.quads) and np.array_equal(d.quads, ref["quads"])
    assert len(both[0].hrules) >= 3 and len(both[0].vrules) >= 3
    blank, _ = OcrPipeline(engine, marks=True, **kw).run(torch.full((2, 320, 448, 3), 255, dtype=torch.uint8, device="cuda"))
    assert all(len(b.texts) == 0 and b.marks.shape == (0, 8) for b in blank)      # pages without a line still report
    few, _ = OcrPipeline(engine, marks=True, mark_params=dict(arch.MARK_PARAMS, max_marks=2), **kw).run(pages)
    assert all(f.marks.shape == (0, 8) for f in few)                               # an overflowing page reports none
