"""GPU: radio buttons through OcrPipeline(marks=True, round_marks=True) and the provider (LUMINA_OCR_SELECTION_MARKS=1 +
LUMINA_OCR_RADIO_BUTTONS=1) with tables on, against the restated pipeline (tests/radio_reference.run_pages) and the ground truth of
synth.synth_radio_page; the option off; the option without the checkboxes' option."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout

import radio_reference as rr
from test_gpu_provider_marks import _comparable, _without

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture(scope="module")
def radio_page():
    return synth.synth_radio_page(1, H, W, n_marks=6, max_side=40)


@pytest.fixture(scope="module")
def restated(radio_page):
    charset = arch.ctc_charset()
    det_w, rec_w = arch.make_det_weights(), arch.make_rec_weights(num_classes=len(charset), code_path=True)
    out, _ = rr.run_pages(det_w, rec_w, radio_page[0][None], charset, post=arch.TEXT_PATH_POST, table_params=True)
    return out[0]


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_tables, s._use_marks, s._use_round_marks, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_tables, s._use_marks, s._use_round_marks, s.apply_deskew = saved


def _run(s, marks: bool, rounds: bool, image):
    s.cleanup()
    s._use_marks, s._use_round_marks, s._use_tables = marks, rounds, True
    return s.process_image_sync(image)


def test_radio_page_through_the_provider_with_tables(service, radio_page, restated):
    page, gt = radio_page
    assert [g["shape"] for g in gt].count("round") == 9 and sum(g["in_table"] for g in gt) == 4
    image = Image.fromarray(page)
    r = _run(service, True, True, image)
    assert r.success, r.error
    got = [b for b in r.layout_boxes if b["type"] == "selection_mark"]
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2], b[1], b[2], b[3], b[0], b[3])]
    assert sorted((m["polygon"], m["state"]) for m in got) == sorted((rect(g["box"]), g["state"]) for g in gt)       # the ground truth
    assert r.json_output["selection_marks_count"] == len(gt) and r.json_output["tables_count"] == 1
    assert all(set(m) == {"type", "state", "confidence", "polygon", "page_number"} for m in got) and layout.validate_layout_boxes(r.layout_boxes) == []
    assert r.markdown.count(":selected:") + r.markdown.count(":unselected:") == len(gt)
    assert sum(td.count(":selected:") + td.count(":unselected:") for td in r.markdown.split("<td>")[1:]) >= 4          # the group in the table
    ref_boxes, ref_md, ref_found = rr.page_result(restated)                                                            # the restated pipeline
    assert len(ref_found) == len(gt) and r.markdown == ref_md and _comparable(r.layout_boxes) == _comparable(ref_boxes)
    # ---- the option off: the provider with checkboxes only, which equals mark_reference's restated page ----
    import mark_reference as mr
    off = _run(service, True, False, image)
    off_boxes, off_md, off_found = mr.page_result(_without(restated, "round_marks"))
    assert off.success and off.markdown == off_md and _comparable(off.layout_boxes) == _comparable(off_boxes)
    assert off.json_output["selection_marks_count"] == len(off_found) == sum(g["shape"] == "square" for g in gt)
    pick = lambda res, *types: [b for b in res.layout_boxes if b["type"] in types]
    assert pick(off, "word", "line", "table", "table_cell", "paragraph") == pick(r, "word", "line", "table", "table_cell", "paragraph")
    assert r.processed_image_bytes == off.processed_image_bytes


def test_the_option_without_selection_marks_is_an_error_result(service, radio_page):
    r = _run(service, False, True, Image.fromarray(radio_page[0]))
    assert not r.success and "LUMINA_OCR_SELECTION_MARKS" in (r.error or "") and r.layout_boxes in ([], None)


def test_pipeline_round_marks_equal_the_restatement_and_off_is_none(engine, radio_page, restated):
    import torch
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    pages = torch.from_numpy(radio_page[0][None]).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on,), _ = OcrPipeline(engine, marks=True, round_marks=True, **kw).run(pages)
    (both,), _ = OcrPipeline(engine, marks=True, round_marks=True, tables=True, **kw).run(pages)
    (split,), _ = OcrPipeline(engine, marks=True, round_marks=True, tables=True, table_params=dict(arch.TABLE_PARAMS, threshold=127), **kw).run(pages)
    (off,), _ = OcrPipeline(engine, marks=True, tables=True, **kw).run(pages)
    for d in (on, both, split):
        assert np.array_equal(d.round_marks, restated["round_marks"]) and d.round_marks.dtype == np.int32 and len(d.round_marks) == 9
        assert np.array_equal(d.marks, restated["marks"]) and d.texts == restated["texts"] and np.array_equal(d.quads, restated["quads"])
    assert on.hrules is None and np.array_equal(both.hrules, restated["hrules"]) and np.array_equal(both.vrules, restated["vrules"])
    assert off.round_marks is None and np.array_equal(off.marks, both.marks) and np.array_equal(off.hrules, both.hrules) and off.texts == both.texts
    (few,), _ = OcrPipeline(engine, marks=True, round_marks=True, mark_params=dict(arch.MARK_PARAMS, max_marks=2), **kw).run(pages)
    assert few.round_marks.shape == (0, 8)                                           # an overflowing page reports none
    (blank,), _ = OcrPipeline(engine, marks=True, round_marks=True, **kw).run(torch.full((1, 320, 448, 3), 255, dtype=torch.uint8, device="cuda"))
    assert len(blank.texts) == 0 and blank.round_marks.shape == (0, 8) and blank.marks.shape == (0, 8)
    with pytest.raises(ValueError):
        OcrPipeline(engine, marks=False, round_marks=True, **kw)
