"""GPU: the provider with LUMINA_OCR_WORD_BOXES=1 — `word` entries carry the device's polygons and confidences, everything else is the
output without the option; single images, page batches, the status; the default provider is unchanged."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_word_boxes, s._use_tables, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_word_boxes, s._use_tables, s.apply_deskew = saved


def _run(s, words: bool, image, tables: bool = False):
    s.cleanup()
    s._use_word_boxes, s._use_tables = words, tables
    return s.process_image_sync(image)


def _words(boxes):
    return [b for b in boxes if b["type"] == "word"]


def _strip(d):
    return {k: v for k, v in d.items() if k not in ("processing_time_ms", "layout_boxes")}


@pytest.fixture(scope="module")
def page_images():
    return [Image.fromarray(synth.synth_page(H, W, 21, n_lines=9)[0]), Image.fromarray(synth.synth_form_page(3)[0])]


@pytest.mark.parametrize("which", [0, 1])
def test_word_boxes_through_the_provider(service, engine, page_images, which):
    image = page_images[which]
    on = _run(service, True, image)
    assert on.success, on.error
    assert service.get_status()["word_boxes"] is True
    off = _run(service, False, image)
    assert off.success and service.get_status()["word_boxes"] is False
    assert layout.validate_layout_boxes(on.layout_boxes) == []
    # every entry that is not a word, and every other field of the result, is the one of the run without the option
    assert [b for b in on.layout_boxes if b["type"] != "word"] == [b for b in off.layout_boxes if b["type"] != "word"]
    assert [b["type"] for b in on.layout_boxes] == [b["type"] for b in off.layout_boxes]
    assert _strip(on.to_dict()) == _strip(off.to_dict()) and on.processed_image_bytes == off.processed_image_bytes
    # words: same contents in the same order, same keys; polygons and confidences are the device's
    w_on, w_off = _words(on.layout_boxes), _words(off.layout_boxes)
    assert len(w_on) >= 10 and [(b["content"], b["page_number"]) for b in w_on] == [(b["content"], b["page_number"]) for b in w_off]
    assert all(list(a) == list(b) for a, b in zip(w_on, w_off))
    assert [b["polygon"] for b in w_on] != [b["polygon"] for b in w_off]
    # ... those of the pipeline on the same page with the provider's seeded networks
    from lumina_ocr.pipeline import OcrPipeline
    import torch
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    pipe = OcrPipeline(engine, charset=charset, post=arch.TEXT_PATH_POST, word_boxes=True)
    dets, _ = pipe.run(torch.from_numpy(np.asarray(image, np.uint8).copy())[None].cuda())
    d = dets[0]
    want = [(d.texts[i][a:a + c], [float(v) for v in q], s) for i, ws in enumerate(d.line_words()) for a, c, q, s in ws]
    key = lambda t: (t[0], t[1], t[2])
    assert sorted(((b["content"], b["polygon"], b["confidence"]) for b in w_on), key=key) == sorted(want, key=key)
    # in reading order too: the words of a line follow each other as the line's text has them
    lines = [b for b in on.layout_boxes if b["type"] == "line"]
    assert [w for ln in lines for w in ln["content"].split()] == [b["content"] for b in w_on]


def test_page_batches_and_tables_carry_the_words(service, page_images):
    service.cleanup()
    service._use_word_boxes, service._use_tables = True, True
    batch = service.process_pages_sync(page_images, first_page_number=3)
    assert all(r.success for r in batch) and [r.page_number for r in batch] == [3, 4]
    single = [_run(service, True, im, tables=True) for im in page_images]
    for k, (b, s) in enumerate(zip(batch, single)):
        fix = lambda boxes: [dict(x, page_number=0) for x in boxes]
        assert fix(b.layout_boxes) == fix(s.layout_boxes) and b.markdown == s.markdown
    off = [_run(service, False, im, tables=True) for im in page_images]
    for s, o in zip(single, off):
        assert s.markdown == o.markdown and s.json_output == o.json_output
        assert [b for b in s.layout_boxes if b["type"] != "word"] == [b for b in o.layout_boxes if b["type"] != "word"]


def test_the_default_provider_is_unchanged(service, page_images, monkeypatch):
    """without the variable the provider builds the pipeline it built before, and its words are the proportional split"""
    from lumina_ocr.services import ocr_service as svc
    monkeypatch.delenv("LUMINA_OCR_WORD_BOXES", raising=False)
    fresh = object.__new__(svc.OCRService)
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_word_boxes is False and fresh.get_status()["word_boxes"] is False
    monkeypatch.setenv("LUMINA_OCR_WORD_BOXES", "1")
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_word_boxes is True
    r = _run(service, False, page_images[0])
    assert r.success and service._pipeline.word_boxes is False
    lines = [(b["polygon"], b["content"], 0.0) for b in r.layout_boxes if b["type"] == "line"]
    guess = [b for b in layout.build_layout_boxes(lines) if b["type"] == "word"]
    got = _words(r.layout_boxes)
    assert [(b["content"], b["polygon"]) for b in got] == [(b["content"], b["polygon"]) for b in guess]
    assert len({b["confidence"] for b in got}) <= len(lines)        # one confidence per line: the line's score
