"""GPU: the orientation classifier through OcrPipeline(angle_cls=True) and the provider (LUMINA_OCR_USE_ANGLE_CLS), against the restated
"oracle pipeline + cls" (tests/cls_reference.py run_pages) — detector text path, recogniser code path, classifier orientation path."""
import numpy as np
import pytest
import torch
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.pipeline import OcrPipeline

import cls_reference as cr

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture(scope="module")
def weights():
    return arch.make_det_weights(1234), arch.make_rec_weights(4321, code_path=True), arch.make_cls_weights(2718, orientation_path=True)


@pytest.fixture(scope="module")
def pages():
    up = synth.synth_page(H, W, 3, n_lines=10, ruled=True)[0]
    return up, np.ascontiguousarray(up[::-1, ::-1])


def _pipe(engine, weights, **kw):
    det_w, rec_w, cls_w = weights
    engine.load_det(det_w)
    engine.load_rec(rec_w)
    engine.load_cls(cls_w)
    return OcrPipeline(engine, max_dimension=2000, post=arch.TEXT_PATH_POST, **kw)


@pytest.mark.parametrize("turned", [False, True])
def test_pipeline_with_angle_cls_equals_the_restatement(engine, weights, pages, turned):
    page = pages[int(turned)]
    pipe = _pipe(engine, weights, angle_cls=True)
    dets, _ = pipe.run(torch.from_numpy(page[None]).cuda())
    ref, _ = cr.run_pages(*weights, page[None], pipe.charset, post=arch.TEXT_PATH_POST)
    d, r = dets[0], ref[0]
    assert len(r["texts"]) >= 8
    assert np.array_equal(d.quads, r["quads"]) and d.texts == r["texts"]
    assert np.array_equal(d.cls_labels, r["labels"]) and (d.cls_labels == int(turned)).all() and (d.cls_scores > 0.9).all()
    plain = OcrPipeline(engine, max_dimension=2000, post=arch.TEXT_PATH_POST)
    off = OcrPipeline(engine, max_dimension=2000, post=arch.TEXT_PATH_POST, angle_cls=False)
    p, _ = plain.run(torch.from_numpy(page[None]).cuda())
    o, _ = off.run(torch.from_numpy(page[None]).cuda())
    assert p[0].texts == o[0].texts and np.array_equal(p[0].quads, o[0].quads) and o[0].cls_labels is None
    if turned:      # the flipped lines read differently from the pipeline without the classifier; the boxes do not move
        assert np.array_equal(p[0].quads, d.quads) and p[0].texts != d.texts
    else:           # upright: nothing is turned, the strings are today's
        assert p[0].texts == d.texts and np.array_equal(p[0].scores, d.scores)


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_angle_cls, s._cls_weights)
    s._allow_synthetic = True
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_angle_cls, s._cls_weights = saved


def _lines(r):
    return [b["content"] for b in r.layout_boxes if b["type"] == "line"]


def test_provider_reads_the_turned_page(service, pages):
    s = service
    turned = Image.fromarray(pages[1])
    s._use_angle_cls = False
    default_turned = s.process_image_sync(turned)
    default_up = s.process_image_sync(Image.fromarray(pages[0]))
    s.cleanup()
    s._use_angle_cls = True                                  # LUMINA_OCR_USE_ANGLE_CLS=1 (+ LUMINA_OCR_ALLOW_SYNTHETIC=1)
    on = s.process_image_sync(turned)
    assert on.success and default_turned.success, (on.error, default_turned.error)
    dets, _ = s._pipeline.run(torch.from_numpy(pages[1][None]).cuda(), deskew=s.apply_deskew)
    assert (dets[0].cls_labels == 1).all() and _lines(on) == dets[0].texts
    assert _lines(on) != _lines(default_turned)
    up = s.process_image_sync(Image.fromarray(pages[0]))    # an upright page reads as it does without the classifier
    assert _lines(up) == _lines(default_up) and up.markdown == default_up.markdown


def test_switch_off_is_the_default_provider(service, pages, monkeypatch):
    """LUMINA_OCR_USE_ANGLE_CLS=0 and the variable unset give the same provider and the same result (its timing aside)."""
    from lumina_ocr.services import ocr_service as svc
    results = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("LUMINA_OCR_USE_ANGLE_CLS", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_USE_ANGLE_CLS", env)
        s = object.__new__(svc.OCRService)
        s._initialized = False
        svc.OCRService.__init__(s)
        s._allow_synthetic = True
        r = s.process_image_sync(Image.fromarray(pages[1]))
        assert r.success and s._use_angle_cls is False and s._pipeline.angle_cls is False
        s.cleanup()
        d = r.to_dict()
        d.pop("processing_time_ms")
        results.append((d, r.processed_image_bytes))
    assert results[0] == results[1]
