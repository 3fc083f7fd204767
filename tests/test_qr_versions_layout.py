"""Host side of the all-versions QR option: the provider's variable, the pipeline's argument and the large-symbol page maker."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr


def _service(monkeypatch, **env):
    from lumina_ocr.services import ocr_service as svc
    for k in ("LUMINA_OCR_QRCODES", "LUMINA_OCR_QR_MAX_VERSION"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = object.__new__(svc.OCRService)           # beside the process's singleton
    s._initialized = False
    svc.OCRService.__init__(s)
    return s


def test_the_provider_reads_the_largest_version_from_the_environment(monkeypatch):
    s = _service(monkeypatch)
    assert s._use_qrcodes is False and s.get_status()["qr_max_version"] is None
    assert _service(monkeypatch, LUMINA_OCR_QR_MAX_VERSION="40").get_status()["qr_max_version"] is None      # ignored without the QR option
    assert _service(monkeypatch, LUMINA_OCR_QRCODES="1").get_status()["qr_max_version"] == 10
    assert _service(monkeypatch, LUMINA_OCR_QRCODES="1", LUMINA_OCR_QR_MAX_VERSION="40").get_status()["qr_max_version"] == 40
    for bad in ("9", "41", "forty", "-3"):
        s = _service(monkeypatch, LUMINA_OCR_QRCODES="1", LUMINA_OCR_QR_MAX_VERSION=bad)
        assert s.get_status()["qr_max_version"] == bad
        s._allow_synthetic = True
        with pytest.raises(RuntimeError, match="LUMINA_OCR_QR_MAX_VERSION"):
            s._ensure_engine()
        r = s.process_image_sync(Image.fromarray(np.full((40, 60, 3), 255, np.uint8)))
        assert not r.success and "LUMINA_OCR_QR_MAX_VERSION" in r.error


def test_the_pipeline_checks_its_argument():
    from lumina_ocr.pipeline import OcrPipeline
    for bad in (9, 41):
        with pytest.raises(ValueError, match="qr_max_version"):
            OcrPipeline(None, charset=["", "a"], qrcodes=True, qr_max_version=bad)


def test_large_symbol_pages_are_seeded():
    a, ga = synth.synth_qr_large_page(7)
    b, gb = synth.synth_qr_large_page(7)
    assert np.array_equal(a, b) and ga == gb and len(ga) == 1 and 11 <= ga[0]["version"] <= 40
    assert {synth.synth_qr_large_page(s)[1][0]["version"] for s in range(12)} != {ga[0]["version"]}
    g = ga[0]
    x0, y0, x1, y1 = g["box"]
    assert x1 - x0 + 1 == qr.dimension(g["version"]) * g["module"] and a[y0:y1 + 1, x0:x1 + 1].min() == 0
