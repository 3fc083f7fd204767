"""GPU: a large Aztec symbol through the provider.  With LUMINA_OCR_AZTEC=1 and LUMINA_OCR_AZTEC_MAX_LAYERS=32 a 16-layer symbol on a
text page is a barcode entry with its content and its Markdown line; with the default (11) the provider does not see it; a value
that is no number of layers 11..32 is an error result that names the variable; without LUMINA_OCR_AZTEC the variable is ignored."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import aztec as az
from lumina_ocr.utils import layout

pytestmark = pytest.mark.gpu

H, W = 620, 900
TEXT = "Fahrschein 2024-10-19 Basel SBB - Wien Hbf, 2. Klasse, 1 Erwachsener. " * 6


@pytest.fixture(scope="module")
def form():
    page = np.full((H, W, 3), 255, np.uint8)
    page[:200] = synth.synth_page(200, W, 11, n_lines=4, noise=0.0)[0]
    return page, az.draw(page, 60, 240, az.encode(TEXT, False, 16), 4, 1)


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_aztec, s._aztec_max_layers, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_aztec, s._aztec_max_layers, s.apply_deskew = saved


def _run(s, image, aztec: bool, max_layers: str):
    s.cleanup()
    s._use_aztec, s._aztec_max_layers = aztec, max_layers
    return s.process_image_sync(image)


def test_the_environment_variable_is_read(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    """on an object of its own: the shared provider is not touched"""
    for value, want in (("27", "27"), ("", "11"), (None, "11")):
        if value is None:
            monkeypatch.delenv("LUMINA_OCR_AZTEC_MAX_LAYERS", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_AZTEC_MAX_LAYERS", value)
        s = object.__new__(svc.OCRService)
        s.__init__()
        assert s._aztec_max_layers == want and s._engine is None


def test_large_symbol_through_the_provider(service, form):
    page, b = form
    image = Image.fromarray(page)
    r = _run(service, image, True, "32")
    assert r.success, r.error
    assert service.get_status()["aztec"] is True and service.get_status()["aztec_max_layers"] == 32
    got = [x for x in r.layout_boxes if x["type"] == "barcode"]
    assert [(g["kind"], g["content"], g["polygon"]) for g in got] == [("Aztec", TEXT, [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)])]
    assert got[0]["confidence"] == 1.0 and r.json_output["aztec_count"] == 1 and layout.validate_layout_boxes(r.layout_boxes) == []
    assert ":barcode: %s" % TEXT in r.markdown.split("\n") and r.markdown.count(":barcode:") == 1
    inside = lambda x: b[0] <= sum(x["polygon"][0::2]) / 4.0 <= b[2] + 1 and b[1] <= sum(x["polygon"][1::2]) / 4.0 <= b[3] + 1
    assert not [x for x in r.layout_boxes if x["type"] in ("word", "line") and inside(x)]
    # ---- the default is the provider as it was: the symbol is not seen ----
    default = _run(service, image, True, "11")
    assert default.success and default.json_output["aztec_count"] == 0 and service.get_status()["aztec_max_layers"] == 11
    assert not [x for x in default.layout_boxes if x["type"] == "barcode"]
    # ---- a bad value is an error result that names the variable; without the Aztec pass the variable is ignored ----
    bad = _run(service, image, True, "40")
    assert not bad.success and "LUMINA_OCR_AZTEC_MAX_LAYERS" in (bad.error or "") and service.get_status()["aztec_max_layers"] == "40"
    off = _run(service, image, False, "40")
    assert off.success and "aztec_count" not in off.json_output and service.get_status()["aztec_max_layers"] is None
