"""GPU: a large Data Matrix symbol through the provider.  With LUMINA_OCR_DATAMATRIX=1 and LUMINA_OCR_DATAMATRIX_MAX_SIZE=144 a 120 x 120
symbol on a text page is a barcode entry with its content and its Markdown line, and the detector's lines inside it are dropped; with
the default (52) the provider does not see it and the result is the one without the variable; a value that is no number 52..144 is
an error result that names the variable; without LUMINA_OCR_DATAMATRIX the variable is ignored."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import layout

import dm_sizes_pages as LP

pytestmark = pytest.mark.gpu

H, W = 620, 900
SIZE = LP.size_of(120)
TEXT = LP.payload(SIZE, "2D-Doc ")


@pytest.fixture(scope="module")
def form():
    page = np.full((H, W, 3), 255, np.uint8)
    page[:200] = synth.synth_page(200, W, 11, n_lines=4, noise=0.0)[0]
    return page, synth.draw_dm(page, 60, 230, synth.dm_encode(TEXT, SIZE), 3, 1)


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_datamatrix, s._dm_max_size, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_datamatrix, s._dm_max_size, s.apply_deskew = saved


def _run(s, image, on: bool, max_size: str):
    s.cleanup()
    s._use_datamatrix, s._dm_max_size = on, max_size
    return s.process_image_sync(image)


def test_the_environment_variable_is_read(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    """on an object of its own: the shared provider is not touched"""
    for value, want in (("104", "104"), ("", "52"), (None, "52")):
        if value is None:
            monkeypatch.delenv("LUMINA_OCR_DATAMATRIX_MAX_SIZE", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_DATAMATRIX_MAX_SIZE", value)
        s = object.__new__(svc.OCRService)
        s.__init__()
        assert s._dm_max_size == want and s._engine is None


def test_large_symbol_through_the_provider(service, form):
    page, b = form
    image = Image.fromarray(page)
    r = _run(service, image, True, "144")
    assert r.success, r.error
    assert service.get_status()["datamatrix"] is True and service.get_status()["datamatrix_max_size"] == 144
    got = [x for x in r.layout_boxes if x["type"] == "barcode"]
    assert [(g["kind"], g["content"], g["polygon"]) for g in got] == [("DataMatrix", TEXT, [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)])]
    assert got[0]["confidence"] == 1.0 and r.json_output["datamatrix_count"] == 1 and layout.validate_layout_boxes(r.layout_boxes) == []
    assert ":barcode: %s" % TEXT in r.markdown.split("\n") and r.markdown.count(":barcode:") == 1
    inside = lambda x: b[0] <= sum(x["polygon"][0::2]) / 4.0 <= b[2] + 1 and b[1] <= sum(x["polygon"][1::2]) / 4.0 <= b[3] + 1
    assert not [x for x in r.layout_boxes if x["type"] in ("word", "line") and inside(x)]
    # ---- the default is the provider as it was: the symbol is not seen, and leaving the variable out gives the same result ----
    default = _run(service, image, True, "52")
    assert default.success and default.json_output["datamatrix_count"] == 0 and service.get_status()["datamatrix_max_size"] == 52
    assert not [x for x in default.layout_boxes if x["type"] == "barcode"]
    # ---- a bad value is an error result that names the variable; without the Data Matrix pass the variable is ignored ----
    for text in ("160", "51", "big"):
        bad = _run(service, image, True, text)
        assert not bad.success and "LUMINA_OCR_DATAMATRIX_MAX_SIZE" in (bad.error or "") and service.get_status()["datamatrix_max_size"] == text
    off = _run(service, image, False, "160")
    assert off.success and "datamatrix_count" not in off.json_output and service.get_status()["datamatrix_max_size"] is None
    plain = _run(service, image, False, "52")
    assert off.markdown == plain.markdown and off.layout_boxes == plain.layout_boxes
