"""GPU: a large QR symbol through the provider.  With LUMINA_OCR_QRCODES=1 and LUMINA_OCR_QR_MAX_VERSION=40 a 25-M symbol on a text page
is one `barcode` entry with its content and the lines inside it are gone; without the variable the page's result is what it is
today: the QR option finds three finders and reports nothing."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import layout

import qr_version_cases as C

pytestmark = pytest.mark.gpu

H, W = 700, 1000


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_qrcodes, s._qr_max_version, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_qrcodes, s._qr_max_version, s.apply_deskew = saved


def _run(s, image, qrcodes: bool, max_version: str = "10"):
    s.cleanup()
    s._use_qrcodes, s._qr_max_version = qrcodes, max_version
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_a_large_symbol_on_a_text_page(service):
    page = np.full((H, W, 3), 255, np.uint8)
    page[:240] = synth.synth_page(240, W, 11, n_lines=5, noise=0.0)[0]
    box, text = C.put(page, 60, 300, 25, 1)
    image = Image.fromarray(page)
    on = _run(service, image, True, "40")
    assert on.success, on.error
    assert service.get_status()["qrcodes"] is True and service.get_status()["qr_max_version"] == 40
    got = [b for b in on.layout_boxes if b["type"] == "barcode"]
    rect = [float(v) for v in (box[0], box[1], box[2] + 1, box[1], box[2] + 1, box[3] + 1, box[0], box[3] + 1)]
    assert [(b["kind"], b["content"], b["polygon"], b["confidence"]) for b in got] == [("QRCode", text, rect, 1.0)]
    assert on.json_output["qrcodes_count"] == 1 and layout.validate_layout_boxes(on.layout_boxes) == []
    assert not [b for b in on.layout_boxes if b["type"] in ("word", "line") and _centre_in(b["polygon"], box)]
    assert ":barcode: %s" % text in on.markdown.split("\n") and on.markdown.count(":barcode:") == 1
    # ---- without the variable: today's result, which has no symbol; at 10 spelled out the same ----
    today = _run(service, image, True)
    assert today.success and service.get_status()["qr_max_version"] == 10
    assert today.json_output["qrcodes_count"] == 0 and not [b for b in today.layout_boxes if b["type"] == "barcode"]
    off = _run(service, image, False, "40")                                          # the variable alone does nothing
    assert off.success and service.get_status()["qr_max_version"] is None
    assert today.layout_boxes == off.layout_boxes and today.markdown == off.markdown and today.json_output == dict(off.json_output, qrcodes_count=0)
    outside = lambda res: [b for b in res.layout_boxes if b["type"] in ("word", "line") and not _centre_in(b["polygon"], box)]
    assert outside(on) == outside(today) and on.processed_image_bytes == today.processed_image_bytes


def test_small_symbols_are_reported_as_before(service):
    page, gt = synth.synth_qr_page(5, h=460, w=620, n_codes=2, text_lines=3, module_px=4)
    image = Image.fromarray(page)
    small, large = _run(service, image, True), _run(service, image, True, "40")
    assert small.success and large.success and small.json_output["qrcodes_count"] == 2
    assert small.layout_boxes == large.layout_boxes and small.markdown == large.markdown and small.json_output == large.json_output
