"""GPU: QR codes through the provider (LUMINA_OCR_QRCODES=1) on one synthetic form: the entries carry what was rendered, nothing the
recogniser made of the modules is left, the option off is a provider that never heard of QR codes, with LUMINA_OCR_BARCODES on as
well the 1-D codes come first, and a page without a symbol is the same page with the option on."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import layout

pytestmark = pytest.mark.gpu

H, W = 700, 1000


@pytest.fixture(scope="module")
def form():
    """text lines above; a 3-M symbol, a 5-Q one turned by 90 degrees and a Code 128 strip below"""
    page = np.full((H, W, 3), 255, np.uint8)
    page[:240] = synth.synth_page(240, W, 11, n_lines=5, noise=0.0)[0]
    gt = []
    for x, y, text, version, level, mask, m, rot in ((60, 300, "https://lumina.example/inv/0042", 3, 1, 2, 5, 0), (400, 290, "LOT 7 / ÄÖ 2024-10", 5, 2, 6, 4, 1)):
        gt.append(dict(text=text, box=synth.draw_qr(page, x, y, synth.qr_encode(text, version, level, mask), m, rot)))
    strip = synth.render_barcode(page, 700, 620, synth.code128_symbols("STRIP-1"), "Code128", 2, 50)
    return page, gt, strip


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s.apply_deskew = saved


def _run(s, image, qrcodes: bool, barcodes: bool = False):
    s.cleanup()
    s._use_qrcodes, s._use_barcodes = qrcodes, barcodes
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_form_through_the_provider(service, form):
    page, gt, strip = form
    image = Image.fromarray(page)
    r = _run(service, image, True)
    assert r.success, r.error
    assert service.get_status()["qrcodes"] is True and service.get_status()["barcodes"] is False
    got = [b for b in r.layout_boxes if b["type"] == "barcode"]
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)]
    assert sorted((b["kind"], b["content"], b["polygon"]) for b in got) == sorted(("QRCode", g["text"], rect(g["box"])) for g in gt)
    assert all(b["confidence"] == 1.0 for b in got) and r.json_output["qrcodes_count"] == len(gt) == 2 and "barcodes_count" not in r.json_output
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [b["type"] for b in r.layout_boxes]
    assert types == sorted(types, key=["word", "line", "selection_mark", "barcode", "table", "table_cell", "paragraph"].index)
    assert not [b for b in r.layout_boxes if b["type"] in ("word", "line") and any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    rows = r.markdown.split("\n")
    assert all(":barcode: %s" % g["text"] in rows for g in gt) and r.markdown.count(":barcode:") == 2
    # ---- the switch: off is a provider that never heard of QR codes ----
    off = _run(service, image, False)
    assert off.success and "qrcodes_count" not in off.json_output and service.get_status()["qrcodes"] is False
    assert not [b for b in off.layout_boxes if b["type"] == "barcode"] and ":barcode:" not in off.markdown
    outside = lambda res: [b for b in res.layout_boxes if b["type"] in ("word", "line") and not any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    assert outside(off) == outside(r)
    assert r.processed_image_bytes == off.processed_image_bytes
    # ---- with the 1-D codes on as well: the strip first, then the symbols ----
    both = _run(service, image, True, barcodes=True)
    kinds = [(b["kind"], b["content"]) for b in both.layout_boxes if b["type"] == "barcode"]
    assert kinds[0] == ("Code128", "STRIP-1") and sorted(kinds[1:]) == sorted(("QRCode", g["text"]) for g in gt)
    assert both.json_output["barcodes_count"] == 1 and both.json_output["qrcodes_count"] == 2
    only = _run(service, image, False, barcodes=True)
    assert [b for b in only.layout_boxes if b["type"] == "barcode" and b["kind"] != "QRCode"] == [b for b in both.layout_boxes if b["type"] == "barcode"][:1]


def test_a_page_without_a_symbol_is_unchanged_by_the_option(service):
    page = synth.synth_page(500, 800, 21, n_lines=10, noise=0.0)[0]
    image = Image.fromarray(page)
    on, off = _run(service, image, True), _run(service, image, False)
    assert on.success and off.success
    assert on.layout_boxes == off.layout_boxes and on.markdown == off.markdown
    assert on.json_output == dict(off.json_output, qrcodes_count=0)
