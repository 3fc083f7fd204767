"""GPU: EAN-13 and ITF-14 through the provider (LUMINA_OCR_BARCODES=1 LUMINA_OCR_BARCODE_KINDS=all) on a small synthetic invoice: the
two entries and their Markdown lines, the text lines untouched; with the default kinds the provider is the one it was."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import layout

import linear_pages as lp

pytestmark = pytest.mark.gpu

H, W = 420, 640


@pytest.fixture(scope="module")
def invoice():
    page = lp.blank(H, W)
    page[:200] = synth.synth_page(200, W, 11, n_lines=5, noise=0.0)[0]
    want = {}
    lp.put(page, want, 40, 250, "EAN13", lp.EAN13_A, m=2, height=50)
    lp.put(page, want, 300, 330, "ITF", lp.ITF14, m=2, height=40, ratio=2.5)
    return page, want


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_barcodes, s._barcode_kinds, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_barcodes, s._barcode_kinds, s.apply_deskew = saved


def _run(s, image, barcodes: bool, kinds: str = "code128,code39"):
    s.cleanup()
    s._use_barcodes, s._barcode_kinds = barcodes, kinds
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_invoice_through_the_provider(service, invoice):
    page, want = invoice
    image = Image.fromarray(page)
    off = _run(service, image, False)
    assert off.success, off.error
    r = _run(service, image, True, "all")
    assert r.success, r.error
    assert service.get_status()["barcode_kinds"] == ["code128", "code39", "ean13", "ean8", "upce", "itf"]
    got = [b for b in r.layout_boxes if b["type"] == "barcode"]
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)]
    assert [(b["kind"], b["content"], b["polygon"], b.get("itf14", False)) for b in got] == [
        (k, c, rect(box), bool(f & 4)) for box, (k, c, f) in sorted(want.items(), key=lambda t: t[0][1])]
    assert [b["kind"] for b in got] == ["EAN13", "ITF"] and got[1]["itf14"] is True
    assert all(b["confidence"] == 1.0 for b in got) and r.json_output["barcodes_count"] == 2
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    rows = r.markdown.split("\n")
    assert ":barcode: %s" % lp.EAN13_A in rows and ":barcode: %s" % lp.ITF14 in rows and r.markdown.count(":barcode:") == 2
    # the text lines that were there without barcodes are still there; what the detector made of the bars is gone
    outside = lambda res: [b for b in res.layout_boxes if b["type"] in ("word", "line") and not any(_centre_in(b["polygon"], box) for box in want)]
    assert outside(r) == outside(off) and len([b for b in outside(off) if b["type"] == "line"]) >= 3
    assert not [b for b in r.layout_boxes if b["type"] in ("word", "line") and any(_centre_in(b["polygon"], box) for box in want)]
    assert r.processed_image_bytes == off.processed_image_bytes
    # the default kinds: no new entries, every line as with barcodes off
    plain = _run(service, image, True)
    assert plain.success and service.get_status()["barcode_kinds"] == ["code128", "code39"]
    assert plain.json_output["barcodes_count"] == 0 and not [b for b in plain.layout_boxes if b["type"] == "barcode"]
    assert plain.layout_boxes == off.layout_boxes and plain.markdown == off.markdown
    # an unknown name is an error result
    bad = _run(service, image, True, "ean13,codabar")
    assert not bad.success and "LUMINA_OCR_BARCODE_KINDS" in bad.error
