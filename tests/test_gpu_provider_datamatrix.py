"""GPU: Data Matrix symbols through the provider (LUMINA_OCR_DATAMATRIX=1) on one synthetic form: the entries carry what was rendered,
nothing the recogniser made of the modules is left, the option off is a provider that never heard of Data Matrix, with
LUMINA_OCR_BARCODES and LUMINA_OCR_QRCODES on as well the order is 1-D, QR, Data Matrix and every symbol is reported once, and a page
without a symbol is the same page with the option on."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import layout

pytestmark = pytest.mark.gpu

H, W = 700, 1000


@pytest.fixture(scope="module")
def form():
    """text lines above; a 22 x 22 symbol, a GS1 16 x 36 one turned by 90 degrees, a QR symbol and a Code 128 strip below"""
    page = np.full((H, W, 3), 255, np.uint8)
    page[:240] = synth.synth_page(240, W, 11, n_lines=5, noise=0.0)[0]
    gt = []
    gt.append(dict(text="https://lumina.example/dm/0042", box=synth.draw_dm(page, 60, 300, synth.dm_encode("https://lumina.example/dm/0042", 7), 5)))
    gs1 = [[232], "0109501101530003", "17251231", "10AB12", [232], "21XYZ"]
    gt.append(dict(text="010950110153000317251231" "10AB12\x1d21XYZ", gs1=True, box=synth.draw_dm(page, 300, 290, synth.dm_encode(gs1, 19), 4, 1)))
    qr = dict(text="QR NEXT TO IT", box=synth.draw_qr(page, 480, 300, synth.qr_encode("QR NEXT TO IT", 2, 1, 2), 5))
    strip = synth.render_barcode(page, 700, 620, synth.code128_symbols("STRIP-1"), "Code128", 2, 50)
    return page, gt, qr, strip


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s._use_datamatrix, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s._use_datamatrix, s.apply_deskew = saved


def _run(s, image, datamatrix: bool, barcodes: bool = False, qrcodes: bool = False):
    s.cleanup()
    s._use_datamatrix, s._use_barcodes, s._use_qrcodes = datamatrix, barcodes, qrcodes
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_form_through_the_provider(service, form):
    page, gt, qr, strip = form
    image = Image.fromarray(page)
    r = _run(service, image, True)
    assert r.success, r.error
    assert service.get_status()["datamatrix"] is True and service.get_status()["qrcodes"] is False
    got = [b for b in r.layout_boxes if b["type"] == "barcode"]
    rect = lambda b: [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)]
    assert sorted((b["kind"], b["content"], b["polygon"]) for b in got) == sorted(("DataMatrix", g["text"], rect(g["box"])) for g in gt)
    assert [bool(b.get("gs1")) for b in sorted(got, key=lambda b: b["polygon"][0])] == [False, True]
    assert all(b["confidence"] == 1.0 for b in got) and r.json_output["datamatrix_count"] == len(gt) == 2 and "qrcodes_count" not in r.json_output
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [b["type"] for b in r.layout_boxes]
    assert types == sorted(types, key=["word", "line", "selection_mark", "barcode", "table", "table_cell", "paragraph"].index)
    assert not [b for b in r.layout_boxes if b["type"] in ("word", "line") and any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    rows = r.markdown.split("\n")
    assert all(":barcode: %s" % g["text"] in rows for g in gt) and r.markdown.count(":barcode:") == 2
    # ---- the switch: off is a provider that never heard of Data Matrix ----
    off = _run(service, image, False)
    assert off.success and "datamatrix_count" not in off.json_output and service.get_status()["datamatrix"] is False
    assert not [b for b in off.layout_boxes if b["type"] == "barcode"] and ":barcode:" not in off.markdown
    outside = lambda res: [b for b in res.layout_boxes if b["type"] in ("word", "line") and not any(_centre_in(b["polygon"], g["box"]) for g in gt)]
    assert outside(off) == outside(r)
    assert r.processed_image_bytes == off.processed_image_bytes
    # ---- with the 1-D codes and QR on as well: the strip, the QR symbol, the Data Matrix symbols; every symbol once ----
    every = _run(service, image, True, barcodes=True, qrcodes=True)
    kinds = [(b["kind"], b["content"]) for b in every.layout_boxes if b["type"] == "barcode"]
    assert kinds[0] == ("Code128", "STRIP-1") and kinds[1] == ("QRCode", qr["text"]) and sorted(kinds[2:]) == sorted(("DataMatrix", g["text"]) for g in gt)
    assert every.json_output["barcodes_count"] == 1 and every.json_output["qrcodes_count"] == 1 and every.json_output["datamatrix_count"] == 2
    assert every.markdown.count(":barcode:") == 4
    others = _run(service, image, False, barcodes=True, qrcodes=True)
    assert [b for b in others.layout_boxes if b["type"] == "barcode"] == [b for b in every.layout_boxes if b["type"] == "barcode"][:2]


def test_a_page_without_a_symbol_is_unchanged_by_the_option(service):
    page = synth.synth_page(500, 800, 21, n_lines=10, noise=0.0)[0]
    image = Image.fromarray(page)
    on, off = _run(service, image, True), _run(service, image, False)
    assert on.success and off.success
    assert on.layout_boxes == off.layout_boxes and on.markdown == off.markdown
    assert on.json_output == dict(off.json_output, datamatrix_count=0)
