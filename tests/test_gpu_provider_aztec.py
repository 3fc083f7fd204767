"""GPU: Aztec symbols through the provider (LUMINA_OCR_AZTEC=1) on one synthetic form with text, an Aztec, a QR and a Data Matrix symbol:
with every option on each symbol is reported once with its content, in the order 1-D, QR, Data Matrix, Aztec; nothing the recogniser
made of the modules is left; the reading order is stable; the option off is a provider that never heard of Aztec; and a page without
a symbol is the same page with the option on."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.utils import aztec as az
from lumina_ocr.utils import layout

pytestmark = pytest.mark.gpu

H, W = 600, 900
TEXT = "Ticket 4711, Basel - Wien. 2nd class"


@pytest.fixture(scope="module")
def form():
    page = np.full((H, W, 3), 255, np.uint8)
    page[:240] = synth.synth_page(240, W, 11, n_lines=5, noise=0.0)[0]
    aztec = dict(text=TEXT, box=az.draw(page, 60, 300, az.encode(TEXT, False, 3), 5, 1))
    qr = dict(text="QR NEXT TO IT", box=synth.draw_qr(page, 300, 300, synth.qr_encode("QR NEXT TO IT", 2, 1, 2), 5))
    dm = dict(text="DM-0042", box=synth.draw_dm(page, 520, 300, synth.dm_encode("DM-0042", 4), 5))
    return page, aztec, qr, dm


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s._use_datamatrix, s._use_aztec, s.apply_deskew)
    s._allow_synthetic, s.apply_deskew = True, False
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_barcodes, s._use_qrcodes, s._use_datamatrix, s._use_aztec, s.apply_deskew = saved


def _run(s, image, aztec: bool, others: bool = False):
    s.cleanup()
    s._use_aztec, s._use_barcodes, s._use_qrcodes, s._use_datamatrix = aztec, others, others, others
    return s.process_image_sync(image)


def _centre_in(poly, box):
    cx, cy = sum(poly[0::2]) / 4.0, sum(poly[1::2]) / 4.0
    return box[0] <= cx <= box[2] + 1 and box[1] <= cy <= box[3] + 1


def test_form_through_the_provider(service, form):
    page, aztec, qr, dm = form
    image = Image.fromarray(page)
    r = _run(service, image, True)
    assert r.success, r.error
    assert service.get_status()["aztec"] is True and service.get_status()["datamatrix"] is False
    got = [b for b in r.layout_boxes if b["type"] == "barcode"]
    b = aztec["box"]
    assert [(g["kind"], g["content"], g["polygon"]) for g in got] == [("Aztec", TEXT, [float(v) for v in (b[0], b[1], b[2] + 1, b[1], b[2] + 1, b[3] + 1, b[0], b[3] + 1)])]
    assert got[0]["confidence"] == 1.0 and r.json_output["aztec_count"] == 1 and "datamatrix_count" not in r.json_output
    assert layout.validate_layout_boxes(r.layout_boxes) == []
    types = [x["type"] for x in r.layout_boxes]
    assert types == sorted(types, key=["word", "line", "selection_mark", "barcode", "table", "table_cell", "paragraph"].index)
    assert not [x for x in r.layout_boxes if x["type"] in ("word", "line") and _centre_in(x["polygon"], b)]
    assert ":barcode: %s" % TEXT in r.markdown.split("\n") and r.markdown.count(":barcode:") == 1
    # ---- the switch: off is a provider that never heard of Aztec ----
    off = _run(service, image, False)
    assert off.success and "aztec_count" not in off.json_output and service.get_status()["aztec"] is False
    assert not [x for x in off.layout_boxes if x["type"] == "barcode"] and ":barcode:" not in off.markdown
    outside = lambda res: [x for x in res.layout_boxes if x["type"] in ("word", "line") and not _centre_in(x["polygon"], b)]
    assert outside(off) == outside(r)
    assert r.processed_image_bytes == off.processed_image_bytes
    # ---- every option on: QR, Data Matrix, Aztec, every symbol once; the lines inside all three are dropped; twice the same ----
    every = _run(service, image, True, others=True)
    kinds = [(x["kind"], x["content"]) for x in every.layout_boxes if x["type"] == "barcode"]
    assert kinds == [("QRCode", qr["text"]), ("DataMatrix", dm["text"]), ("Aztec", TEXT)]
    assert every.json_output["qrcodes_count"] == 1 and every.json_output["datamatrix_count"] == 1 and every.json_output["aztec_count"] == 1
    assert every.json_output["barcodes_count"] == 0 and every.markdown.count(":barcode:") == 3
    assert not [x for x in every.layout_boxes if x["type"] in ("word", "line") and any(_centre_in(x["polygon"], g["box"]) for g in (aztec, qr, dm))]
    again = _run(service, image, True, others=True)
    assert again.layout_boxes == every.layout_boxes and again.markdown == every.markdown
    others = _run(service, image, False, others=True)
    assert [x for x in others.layout_boxes if x["type"] == "barcode"] == [x for x in every.layout_boxes if x["type"] == "barcode"][:2]


def test_a_page_without_a_symbol_is_unchanged_by_the_option(service):
    page = synth.synth_page(500, 800, 21, n_lines=10, noise=0.0)[0]
    image = Image.fromarray(page)
    on, off = _run(service, image, True), _run(service, image, False)
    assert on.success and off.success
    assert on.layout_boxes == off.layout_boxes and on.markdown == off.markdown
    assert on.json_output == dict(off.json_output, aztec_count=0)
