"""GPU: layered scanned PDFs through the provider with LUMINA_OCR_PDF_SCANS and LUMINA_OCR_PDF_LAYERS (OCRService.pdf_layers), no
rasteriser installed.  The layers are decoded and put together on the device, so a page must give exactly what process_pages_sync gives
for the bitmap the page shows; page order and numbers hold in a mixed document; with the option off the same file gives the per-page
errors it gave before."""
import numpy as np
import pytest
from PIL import Image

import pdf_cases as pc
import pdf_layer_cases as lc

pytestmark = pytest.mark.gpu

CUTS = [1, 333, 640, 998]


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_pdf, s.pdf_layers
    yield s
    s.device_pdf, s.pdf_layers = saved
    s.cleanup()


def _no_rasteriser(s, monkeypatch):
    """pdf_to_images as it is on a machine without pdf2image / poppler"""
    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed. Install with: pip install pdf2image (and poppler)")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height, r.page_width_inches, r.page_height_inches)


@pytest.fixture(scope="module")
def material():
    """(strips page dict, its bitmap, mixed raster page dict, its bitmap)"""
    strips, strips_want = lc.strips_page(lc.source_page(), CUTS, ["rgb", "gray", "g4"])
    mixed, mixed_want = lc.mixed_raster_page(g4=True)
    return strips, strips_want, mixed, mixed_want


def test_strips_and_mixed_raster_pages_equal_their_bitmaps(service, monkeypatch, tmp_path, material):
    s = service
    _no_rasteriser(s, monkeypatch)
    strips, strips_want, mixed, mixed_want = material
    pdf = tmp_path / "layers.pdf"
    pdf.write_bytes(pc.document([strips, mixed, strips], xref="stream", objstm=True))
    s.device_pdf = s.pdf_layers = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success and doc.total_pages == 3 and [p.page_number for p in doc.pages] == [1, 2, 3], (doc.error, [p.error for p in doc.pages])
    assert s.get_status()["pdf_layers"] is True
    want = s.process_pages_sync([Image.fromarray(strips_want), Image.fromarray(mixed_want), Image.fromarray(strips_want)])
    for got, w in zip(doc.pages, want):
        assert w.success and w.layout_boxes
        assert _key(got) == _key(w)
    assert (doc.pages[0].image_width, doc.pages[0].image_height, doc.pages[1].image_width, doc.pages[1].image_height) == (700, 1000, 699, 1002)


def test_a_mixed_document_keeps_page_order_and_numbers(service, monkeypatch, tmp_path, material):
    s = service
    _no_rasteriser(s, monkeypatch)
    strips, strips_want, mixed, mixed_want = material
    page = lc.source_page(41)
    one = {"image": lc.rgb_obj(page), "box": lc.BOX}
    text = {"image": lc.rgb_obj(page), "box": lc.BOX, "content": pc.page_content(*lc.BOX) + b"\nBT /F1 12 Tf 72 300 Td (born digital) Tj ET"}
    searchable = {"image": lc.rgb_obj(page), "box": lc.BOX, "content": pc.page_content(*lc.BOX) + b"\nBT /F1 12 Tf 3 Tr 72 300 Td (ocr layer) Tj ET"}
    pdf = tmp_path / "mixed.pdf"
    pdf.write_bytes(pc.document([mixed, one, text, strips, searchable]))
    s.device_pdf = s.pdf_layers = True
    doc = s.process_pdf_sync(pdf)
    assert not doc.success and doc.error == "Some pages failed" and doc.total_pages == 5
    assert [p.success for p in doc.pages] == [True, True, False, True, True] and [p.page_number for p in doc.pages] == [1, 2, 3, 4, 5]
    assert "text operators on the page (Tj)" in doc.pages[2].error and "pdf2image" in doc.pages[2].error
    for k, bitmap in ((0, mixed_want), (1, page), (3, strips_want), (4, page)):
        w = s.process_pages_sync([Image.fromarray(bitmap)], first_page_number=k + 1)[0]
        assert w.success and w.layout_boxes and _key(doc.pages[k]) == _key(w)


def test_rotate_90_on_a_strips_page(service, monkeypatch, tmp_path):
    s = service
    _no_rasteriser(s, monkeypatch)
    sideways = np.ascontiguousarray(np.rot90(lc.source_page(42), 1))   # the scan lies on its left side: /Rotate 90 turns it upright
    h, w = sideways.shape[:2]
    d, want = lc.strips_page(sideways, [1, 250, 699], ["rgb", "gray"], box=(w, h), attrs="/Rotate 90")
    pdf = tmp_path / "rotated.pdf"
    pdf.write_bytes(pc.document([d]))
    s.device_pdf = s.pdf_layers = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success, (doc.error, [p.error for p in doc.pages])
    turned = Image.fromarray(want).transpose(Image.ROTATE_270)
    assert turned.size == (700, 1000)
    w_ = s.process_pages_sync([turned])[0]
    assert w_.layout_boxes and _key(doc.pages[0]) == _key(w_)


def test_option_off_gives_the_per_page_errors_of_before(service, monkeypatch, tmp_path, material):
    s = service
    _no_rasteriser(s, monkeypatch)
    strips, _, mixed, _ = material
    pdf = tmp_path / "layers.pdf"
    pdf.write_bytes(pc.document([strips, mixed]))
    s.device_pdf, s.pdf_layers = True, False
    doc = s.process_pdf_sync(pdf)
    assert not doc.success and [p.success for p in doc.pages] == [False, False] and [p.page_number for p in doc.pages] == [1, 2]
    assert "several images on the page" in doc.pages[0].error and "content operator 'rg'" in doc.pages[1].error
    assert all("pdf2image" in p.error for p in doc.pages)
    assert s.get_status()["pdf_layers"] is False
    s.device_pdf, s.pdf_layers = False, True   # ignored without LUMINA_OCR_PDF_SCANS: the rasteriser path, whole
    doc = s.process_pdf_sync(pdf)
    assert not doc.success and doc.pages == [] and doc.error.startswith("pdf2image not installed")
