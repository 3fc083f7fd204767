"""GPU: scanned PDFs through the provider with LUMINA_OCR_PDF_SCANS (OCRService.device_pdf).  The pages' embedded images are decoded on
the device, so a lossless page must give exactly what process_pages_sync gives for its source image, and a DCT page what
process_image_sync gives for the embedded JPEG; refused pages become per-page results; with the option off nothing changes."""
import asyncio
import importlib.util
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import ccitt_cases as cc
import pdf_cases as pc
from lumina_ocr import synth

pytestmark = pytest.mark.gpu

W, H = 700, 1000


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_pdf
    yield s
    s.device_pdf = saved
    s.cleanup()


def _no_rasteriser(s, monkeypatch):
    """pdf_to_images as it is on a machine without pdf2image / poppler"""
    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed. Install with: pip install pdf2image (and poppler)")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=12)[0] for seed in (21, 22, 23)]


def _flate_rgb(page) -> bytes:
    return pc.image_obj(W, H, "/FlateDecode", zlib.compress(pc.png_filter_rows(page.reshape(H, -1), 3, [1, 2, 4]), 6), cs="/DeviceRGB",
                        parms="<< /Predictor 15 /Colors 3 /BitsPerComponent 8 /Columns %d >>" % W)


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height, r.page_width_inches, r.page_height_inches)


def test_three_filters_equal_the_image_paths(service, monkeypatch, tmp_path, pages):
    s = service
    _no_rasteriser(s, monkeypatch)
    black = pages[0].mean(axis=2) < 128
    bilevel = np.repeat(np.where(black, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)
    jpeg = pc.jpeg_bytes(pages[2])
    doc_pages = [
        {"image": pc.image_obj(W, H, "/CCITTFaxDecode", cc.g4_encode(black), bits=1, parms="<< /K -1 /Columns %d /Rows %d >>" % (W, H)), "box": (504, 720)},
        {"image": _flate_rgb(pages[1]), "box": (504, 720)},
        {"image": pc.image_obj(W, H, "/DCTDecode", jpeg, cs="/DeviceRGB"), "box": (504, 720)},
    ]
    pdf = tmp_path / "scan.pdf"
    pdf.write_bytes(pc.document(doc_pages, xref="stream", objstm=True))
    s.device_pdf = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success and doc.total_pages == 3 and [p.page_number for p in doc.pages] == [1, 2, 3], doc.error
    assert s.get_status()["device_pdf"] is True
    lossless = s.process_pages_sync([Image.fromarray(bilevel), Image.fromarray(pages[1])])
    dct = s.process_image_sync(jpeg, page_number=3)
    for got, want in zip(doc.pages, lossless + [dct]):
        assert want.success and want.layout_boxes
        assert _key(got) == _key(want)
    assert doc.combined_layout_boxes == [b for p in doc.pages for b in p.layout_boxes]
    assert all(p.markdown in doc.combined_markdown for p in doc.pages)


def test_rotate_90_equals_the_turned_image(service, monkeypatch, tmp_path, pages):
    s = service
    _no_rasteriser(s, monkeypatch)
    sideways = np.ascontiguousarray(np.rot90(pages[1], 1))   # the scan lies on its left side: /Rotate 90 turns it upright
    h, w = sideways.shape[:2]
    body = pc.image_obj(w, h, "/FlateDecode", zlib.compress(sideways.tobytes(), 1), cs="/DeviceRGB")
    pdf = tmp_path / "rotated.pdf"
    pdf.write_bytes(pc.document([{"image": body, "box": (w, h), "media": False}], tree_attrs="/Rotate 90 /MediaBox [0 0 %d %d]" % (w, h)))
    s.device_pdf = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success, doc.error
    turned = Image.fromarray(sideways).transpose(Image.ROTATE_270)
    assert np.array_equal(np.asarray(turned), pages[1])
    want = s.process_pages_sync([turned])[0]
    assert want.layout_boxes and _key(doc.pages[0]) == _key(want)


def test_text_page_is_a_per_page_error(service, monkeypatch, tmp_path, pages):
    s = service
    _no_rasteriser(s, monkeypatch)
    img = _flate_rgb(pages[1])
    pdf = tmp_path / "mixed.pdf"
    pdf.write_bytes(pc.document([{"image": img, "box": (504, 720)},
                                 {"image": img, "box": (504, 720), "content": b"BT /F1 12 Tf 72 700 Td (born digital) Tj ET"},
                                 {"image": img, "box": (504, 720)}]))
    s.device_pdf = True
    doc = s.process_pdf_sync(pdf)
    assert not doc.success and doc.error == "Some pages failed" and doc.total_pages == 3
    assert [p.success for p in doc.pages] == [True, False, True] and [p.page_number for p in doc.pages] == [1, 2, 3]
    assert "text operators" in doc.pages[1].error and "pdf2image" in doc.pages[1].error
    assert doc.pages[0].layout_boxes and doc.pages[0].markdown == doc.pages[2].markdown


def test_progressive_jpeg_page_is_decoded_by_pillow(service, monkeypatch, tmp_path, pages):
    """the device JPEG decoder refuses a progressive file; the page takes the fallback JPEG files have and still needs no rasteriser"""
    s = service
    _no_rasteriser(s, monkeypatch)
    op = io.BytesIO()
    Image.fromarray(pages[2]).save(op, "JPEG", quality=90, progressive=True)
    pdf = tmp_path / "progressive.pdf"
    pdf.write_bytes(pc.document([{"image": pc.image_obj(W, H, "/DCTDecode", op.getvalue(), cs="/DeviceRGB"), "box": (504, 720)}]))
    s.device_pdf = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success, doc.error
    want = s.process_image_sync(op.getvalue())
    assert want.layout_boxes and _key(doc.pages[0]) == _key(want)


def test_option_off_is_the_rasteriser_path(service, monkeypatch, tmp_path, pages):
    s = service
    if importlib.util.find_spec("pdf2image") is not None:
        _no_rasteriser(s, monkeypatch)
    pdf = tmp_path / "scan.pdf"
    pdf.write_bytes(pc.document([{"image": _flate_rgb(pages[1]), "box": (504, 720)}]))
    s.device_pdf = False
    doc = s.process_pdf_sync(pdf)
    assert not doc.success and doc.pages == [] and doc.error.startswith("pdf2image not installed")
    assert s.get_status()["device_pdf"] is False


def test_pillow_written_pdf_through_process_document(service, monkeypatch, tmp_path, pages):
    s = service
    _no_rasteriser(s, monkeypatch)
    bilevel = Image.fromarray(np.where(pages[0].mean(axis=2) < 128, 0, 255).astype(np.uint8)).convert("1")
    pdf = tmp_path / "pillow.pdf"
    Image.fromarray(pages[2]).save(pdf, "PDF", save_all=True, append_images=[bilevel], resolution=200.0)
    s.device_pdf = True
    doc = asyncio.run(s.process_document(pdf, "pdf"))
    assert doc.success and doc.total_pages == 2, doc.error
    assert all(p.layout_boxes and p.markdown.strip() for p in doc.pages)
    assert _key(doc.pages[1]) == _key(s.process_pages_sync([bilevel.convert("RGB")], first_page_number=2)[0])
