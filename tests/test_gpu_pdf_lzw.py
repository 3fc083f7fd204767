"""GPU: scanned PDFs whose page images are /LZWDecode or /RunLengthDecode streams, through the provider with LUMINA_OCR_PDF_SCANS and
LUMINA_OCR_DEVICE_TIFF: lumina_ocr_strip_image_decode takes them as one-strip pages, so each page must give exactly what the same rows
embedded as /FlateDecode give; /EarlyChange 0 and, without LUMINA_OCR_DEVICE_TIFF, both filters go to the rasteriser with their reason."""
import zlib

import numpy as np
import pytest
from PIL import Image

import pdf_cases as pc
import tiff_cases as tc
import tiff_reference as tr
from lumina_ocr import synth

pytestmark = pytest.mark.gpu

W, H = 700, 1000


@pytest.fixture
def service(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_pdf, s.device_tiff

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):   # as on a machine without pdf2image / poppler
        raise ImportError("pdf2image not installed. Install with: pip install pdf2image (and poppler)")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    s.device_pdf = s.device_tiff = True
    yield s
    s.device_pdf, s.device_tiff = saved
    s.cleanup()


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=12)[0] for seed in (41, 42, 43)]


def _lzw(rows: np.ndarray, comps: int, predictor: int) -> bytes:
    """the rows as one libtiff LZW strip (the coding of PDF's /LZWDecode with /EarlyChange 1)"""
    im = Image.fromarray(rows.reshape(H, W, 3) if comps == 3 else rows)
    _, strips, _ = tc.libtiff_strips(im, "tiff_lzw", {278: H, 317: predictor})
    assert len(strips) == 1
    return strips[0]


def _bodies(pages):
    """[(the page as an LZW / RunLength image, the same rows as a Flate image)]"""
    rgb = pages[0].reshape(H, W * 3)
    grey = np.asarray(Image.fromarray(pages[1]).convert("L"))
    bits = pc.pack_bits((pages[2].mean(axis=2) >= 128).astype(np.uint8), 1)
    p2 = "<< /Predictor 2 /Colors 3 /BitsPerComponent 8 /Columns %d >>" % W
    return [
        (pc.image_obj(W, H, "/LZWDecode", _lzw(rgb, 3, 2), cs="/DeviceRGB", parms=p2),
         pc.image_obj(W, H, "/FlateDecode", zlib.compress(pc.tiff_predict_rows(rgb, 3), 1), cs="/DeviceRGB", parms=p2)),
        (pc.image_obj(W, H, "/LZWDecode", _lzw(grey, 1, 1), parms="<< /EarlyChange 1 >>"),
         pc.image_obj(W, H, "/FlateDecode", zlib.compress(grey.tobytes(), 1))),
        (pc.image_obj(W, H, "/RunLengthDecode", tr.packbits_encode(bits.tobytes(), eod=True), bits=1, extra="/Decode [1 0]"),
         pc.image_obj(W, H, "/FlateDecode", zlib.compress(bits.tobytes(), 1), bits=1, extra="/Decode [1 0]")),
    ]


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height, r.page_width_inches, r.page_height_inches, r.page_number)


def _doc(s, tmp_path, name, bodies):
    pdf = tmp_path / name
    pdf.write_bytes(pc.document([{"image": b, "box": (504, 720)} for b in bodies]))
    return s.process_pdf_sync(pdf)


def test_one_page_lzw_equals_flate(service, tmp_path, pages):
    new, old = _bodies(pages)[0]
    got, want = _doc(service, tmp_path, "lzw.pdf", [new]), _doc(service, tmp_path, "flate.pdf", [old])
    assert got.success and want.success and want.pages[0].layout_boxes, (got.error, got.pages and got.pages[0].error)
    assert _key(got.pages[0]) == _key(want.pages[0])


def test_three_pages_of_lzw_and_run_length_equal_flate(service, tmp_path, pages):
    b = _bodies(pages)
    got, want = _doc(service, tmp_path, "new.pdf", [x[0] for x in b]), _doc(service, tmp_path, "old.pdf", [x[1] for x in b])
    assert got.success and want.success and got.total_pages == 3, [p.error for p in got.pages]
    for g, w in zip(got.pages, want.pages):
        assert w.layout_boxes and _key(g) == _key(w)


def test_early_change_0_and_option_off_go_to_the_rasteriser(service, tmp_path, pages):
    s = service
    grey = np.asarray(Image.fromarray(pages[1]).convert("L"))
    body = pc.image_obj(W, H, "/LZWDecode", _lzw(grey, 1, 1), parms="<< /EarlyChange 0 >>")
    doc = _doc(s, tmp_path, "early0.pdf", [body])
    assert not doc.success and "EarlyChange 0" in doc.pages[0].error and "pdf2image" in doc.pages[0].error
    body = pc.image_obj(W, H, "/LZWDecode", _lzw(grey, 1, 1), parms="<< /Predictor 12 /Columns %d >>" % W)
    assert "LZW /Predictor 12" in _doc(s, tmp_path, "png_predictor.pdf", [body]).pages[0].error
    s.device_tiff = False
    doc = _doc(s, tmp_path, "off.pdf", [_bodies(pages)[1][0]])
    assert not doc.success and "image filter LZWDecode" in doc.pages[0].error
