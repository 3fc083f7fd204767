"""GPU: fax-coded scans through the provider, synthetic weights.  With LUMINA_OCR_DEVICE_TIFF the strips of Compression 2 and 3 pages
are decoded on the device (lumina_ocr_fax_decode), byte-identical to Pillow, so every result equals the one with the option off; with
LUMINA_OCR_PDF_SCANS a /CCITTFaxDecode page of any /K is; a damaged strip is refused by the device and read by libtiff, as with the
option off."""
import numpy as np
import pytest
from PIL import Image, features

import ccitt_cases as cc
import fax_cases as fc
import pdf_cases as pc
import tiff_cases as tc
from lumina_ocr import synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the fax encoder of these cases")]

W, H = 700, 1000


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_tiff, s.device_pdf
    yield s
    s.device_tiff, s.device_pdf = saved
    s.cleanup()


@pytest.fixture(scope="module")
def blacks():
    return [synth.synth_page(H, W, seed, n_lines=12)[0].mean(axis=2) < 128 for seed in (41, 42, 43)]


def _untimed(v):
    if isinstance(v, dict):
        return {k: _untimed(x) for k, x in v.items() if "time" not in k}
    if isinstance(v, list):
        return [_untimed(x) for x in v]
    return v


def _same(a, b):
    return _untimed(a.to_dict()) == _untimed(b.to_dict())


def _spied(s, name, call):
    """call() with s.<name> (a _decode_*_pages method) wrapped: -> (call's result, [(pages the device decoded, reasons so far)])"""
    seen = []
    inner = getattr(s, name)

    def spy(entries, reasons):
        res = inner(entries, reasons)
        seen.append((sorted(res), dict(reasons)))
        return res
    setattr(s, name, spy)
    try:
        return call(), seen
    finally:
        delattr(s, name)


def test_three_page_tiff_of_three_codings(service, blacks, tmp_path):
    """1-D, 2-D with aligned EOLs, CCITT RLE; RowsPerStrip 7: 142 full strips and one of six rows a page, all of one group"""
    s = service
    frames = [fc.g3_frame(blacks[0], "1d", 0, 1, rps=7), fc.g3_frame(blacks[1], "2d_aligned", 1, 1, rps=7), fc.g3_frame(blacks[2], "rle", 0, 1, rps=7)]
    path = tmp_path / "fax.tif"
    path.write_bytes(tc.tiff_file(frames))
    s.device_tiff = True
    doc, seen = _spied(s, "_decode_tiff_pages", lambda: s.process_tiff_sync(path))
    assert seen == [([0, 1, 2], {})], seen
    assert doc.success and doc.total_pages == 3 and [(p.image_width, p.image_height) for p in doc.pages] == [(W, H)] * 3, doc.error
    s.device_tiff = False
    for k in range(3):
        im = Image.open(path)
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("L")) < 128, blacks[k])
        want = s.process_image_sync(im, page_number=k + 1)
        assert want.success and want.layout_boxes
        assert _same(doc.pages[k], want), k


def _on_and_off(s, data):
    s.device_tiff = False
    off = s.process_image_sync(data)
    s.device_tiff = True
    on, seen = _spied(s, "_decode_tiff_pages", lambda: s.process_image_sync(data))
    assert off.success and off.layout_boxes and (off.image_width, off.image_height) == (W, H), off.error
    return on, off, seen


def test_one_strip_fill_order_2(service, blacks):
    """a TIFF-F page as fax servers write it: one strip, two-dimensional, FillOrder 2, big-endian"""
    data = tc.tiff_file([fc.g3_frame(blacks[0], "2d", 0, 2)], big_endian=True)
    on, off, seen = _on_and_off(service, data)
    assert seen == [([0], {})] and _same(on, off)


def test_damaged_strip_is_libtiffs_with_the_option_on_as_off(service, blacks):
    frame = fc.g3_frame(blacks[1], "1d", 0, 1, rps=250)
    strip = frame["strips"][2]
    frame["strips"][2] = cc.flip_bit(strip, 8 * len(strip) - 60)   # one bit in the third strip's last lines: libtiff repairs the line
    on, off, seen = _on_and_off(service, tc.tiff_file([frame]))
    assert seen == [([], {0: "group3 strips corrupt (status -1)"})] and _same(on, off)


def test_pdf_pages_with_k_0_and_k_4(service, monkeypatch, tmp_path, blacks):
    s = service

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    image = lambda stream, parms: {"image": pc.image_obj(W, H, "/CCITTFaxDecode", stream, bits=1, parms=parms % (W, H)), "box": (504, 720)}
    doc_pages = [image(fc.g3_encode(blacks[0], "1d"), "<< /K 0 /Columns %d /Rows %d /EndOfLine true >>"),
                 image(fc.g3_encode(blacks[1], "2d"), "<< /K 4 /Columns %d /Rows %d /EndOfLine true /EndOfBlock false >>"),
                 image(fc.g3_encode(blacks[2], "rle"), "<< /K 0 /EncodedByteAlign true /Columns %d /Rows %d >>"),
                 image(fc.fax_encode_policy(blacks[2], eol=False), "<< /K 0 /Columns %d /Rows %d >>")]
    pdf = tmp_path / "fax.pdf"
    pdf.write_bytes(pc.document(doc_pages))
    s.device_pdf = True
    doc, seen = _spied(s, "_decode_pdf_pages", lambda: s.process_pdf_sync(pdf))
    assert seen == [([0, 1, 2, 3], {})], seen
    assert doc.success and doc.total_pages == 4, doc.error
    bilevel = [Image.fromarray(np.repeat(np.where(b, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)) for b in blacks]
    want = s.process_pages_sync(bilevel + [bilevel[2]])
    key = lambda r: (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height)
    for got, ref in zip(doc.pages, want):
        assert ref.success and ref.layout_boxes
        assert key(got) == key(ref)
