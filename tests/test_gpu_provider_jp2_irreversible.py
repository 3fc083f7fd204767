"""GPU: 9/7 JPEG 2000 inputs through the provider with LUMINA_OCR_JP2_IRREVERSIBLE (OCRService.jp2_irreversible) on and off: a
9/7 .jp2 path, bytes, lazily opened pages of a batch and a /JPXDecode page of a scanned PDF give the OCROutput the Pillow path gives
for the same file; with the option off the provider makes the calls it made before (the plain pair, never the new one), and the
option alone, without LUMINA_OCR_DEVICE_JP2, changes nothing."""
import io

import numpy as np
import pytest
from PIL import Image

import jp2_cases as jc
import pdf_cases as pc
from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu

H, W = 300, 420
NAMES = ("jp2_probe", "jp2_decode", "jp2_probe_irreversible", "jp2_decode_irreversible")


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_jp2, s.device_pdf, s.jp2_irreversible
    yield s
    s.device_jp2, s.device_pdf, s.jp2_irreversible = saved
    s.cleanup()


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the four JPEG 2000 bindings"""
    n = dict.fromkeys(NAMES, 0)

    def counting(name, static):
        inner = getattr(Engine, name)

        def probe(data):
            n[name] += 1
            return inner(data)

        def decode(self, *a, **kw):
            n[name] += 1
            return inner(self, *a, **kw)
        return staticmethod(probe) if static else decode
    for name in NAMES:
        monkeypatch.setattr(Engine, name, counting(name, "probe" in name))
    return n


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.processed_image_bytes, r.image_width, r.image_height)


def _png(rgb):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=6)[0] for seed in (35, 36)]


def test_default_is_off(service):
    assert service.jp2_irreversible is False


def test_path_and_bytes(service, calls, tmp_path, pages):
    s = service
    lossy = jc.write(pages[0], irreversible=True, quality_layers=[10])
    grey = jc.write(np.ascontiguousarray(pages[1][:, :, 1]), irreversible=True)
    path = tmp_path / "scan.jp2"
    path.write_bytes(grey)
    s.device_jp2 = s.jp2_irreversible = True
    got_bytes, got_path = s.process_image_sync(lossy), s.process_image_sync(path)
    assert calls == {"jp2_probe": 0, "jp2_decode": 0, "jp2_probe_irreversible": 2, "jp2_decode_irreversible": 2}
    want_bytes, want_path = s.process_image_sync(_png(jc.expected(lossy))), s.process_image_sync(_png(jc.expected(grey)))
    assert got_bytes.success and got_bytes.layout_boxes, got_bytes.error
    assert _key(got_bytes) == _key(want_bytes) and _key(got_path) == _key(want_path)
    # option off: the plain probe refuses the file and Pillow decodes it, as before; the result is the same
    s.jp2_irreversible = False
    before = dict(calls)
    off = s.process_image_sync(lossy)
    assert calls == dict(before, jp2_probe=1) and _key(off) == _key(want_bytes)
    # the option without LUMINA_OCR_DEVICE_JP2 is ignored: no entry is called
    s.device_jp2, s.jp2_irreversible = False, True
    before = dict(calls)
    ignored = s.process_image_sync(lossy)
    assert calls == before and _key(ignored) == _key(want_bytes)


def test_lazy_pages_of_both_transforms(service, calls, pages):
    s = service
    files = [jc.write(pages[0], irreversible=True), jc.write(pages[1], irreversible=False), jc.write(pages[1][:, :, 1].copy(), irreversible=True, quality_layers=[15])]
    s.device_jp2 = s.jp2_irreversible = True
    opened = [Image.open(io.BytesIO(f)) for f in files]
    got = s.process_pages_sync(opened)
    assert calls["jp2_decode_irreversible"] == 1 and calls["jp2_decode"] == 0   # one size, one call, both transforms in it
    assert all(getattr(im, "_im", None) is None for im in opened), "no page may be decoded by Pillow"
    want = s.process_pages_sync([Image.fromarray(jc.expected(f)) for f in files])
    for p, q in zip(got, want):
        assert p.success and _key(p) == _key(q)


def test_jpx_pdf_page(service, calls, monkeypatch, tmp_path, pages):
    s = service

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    files = [jc.write(pages[0], irreversible=True, quality_layers=[12]), jc.write(pages[1], irreversible=False)]

    def obj(data):
        return pc.stream_obj("/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /JPXDecode" % (W, H), data)
    pdf = tmp_path / "scan.pdf"
    pdf.write_bytes(pc.document([{"image": obj(f), "box": (504, 360)} for f in files]))
    s.device_pdf = s.device_jp2 = s.jp2_irreversible = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success and doc.total_pages == 2, [p.error for p in doc.pages]
    assert calls["jp2_decode_irreversible"] == 1 and calls["jp2_decode"] == 0
    want = s.process_pages_sync([Image.fromarray(jc.expected(f)) for f in files])
    key = lambda r: (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height)   # (as tests/test_gpu_provider_jp2.py)
    for got, w in zip(doc.pages, want):
        assert w.success and key(got) == key(w)
    # option off: the plain entry is called as before, and never the new one
    s.jp2_irreversible = False
    before = dict(calls)
    s.process_pdf_sync(pdf)
    assert calls["jp2_decode"] == before["jp2_decode"] + 1 and calls["jp2_decode_irreversible"] == before["jp2_decode_irreversible"]
