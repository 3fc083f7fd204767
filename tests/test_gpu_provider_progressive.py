"""GPU: LUMINA_OCR_PROGRESSIVE_JPEG through the provider.  Option on: a progressive .jpg (path and bytes) and a progressive /DCTDecode
page of a scanned PDF are decoded on the device (Engine.jpeg_decode_progressive) and give the host path's boxes, markdown and processed
bytes.  Option off (the default): the new engine method is never called and the results are the same."""
import io

import pytest
from PIL import Image

import pdf_cases
from lumina_ocr import synth

pytestmark = pytest.mark.gpu

W, H = 700, 1000


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    yield s
    s.cleanup()


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.processed_image_bytes, r.image_width, r.image_height)


def test_progressive_inputs_on_and_off(service, monkeypatch, tmp_path):
    s = service
    assert s.progressive_jpeg is False and s.get_status()["progressive_jpeg"] is False      # off by default
    page = synth.synth_page(H, W, 31, n_lines=12)[0]
    f = tmp_path / "prog.jpg"
    Image.fromarray(page).save(f, format="JPEG", quality=90, progressive=True)
    data = f.read_bytes()
    pdf = tmp_path / "prog.pdf"
    pdf.write_bytes(pdf_cases.document([{"image": pdf_cases.image_obj(W, H, "/DCTDecode", data, cs="/DeviceRGB"), "box": (504, 720)}]))

    def no_rasteriser(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed")
    monkeypatch.setattr(s._pre, "pdf_to_images", no_rasteriser)
    s._ensure_engine()
    calls = []
    real = s._engine.jpeg_decode_progressive

    def counted(files, *a, **k):
        out, status = real(files, *a, **k)
        calls.append(list(status))
        return out, status
    s._engine.jpeg_decode_progressive = counted
    s.device_pdf = True
    # option off: Pillow decodes the progressive file, the new method is not called
    host = s.process_image_sync(f)
    host_doc = s.process_pdf_sync(pdf)
    assert host.success and host.layout_boxes and host_doc.success and not calls
    # option on
    s.progressive_jpeg = True
    assert s.get_status()["progressive_jpeg"] is True
    dev_path, dev_bytes = s.process_image_sync(f), s.process_image_sync(data)
    doc = s.process_pdf_sync(pdf)
    assert calls == [[0], [0], [0]]
    assert doc.success and doc.total_pages == 1, doc.error
    for r in (dev_path, dev_bytes):
        assert _key(r) == _key(host)
    assert _key(doc.pages[0])[:4] == _key(host_doc.pages[0])[:4] and doc.pages[0].processed_image_bytes == host_doc.pages[0].processed_image_bytes
    # a baseline file with the option on: the same result as with it off
    b = io.BytesIO()
    Image.fromarray(page).save(b, format="JPEG", quality=90)
    on = s.process_image_sync(b.getvalue())
    s.progressive_jpeg = False
    off = s.process_image_sync(b.getvalue())
    assert calls[-1] == [0] and len(calls) == 4 and _key(on) == _key(off)


def test_environment_variable_sets_the_option(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    monkeypatch.setenv("LUMINA_OCR_PROGRESSIVE_JPEG", "1")
    monkeypatch.setattr(svc.OCRService, "_instance", None)      # (the provider is a singleton: a fresh one reads the environment)
    s = svc.OCRService()
    try:
        assert s.progressive_jpeg is True and s.get_status()["progressive_jpeg"] is True
    finally:
        s.cleanup()
