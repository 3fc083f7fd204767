"""GPU: PNG inputs through the provider with the device PNG decoder on and off (LUMINA_OCR_DEVICE_PNG).  Single images from a path and
from bytes, process_document(..., "png"), and PDF pages that arrive as lazily opened PNG images (what pdf2image returns): the results
must be identical either way, the device path must never make Pillow decode the file, and refused files must take today's path."""
import asyncio
import io

import numpy as np
import pytest
from PIL import Image, PngImagePlugin

import png_cases as pc
from lumina_ocr import synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_png
    yield s
    s.device_png = saved
    s.cleanup()


@pytest.fixture
def load_calls(monkeypatch):
    calls = []
    orig = PngImagePlugin.PngImageFile.load

    def counting(self, *a, **kw):
        calls.append(1)
        return orig(self, *a, **kw)
    monkeypatch.setattr(PngImagePlugin.PngImageFile, "load", counting)
    return calls


def _with_exif(data: bytes, orientation: int) -> bytes:
    """the same file with an eXIf chunk (before IDAT) carrying the orientation"""
    p = data.index(b"IDAT") - 4
    return data[:p] + pc.chunk(b"eXIf", pc.exif_orientation(orientation)) + data[p:]


def _pages():
    page = synth.synth_page(300, 420, 9, n_lines=6)[0]
    im = Image.fromarray(page)
    rng = np.random.default_rng(1)
    alpha = Image.fromarray(rng.integers(0, 256, page.shape[:2], dtype=np.uint8))
    return {
        "RGB": pc.pil_bytes(im),
        "RGBA": pc.pil_bytes(Image.merge("RGBA", (*im.split(), alpha))),
        "P": pc.pil_bytes(im.quantize(32)),
        "L": pc.pil_bytes(im.convert("L")),
        "LA": pc.pil_bytes(Image.merge("LA", (im.convert("L"), alpha))),
        "1": pc.pil_bytes(im.convert("L").point(lambda v: 255 if v > 160 else 0).convert("1")),
    }


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.processed_image_bytes, r.image_width, r.image_height)


@pytest.mark.parametrize("mode", ["RGB", "RGBA", "P", "L", "LA", "1"])
@pytest.mark.parametrize("orientation", [None, 6])
def test_single_image_device_equals_host(service, load_calls, tmp_path, mode, orientation):
    s = service
    data = _pages()[mode]
    if orientation:
        data = _with_exif(data, orientation)
    path = tmp_path / "page.png"
    path.write_bytes(data)
    s.device_png = True
    load_calls.clear()
    dev_path, dev_bytes = s.process_image_sync(path), s.process_image_sync(data)
    doc = asyncio.run(s.process_document(path, "png"))
    assert load_calls == [], "the device path made Pillow decode the file"
    s.device_png = False
    host_path, host_bytes = s.process_image_sync(path), s.process_image_sync(data)
    assert load_calls, "the host path is expected to decode with Pillow"
    assert dev_path.success and dev_path.layout_boxes, dev_path.error
    assert _key(dev_path) == _key(host_path) and _key(dev_bytes) == _key(host_bytes) == _key(host_path)
    assert doc.success and doc.combined_markdown == host_path.markdown and doc.combined_layout_boxes == host_path.layout_boxes


@pytest.mark.parametrize("kind", ["raw_profile", "xmp"])
def test_orientation_from_a_text_chunk(service, monkeypatch, tmp_path, kind):
    """The host path rotates such a page (auto_orient); with the device path on the result must be the same, as a single image and
    as a PDF page."""
    s = service
    data = pc.text_orientation_files(Image.fromarray(synth.synth_page(300, 420, 12, n_lines=6)[0]))[kind]
    s.device_png = False
    host = s.process_image_sync(data)
    assert host.success and (host.page_width_inches, host.page_height_inches) == (300.0, 420.0)   # rotated: 420 x 300 -> 300 x 420
    s.device_png = True
    assert _key(s.process_image_sync(data)) == _key(host)
    monkeypatch.setattr(s._pre, "pdf_to_images", lambda path, dpi=None: [Image.open(io.BytesIO(data))])
    pdf = tmp_path / "doc.pdf"
    pdf.write_bytes(b"%PDF-1.4 stand-in")
    doc = asyncio.run(s.process_document(pdf, "pdf"))
    assert doc.success and _key(doc.pages[0]) == _key(host)


def test_refused_file_takes_the_host_path(service, load_calls, tmp_path):
    """A 16-bit page (-2) and one with a chunk after IDAT (-2): the same result as with the device path off, decoded by Pillow."""
    s = service
    page = synth.synth_page(200, 260, 4, n_lines=4)[0].astype(np.int64)
    files = [pc.write_png(page.reshape(200, -1) * 257, 260, 200, 16, 2),
             pc.write_png(page.reshape(200, -1), 260, 200, 8, 2, tail=pc.chunk(b"tEXt", b"k\x00v") + pc.chunk(b"IEND", b""))]
    for data in files:
        s.device_png = True
        load_calls.clear()
        dev = s.process_image_sync(data)
        assert load_calls, "a refused file must be decoded by Pillow"
        s.device_png = False
        host = s.process_image_sync(data)
        assert dev.success and _key(dev) == _key(host)


def test_pdf_pages_as_lazy_png_images(service, monkeypatch, tmp_path):
    """pdf_to_images stand-in returning lazily opened PNG pages of two sizes (one with EXIF orientation 6, one refused 16-bit page):
    one png_decode per size group, results equal to the host path."""
    s = service
    a, b, c = (synth.synth_page(*hw, seed, n_lines=6)[0] for hw, seed in (((360, 260), 1), ((260, 360), 2), ((360, 260), 3)))
    files = [pc.pil_bytes(Image.fromarray(a)), pc.pil_bytes(Image.fromarray(b).quantize(64)), _with_exif(pc.pil_bytes(Image.fromarray(c)), 6),
             pc.pil_bytes(Image.fromarray(c).convert("L")), pc.write_png(a.astype(np.int64).reshape(360, -1) * 257, 260, 360, 16, 2)]
    opened = []

    def pdf_to_images(path, dpi=None):
        opened.append([Image.open(io.BytesIO(f)) for f in files])
        return opened[-1]
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    pdf = tmp_path / "doc.pdf"
    pdf.write_bytes(b"%PDF-1.4 stand-in")
    s._ensure_engine()
    calls = []
    orig = s._engine.png_decode

    def counting(files_, h, w, out=None):
        calls.append((len(files_), h, w))
        return orig(files_, h, w, out)
    monkeypatch.setattr(s._engine, "png_decode", counting)
    s.device_png = True
    dev = asyncio.run(s.process_document(pdf, "pdf"))
    assert sorted(calls) == sorted([(3, 360, 260), (1, 260, 360)]), calls   # the 16-bit page is refused by the probe
    assert [getattr(im, "_im", None) is None for im in opened[0]] == [True] * 4 + [False], "only the refused page may be decoded by Pillow"
    s.device_png = False
    host = asyncio.run(s.process_document(pdf, "pdf"))
    assert dev.success and host.success and dev.total_pages == 5
    for p, q in zip(dev.pages, host.pages):
        assert _key(p) == _key(q) and p.page_number == q.page_number
    assert dev.combined_markdown == host.combined_markdown
