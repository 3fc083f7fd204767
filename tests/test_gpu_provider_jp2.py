"""GPU: JPEG 2000 inputs through the provider with LUMINA_OCR_DEVICE_JP2 (OCRService.device_jp2) on and off: JP2 bytes, a J2K path,
process_document, lazily opened pages of a batch and the /JPXDecode pages of a scanned PDF give the OCROutput the same pixels give as a
PNG; with the option off neither new engine entry is called; a 9/7 file goes to Pillow and still yields a result."""
import asyncio
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


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_jp2, s.device_pdf
    yield s
    s.device_jp2, s.device_pdf = saved
    s.cleanup()


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the two new bindings"""
    n = {"probe": 0, "decode": 0}
    probe, decode = Engine.jp2_probe, Engine.jp2_decode

    def counting_probe(data):
        n["probe"] += 1
        return probe(data)

    def counting_decode(self, *a, **kw):
        n["decode"] += 1
        return decode(self, *a, **kw)
    monkeypatch.setattr(Engine, "jp2_probe", staticmethod(counting_probe))
    monkeypatch.setattr(Engine, "jp2_decode", counting_decode)
    return n


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.processed_image_bytes, r.image_width, r.image_height)


def _png(rgb):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=6)[0] for seed in (31, 32, 33)]


def test_bytes_path_and_document(service, calls, tmp_path, pages):
    s = service
    jp2 = jc.write(pages[0], irreversible=False)
    j2k = jc.write(pages[1], irreversible=False, no_jp2=True, quality_layers=[12])   # layered: its pixels are Pillow's decode, not the source
    path = tmp_path / "scan.dat"   # (recognised by magic, not by extension)
    path.write_bytes(j2k)
    named = tmp_path / "scan.j2k"
    named.write_bytes(j2k)
    s.device_jp2 = True
    got_bytes, got_path = s.process_image_sync(jp2), s.process_image_sync(path)
    doc = asyncio.run(s.process_document(named, "j2k"))
    assert calls["decode"] == 3 and calls["probe"] == 3
    want_bytes = s.process_image_sync(_png(pages[0]))
    want_path = s.process_image_sync(_png(jc.expected(j2k)))
    assert got_bytes.success and got_bytes.layout_boxes, got_bytes.error
    assert _key(got_bytes) == _key(want_bytes) and _key(got_path) == _key(want_path)
    assert doc.success and doc.combined_markdown == want_path.markdown and doc.combined_layout_boxes == want_path.layout_boxes


def test_option_off_calls_neither_entry(service, calls, tmp_path, pages):
    s = service
    jp2 = jc.write(pages[0], irreversible=False)
    path = tmp_path / "scan.jp2"
    path.write_bytes(jp2)
    s.device_jp2 = False
    a, b = s.process_image_sync(jp2), s.process_image_sync(path)
    batch = s.process_pages_sync([Image.open(io.BytesIO(jp2))])
    doc = asyncio.run(s.process_document(path, "jp2"))
    assert calls == {"probe": 0, "decode": 0}
    assert a.success and _key(a) == _key(b) == _key(batch[0]) == _key(s.process_image_sync(_png(pages[0])))   # Pillow decoded it
    assert not doc.success and "Unsupported file type" in doc.error   # as before the option existed
    assert s.get_status()["device_jp2"] is False


def test_irreversible_file_goes_to_pillow(service, calls, pages):
    s = service
    lossy = jc.write(pages[2], irreversible=True, quality_layers=[10])
    s.device_jp2 = True
    got = s.process_image_sync(lossy)
    assert calls == {"probe": 1, "decode": 0}
    assert got.success and _key(got) == _key(s.process_image_sync(_png(jc.expected(lossy))))


def test_lazy_pages_grouped_by_size(service, calls, pages):
    s = service
    other = synth.synth_page(W, H, 34, n_lines=6)[0]
    files = [jc.write(pages[0], irreversible=False), jc.write(other, irreversible=False), jc.write(pages[1][:, :, 1].copy(), irreversible=False),
             jc.write(pages[2], irreversible=True)]
    s.device_jp2 = True
    opened = [Image.open(io.BytesIO(f)) for f in files]
    got = s.process_pages_sync(opened)
    assert calls["decode"] == 2   # two sizes; the 9/7 page is refused by the probe
    assert [getattr(im, "_im", None) is None for im in opened] == [True, True, True, False], "only the refused page may be decoded by Pillow"
    want = s.process_pages_sync([Image.fromarray(jc.expected(f)) for f in files])
    for p, q in zip(got, want):
        assert p.success and _key(p) == _key(q)


def test_three_page_jpx_pdf(service, calls, monkeypatch, tmp_path, pages):
    s = service

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    files = [jc.write(pages[0], irreversible=False), jc.write(pages[1][:, :, 1].copy(), irreversible=False, quality_layers=[15]),
             jc.write(pages[2], irreversible=False, no_jp2=True)]

    def obj(data, cs):
        return pc.stream_obj("/Type /XObject /Subtype /Image /Width %d /Height %d %s /BitsPerComponent 8 /Filter /JPXDecode" % (W, H, cs), data)
    pdf = tmp_path / "scan.pdf"
    pdf.write_bytes(pc.document([{"image": obj(files[0], "/ColorSpace /DeviceRGB"), "box": (504, 360)},
                                 {"image": obj(files[1], "/ColorSpace /DeviceGray"), "box": (504, 360), "attrs": "/Rotate 90"},
                                 {"image": obj(files[2], ""), "box": (504, 360)}]))
    s.device_pdf = s.device_jp2 = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success and doc.total_pages == 3, [p.error for p in doc.pages]
    assert calls["decode"] == 1   # one size, one call
    upright = [jc.expected(files[0]), np.ascontiguousarray(np.rot90(jc.expected(files[1]), -1)), jc.expected(files[2])]   # /Rotate 90: clockwise
    want = s.process_pages_sync([Image.fromarray(a) for a in upright])
    # (processed_image_bytes is left out of this key, as tests/test_gpu_provider_fax.py does for the PDF path; that the decoded pixels
    # are Pillow's is held in tests/test_gpu_jp2.py)
    key = lambda r: (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height)
    for got, w in zip(doc.pages, want):
        assert w.success and key(got) == key(w)
    # without the JPEG 2000 option the pages are refused by the reader, as before
    s.device_jp2 = False
    before = dict(calls)
    doc = s.process_pdf_sync(pdf)
    assert calls == before and not doc.success and "image filter JPXDecode" in doc.pages[0].error
