"""GPU: tiled JPEG 2000 inputs through the provider with LUMINA_OCR_JP2_TILES (OCRService.jp2_tiles) on and off: a tiled .jp2 path,
tiled bytes, lazily opened pages of a batch and a /JPXDecode page of a scanned PDF reach lumina_ocr_jp2_decode_ex and give the
OCROutput the Pillow path gives for the same file; the option combines with LUMINA_OCR_JP2_IRREVERSIBLE; with it off the provider makes
the calls it made before, and the option alone, without LUMINA_OCR_DEVICE_JP2, changes nothing."""
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
NAMES = ("jp2_probe", "jp2_decode", "jp2_probe_irreversible", "jp2_decode_irreversible", "jp2_probe_ex", "jp2_decode_ex")
TILED = dict(tile_size=(128, 128), precinct_size=(64, 64), progression="RPCL")


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_jp2, s.device_pdf, s.jp2_irreversible, s.jp2_tiles
    yield s
    s.device_jp2, s.device_pdf, s.jp2_irreversible, s.jp2_tiles = saved
    s.cleanup()


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the six JPEG 2000 bindings, and keeps the flags of the last _ex call"""
    n = dict.fromkeys(NAMES, 0)
    n["flags"] = None

    def counting(name, static):
        inner = getattr(Engine, name)

        def probe(data, *flags):
            n[name] += 1
            if flags:
                n["flags"] = flags[0]
            return inner(data, *flags)

        def decode(self, *a, **kw):
            n[name] += 1
            if name.endswith("_ex"):
                n["flags"] = a[3] if len(a) > 3 else kw["flags"]
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


def _counts(calls):
    return {k: calls[k] for k in NAMES}


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=6)[0] for seed in (45, 46)]


def test_default_is_off(service):
    assert service.jp2_tiles is False and service.get_status()["jp2_tiles"] is False


def test_path_and_bytes(service, calls, tmp_path, pages):
    s = service
    tiled = jc.write(pages[0], irreversible=False, **TILED)
    grey = jc.write(np.ascontiguousarray(pages[1][:, :, 1]), irreversible=False, tile_size=(256, 256), offset=(3, 5))
    path = tmp_path / "scan.jp2"
    path.write_bytes(grey)
    s.device_jp2 = s.jp2_tiles = True
    s.jp2_irreversible = False
    got_bytes, got_path = s.process_image_sync(tiled), s.process_image_sync(path)
    assert _counts(calls) == dict.fromkeys(NAMES, 0) | {"jp2_probe_ex": 2, "jp2_decode_ex": 2} and calls["flags"] == Engine.JP2_F_TILES
    want_bytes, want_path = s.process_image_sync(_png(jc.expected(tiled))), s.process_image_sync(_png(jc.expected(grey)))
    assert got_bytes.success and got_bytes.layout_boxes, got_bytes.error
    assert _key(got_bytes) == _key(want_bytes) and _key(got_path) == _key(want_path)
    # with LUMINA_OCR_JP2_IRREVERSIBLE both flags travel, and a tiled 9/7 file is decoded on the device too
    lossy = jc.write(pages[0], irreversible=True, quality_layers=[10], **TILED)
    s.jp2_irreversible = True
    before = _counts(calls)
    got_lossy = s.process_image_sync(lossy)
    assert _counts(calls) == before | {"jp2_probe_ex": 3, "jp2_decode_ex": 3} and calls["flags"] == Engine.JP2_F_TILES | Engine.JP2_F_IRREVERSIBLE
    assert _key(got_lossy) == _key(s.process_image_sync(_png(jc.expected(lossy))))
    # option off: the plain probe refuses the file and Pillow decodes it, as before; the result is the same
    s.jp2_tiles = s.jp2_irreversible = False
    before = _counts(calls)
    off = s.process_image_sync(tiled)
    assert _counts(calls) == before | {"jp2_probe": 1} and _key(off) == _key(want_bytes)
    # the option without LUMINA_OCR_DEVICE_JP2 is ignored: no entry is called
    s.device_jp2, s.jp2_tiles = False, True
    before = _counts(calls)
    ignored = s.process_image_sync(tiled)
    assert _counts(calls) == before and _key(ignored) == _key(want_bytes)


def test_lazy_pages(service, calls, pages):
    s = service
    files = [jc.write(pages[0], irreversible=False, **TILED), jc.write(pages[1], irreversible=False),
             jc.write(pages[1][:, :, 1].copy(), irreversible=False, tile_size=(200, 100), quality_layers=[15])]
    s.device_jp2 = s.jp2_tiles = True
    opened = [Image.open(io.BytesIO(f)) for f in files]
    got = s.process_pages_sync(opened)
    assert calls["jp2_decode_ex"] == 1 and calls["jp2_decode"] == 0   # one size, one call, tiled and one-tile files in it
    assert all(getattr(im, "_im", None) is None for im in opened), "no page may be decoded by Pillow"
    want = s.process_pages_sync([Image.fromarray(jc.expected(f)) for f in files])
    for p, q in zip(got, want):
        assert p.success and _key(p) == _key(q)


def test_jpx_pdf_page(service, calls, monkeypatch, tmp_path, pages):
    s = service

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        raise ImportError("pdf2image not installed")
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    files = [jc.write(pages[0], irreversible=False, **TILED), jc.write(pages[1], irreversible=False)]

    def obj(data):
        return pc.stream_obj("/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /JPXDecode" % (W, H), data)
    pdf = tmp_path / "scan.pdf"
    pdf.write_bytes(pc.document([{"image": obj(f), "box": (504, 360)} for f in files]))
    s.device_pdf = s.device_jp2 = s.jp2_tiles = True
    doc = s.process_pdf_sync(pdf)
    assert doc.success and doc.total_pages == 2, [p.error for p in doc.pages]
    assert calls["jp2_decode_ex"] == 1 and calls["jp2_decode"] == 0 and calls["jp2_decode_irreversible"] == 0
    want = s.process_pages_sync([Image.fromarray(jc.expected(f)) for f in files])
    key = lambda r: (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height)   # (as tests/test_gpu_provider_jp2.py)
    for got, w in zip(doc.pages, want):
        assert w.success and key(got) == key(w)
    # option off: the plain entry is called as before, and never the new one
    s.jp2_tiles = False
    before = _counts(calls)
    s.process_pdf_sync(pdf)
    assert calls["jp2_decode"] == before["jp2_decode"] + 1 and calls["jp2_decode_ex"] == before["jp2_decode_ex"]
