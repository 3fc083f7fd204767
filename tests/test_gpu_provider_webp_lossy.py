"""GPU: lossy WebP inputs through the provider with LUMINA_OCR_DEVICE_WEBP and LUMINA_OCR_WEBP_LOSSY.  With both on, a lossy path and
lossy bytes give the Pillow path's result and the device really decoded them; with only the first no lossy entry is called; with only the
second no WebP entry at all; EXIF orientation 6 is applied on the device; a file with XMP and one with ALPH make no device decode."""
import io

import pytest
from PIL import Image

from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_webp, s.webp_lossy
    yield s
    s.device_webp, s.webp_lossy = saved
    s.cleanup()


@pytest.fixture
def calls(service, monkeypatch):
    """counts of every WebP entry: the service's hook, the two probes and the two device decodes"""
    s = service
    s._ensure_engine()
    counts = {"hook": 0, "probe": 0, "decode": 0, "probe_lossy": 0, "decode_lossy": 0}

    def counted(key, fn):
        def f(*a, **kw):
            counts[key] += 1
            return fn(*a, **kw)
        return f
    monkeypatch.setattr(s, "_process_webp_on_device", counted("hook", s._process_webp_on_device))
    monkeypatch.setattr(Engine, "webp_probe", staticmethod(counted("probe", Engine.webp_probe)))
    monkeypatch.setattr(Engine, "webp_probe_lossy", staticmethod(counted("probe_lossy", Engine.webp_probe_lossy)))
    monkeypatch.setattr(s._engine, "webp_decode", counted("decode", s._engine.webp_decode))
    monkeypatch.setattr(s._engine, "webp_decode_lossy", counted("decode_lossy", s._engine.webp_decode_lossy))
    return counts


def _page(seed=9):
    return Image.fromarray(synth.synth_page(300, 420, seed, n_lines=6)[0])


def _webp(im, **kw):
    b = io.BytesIO()
    im.save(b, "WEBP", **kw)
    return b.getvalue()


def _exif(orientation):
    e = Image.Exif()
    e[0x0112] = orientation
    return e.tobytes()


def _key(r):
    return (r.success, r.error, r.markdown, r.layout_boxes, r.processed_image_bytes, r.image_width, r.image_height)


def test_lossy_path_and_bytes_device_equals_host(service, calls, tmp_path):
    s = service
    data = _webp(_page(), quality=80)
    assert Engine.webp_probe_lossy(data)[1]["lossy"] == 1
    calls["probe_lossy"] = 0
    path = tmp_path / "page.bin"   # (recognised by magic, never by extension)
    path.write_bytes(data)
    s.device_webp = s.webp_lossy = True
    dev_path = s.process_image_sync(path)
    assert calls["decode_lossy"] == 1 and calls["probe_lossy"] == 1
    dev_bytes = s.process_image_sync(data)
    assert calls["decode_lossy"] == 2 and calls["hook"] == 2 and calls["decode"] == 0 and calls["probe"] == 0
    s.device_webp = s.webp_lossy = False
    host_path, host_bytes = s.process_image_sync(path), s.process_image_sync(data)
    assert calls["decode_lossy"] == 2 and calls["hook"] == 2
    assert dev_path.success and dev_path.layout_boxes, dev_path.error
    assert _key(dev_path) == _key(host_path) and _key(dev_bytes) == _key(host_bytes) == _key(host_path)


def test_device_webp_alone_calls_no_lossy_entry(service, calls):
    s = service
    s.device_webp, s.webp_lossy = True, False
    lossy, lossless = _webp(_page(4), quality=80), _webp(_page(4), lossless=True)
    assert s.process_image_sync(lossy).success and s.process_image_sync(lossless).success
    assert calls["probe_lossy"] == 0 and calls["decode_lossy"] == 0 and calls["probe"] == 2 and calls["decode"] == 1


def test_webp_lossy_alone_calls_no_webp_entry(service, calls):
    s = service
    s.device_webp, s.webp_lossy = False, True
    assert s.process_image_sync(_webp(_page(4), quality=80)).success and s.process_image_sync(_webp(_page(4), lossless=True)).success
    assert calls == {"hook": 0, "probe": 0, "decode": 0, "probe_lossy": 0, "decode_lossy": 0}


def test_exif_orientation_6_device_equals_host(service, calls):
    s = service
    data = _webp(_page(12), quality=85, exif=_exif(6))
    assert Engine.webp_probe_lossy(data)[1]["exif"] == 1
    s.device_webp = s.webp_lossy = True
    dev = s.process_image_sync(data)
    assert calls["decode_lossy"] == 1
    s.device_webp = s.webp_lossy = False
    host = s.process_image_sync(data)
    assert calls["decode_lossy"] == 1
    assert dev.success and dev.layout_boxes and _key(dev) == _key(host)
    assert (host.image_width, host.image_height) == (dev.image_width, dev.image_height)


def test_xmp_and_alph_files_make_no_device_decode(service, calls):
    s = service
    xmp = _webp(_page(4), quality=80, xmp=b'<x:xmpmeta xmlns:x="adobe:ns:meta/"></x:xmpmeta>')
    assert Image.open(io.BytesIO(xmp)).info.get("xmp")
    rgba = _page(4).convert("RGBA")
    rgba.putalpha(Image.linear_gradient("L").resize(rgba.size))
    alph = _webp(rgba, quality=80)
    assert Engine.webp_probe_lossy(alph)[0] == -2
    for data in (xmp, alph):
        s.device_webp = s.webp_lossy = True
        dev = s.process_image_sync(data)
        s.device_webp = s.webp_lossy = False
        host = s.process_image_sync(data)
        assert dev.success and _key(dev) == _key(host)
    assert calls["decode_lossy"] == 0 and calls["decode"] == 0 and calls["hook"] == 2


def test_option_is_off_by_default(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    monkeypatch.delenv("LUMINA_OCR_WEBP_LOSSY", raising=False)
    s = svc.OCRService()
    try:
        assert s.webp_lossy is False
    finally:
        s.cleanup()
