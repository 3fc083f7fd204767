"""GPU: WebP inputs through the provider with the device WebP decoder on and off (LUMINA_OCR_DEVICE_WEBP).  Lossless files from a path
and from bytes, with and without an EXIF orientation: the results must be identical either way and the device path must really have
decoded the file; lossy files and files with XMP must make no device-decode call; with the option off no WebP entry is called at all."""
import io

import numpy as np
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
    saved = s.device_webp
    yield s
    s.device_webp = saved
    s.cleanup()


@pytest.fixture
def calls(service, monkeypatch):
    """counts of every WebP entry: the service's hook, the probe and the device decode"""
    s = service
    s._ensure_engine()
    counts = {"hook": 0, "probe": 0, "decode": 0}
    hook, probe, decode = s._process_webp_on_device, Engine.webp_probe, s._engine.webp_decode

    def c_hook(*a, **kw):
        counts["hook"] += 1
        return hook(*a, **kw)

    def c_probe(data):
        counts["probe"] += 1
        return probe(data)

    def c_decode(*a, **kw):
        counts["decode"] += 1
        return decode(*a, **kw)
    monkeypatch.setattr(s, "_process_webp_on_device", c_hook)
    monkeypatch.setattr(Engine, "webp_probe", staticmethod(c_probe))
    monkeypatch.setattr(s._engine, "webp_decode", c_decode)
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


def test_lossless_path_and_bytes_device_equals_host(service, calls, tmp_path):
    s = service
    data = _webp(_page(), lossless=True)
    path = tmp_path / "page.bin"   # (recognised by magic, never by extension)
    path.write_bytes(data)
    s.device_webp = True
    dev_path, dev_bytes = s.process_image_sync(path), s.process_image_sync(data)
    assert calls["decode"] == 2 and calls["hook"] == 2
    s.device_webp = False
    host_path, host_bytes = s.process_image_sync(path), s.process_image_sync(data)
    assert calls["decode"] == 2 and calls["hook"] == 2
    assert dev_path.success and dev_path.layout_boxes, dev_path.error
    assert _key(dev_path) == _key(host_path) and _key(dev_bytes) == _key(host_bytes) == _key(host_path)


@pytest.mark.parametrize("orientation", [1, 3, 6, 8])
def test_exif_orientation_device_equals_host(service, calls, orientation):
    s = service
    data = _webp(_page(12), lossless=True, exif=_exif(orientation))
    assert Engine.webp_probe(data)[1]["exif"] == 1
    s.device_webp = True
    dev = s.process_image_sync(data)
    assert calls["decode"] == 1
    s.device_webp = False
    host = s.process_image_sync(data)
    assert calls["decode"] == 1
    assert dev.success and dev.layout_boxes and _key(dev) == _key(host)
    if orientation in (6, 8):
        assert (host.image_width, host.image_height) == (dev.image_width, dev.image_height)


def test_lossy_and_xmp_files_make_no_device_decode(service, calls):
    s = service
    lossy = _webp(_page(4), quality=80)
    xmp = _webp(_page(4), lossless=True, xmp=b'<x:xmpmeta xmlns:x="adobe:ns:meta/"></x:xmpmeta>')
    assert Image.open(io.BytesIO(xmp)).info.get("xmp")
    for data in (lossy, xmp):
        s.device_webp = True
        dev = s.process_image_sync(data)
        s.device_webp = False
        host = s.process_image_sync(data)
        assert dev.success and _key(dev) == _key(host)
    assert calls["decode"] == 0 and calls["hook"] == 2


def test_option_off_calls_no_webp_entry(service, calls, tmp_path):
    s = service
    s.device_webp = False
    data = _webp(_page(), lossless=True)
    path = tmp_path / "page.webp"
    path.write_bytes(data)
    assert s.process_image_sync(path).success and s.process_image_sync(data).success
    assert calls == {"hook": 0, "probe": 0, "decode": 0}


def test_option_is_off_by_default(monkeypatch):
    from lumina_ocr.services import ocr_service as svc
    monkeypatch.delenv("LUMINA_OCR_DEVICE_WEBP", raising=False)
    s = svc.OCRService()
    try:
        assert s.device_webp is False
    finally:
        s.cleanup()
