"""CPU: /JBIG2Decode in the scanned-PDF reader (utils/pdf_pages.py, read_pages(..., jbig2=True)) on PDFs made with the test-side JBIG2
encoder and the helpers of tests/pdf_layer_cases.py: a one-image JBIG2 page with and without /JBIG2Globals, /Decode [1 0], an /ImageMask
alone on a page, a JBIG2 stencil over a DCT background, a JBIG2 /Mask stream and a 1-bit JBIG2 /SMask; each record, decoded by the
restatement (tests/jbig2_reference.py) and put together by tests/pdf_layers_reference.py, shows the page the file was made from.  With
jbig2=False the same files give the refusals they gave before the option existed, and the provider asks for JBIG2 only with
LUMINA_OCR_PDF_JBIG2 (OCRService.pdf_jbig2) beside LUMINA_OCR_PDF_SCANS."""
import numpy as np
import pytest

import jbig2_cases as jc
import jbig2_reference as jr
import jbig2_writer as jw
import pdf_cases as pc
import pdf_layer_cases as lc
from lumina_ocr.utils import pdf_pages as pp

from pdf_jbig2_cases import BOX, FULL, decode_record, files as _files, render


@pytest.fixture(scope="module")
def files():
    return _files()


@pytest.mark.parametrize("name", ["one_image", "one_image_globals", "decode_1_0", "image_mask_alone", "stencil_over_dct", "mask_stream", "smask"])
def test_pages_show_their_bitmaps(files, name):
    data, want, layered = files[name]
    for layers in ((True,) if layered else (False, True)):
        entry, = pp.read_pages(data, layers=layers, jbig2=True)
        assert not isinstance(entry, pp.PdfRefused), entry.reason
        assert np.array_equal(render(entry), want), (name, layers)


def test_records(files):
    one, = pp.read_pages(files["one_image"][0], jbig2=True)
    assert (one.filter, one.width, one.height, one.params) == ("JBIG2Decode", FULL[1], FULL[0], {"globals": None, "invert": False})
    assert _probe_record(one)[0] == 0
    g, = pp.read_pages(files["one_image_globals"][0], jbig2=True)
    assert isinstance(g.params["globals"], bytes) and jr.probe(bytes(g.stream))[0] == -1 and jr.probe(bytes(g.stream), g.params["globals"])[0] == 0
    inv, = pp.read_pages(files["decode_1_0"][0], jbig2=True)
    assert inv.params["invert"] is True
    st, = pp.read_pages(files["stencil_over_dct"][0], layers=True, jbig2=True)
    assert [(l.kind, l.flip, None if l.mask is None else l.mask.filter) for l in st.layers] == [(0, 0, None), (1, 0, "JBIG2Decode")]
    assert st.layers[1].fill == lc.FILL8 and (st.width, st.height) == (FULL[1], FULL[0])
    m, = pp.read_pages(files["mask_stream"][0], layers=True, jbig2=True)
    assert [(l.kind, None if l.mask is None else l.mask.filter) for l in m.layers] == [(0, None), (3, "JBIG2Decode")]
    sm, = pp.read_pages(files["smask"][0], layers=True, jbig2=True)
    assert [(l.kind, None if l.mask is None else l.mask.filter) for l in sm.layers] == [(0, None), (2, "JBIG2Decode")]


def _probe_record(rec):
    return jr.probe(bytes(rec.stream), rec.params["globals"])


def test_refused_shapes_with_the_option_on():
    bm = jc.bitmap(20, 10, 77)
    first = lc.first_image_numbers([2])[0]
    e = "/Type /XObject /Subtype /Image /Width 20 /Height 10 /ColorSpace /DeviceGray /BitsPerComponent %d /Filter /JBIG2Decode %s"
    stream = jw.page(20, 10, [dict(bitmap=bm)])
    cases = [(pc.stream_obj(e % (8, ""), stream), "JBIG2 image that is not one bit of grey"),
             (pc.stream_obj(e.replace("/DeviceGray", "/DeviceRGB") % (1, ""), stream), "JBIG2 image that is not one bit of grey"),
             (pc.stream_obj(e % (1, "/DecodeParms << /JBIG2Globals 12 >>"), stream), "/JBIG2Globals is not a stream"),
             (pc.stream_obj(e % (1, "/Decode [0 0.5]"), stream), "/Decode [0, 0.5] on a mask")]
    for body, reason in cases:
        entry, = pp.read_pages(pc.document([{"image": body, "box": (20, 10)}]), jbig2=True)
        assert isinstance(entry, pp.PdfRefused) and entry.reason == reason, entry
    # a /JBIG2Globals reference that points at the image itself is followed once and refused, not followed for ever
    body = pc.stream_obj(e % (1, "/DecodeParms << /JBIG2Globals %d 0 R >>" % first), stream)
    entry, = pp.read_pages(pc.document([{"image": body, "box": (20, 10)}]), jbig2=True)
    assert isinstance(entry, pp.PdfRefused)


def test_option_off_gives_the_refusals_of_before(files):
    want = {"one_image": (False, "image filter JBIG2Decode"), "one_image_globals": (False, "image filter JBIG2Decode"),
            "decode_1_0": (False, "image filter JBIG2Decode"), "image_mask_alone": (False, "/ImageMask"),
            "stencil_over_dct": (True, "stencil filter JBIG2Decode"), "mask_stream": (True, "stencil filter JBIG2Decode"),
            "smask": (True, "/SMask filter JBIG2Decode")}
    for name, (layers, reason) in want.items():
        for kw in ({}, {"jbig2": False}):
            entry, = pp.read_pages(files[name][0], layers=layers, **kw)
            assert isinstance(entry, pp.PdfRefused) and entry.reason == reason, (name, entry)
    entry, = pp.read_pages(files["image_mask_alone"][0], layers=True)
    assert isinstance(entry, pp.PdfRefused) and entry.reason == "stencil filter JBIG2Decode"


# ---- the provider: which calls it makes

def _service(monkeypatch, **env):
    from lumina_ocr.services import ocr_service as svc
    for k in ("LUMINA_OCR_PDF_SCANS", "LUMINA_OCR_PDF_LAYERS", "LUMINA_OCR_PDF_JBIG2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = object.__new__(svc.OCRService)           # beside the process's singleton
    s._initialized = False
    svc.OCRService.__init__(s)
    return s, svc


def _recorded(monkeypatch, tmp_path, files, **env):
    """the calls process_pdf_sync makes to read_pages and to the rasteriser on a JBIG2 file, with no engine and no rasteriser"""
    s, svc = _service(monkeypatch, **env)
    calls = []
    real = svc.pdf_pages.read_pages

    def read_pages(data, **kw):
        calls.append(("read_pages", tuple(sorted(kw.items()))))
        entries = real(data, **kw)
        calls.append(("entries", tuple(type(e).__name__ for e in entries)))
        raise svc.pdf_pages.PdfRefused("stop here: this test has no device")

    def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
        calls.append(("pdf_to_images",))
        raise ImportError("pdf2image not installed. Install with: pip install pdf2image (and poppler)")

    monkeypatch.setattr(svc.pdf_pages, "read_pages", read_pages)
    monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
    pdf = tmp_path / "jbig2.pdf"
    pdf.write_bytes(files["one_image"][0])
    doc = s.process_pdf_sync(pdf)
    assert not doc.success
    return s, calls


def test_provider_option_off_makes_the_calls_of_before(monkeypatch, tmp_path, files):
    s, calls = _recorded(monkeypatch, tmp_path, files, LUMINA_OCR_PDF_SCANS="1")
    assert s.pdf_jbig2 is False and s.get_status()["pdf_jbig2"] is False
    assert calls == [("read_pages", (("strip_filters", False),)), ("entries", ("PdfRefused",)), ("pdf_to_images",)]
    s, calls = _recorded(monkeypatch, tmp_path, files, LUMINA_OCR_PDF_JBIG2="1")   # ignored without LUMINA_OCR_PDF_SCANS
    assert s.pdf_jbig2 is True and calls == [("pdf_to_images",)]
    s, calls = _recorded(monkeypatch, tmp_path, files)
    assert calls == [("pdf_to_images",)]


def test_provider_option_on_asks_for_jbig2(monkeypatch, tmp_path, files):
    s, calls = _recorded(monkeypatch, tmp_path, files, LUMINA_OCR_PDF_SCANS="1", LUMINA_OCR_PDF_JBIG2="1")
    assert s.get_status()["pdf_jbig2"] is True
    assert calls[:2] == [("read_pages", (("jbig2", True), ("strip_filters", False))), ("entries", ("PageImage",))]
    s, calls = _recorded(monkeypatch, tmp_path, files, LUMINA_OCR_PDF_SCANS="1", LUMINA_OCR_PDF_JBIG2="1", LUMINA_OCR_PDF_LAYERS="1")
    assert calls[0] == ("read_pages", (("jbig2", True), ("layers", True), ("strip_filters", False)))
