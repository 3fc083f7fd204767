"""The host half of the EAN / UPC / ITF kinds (lumina_ocr/utils/barcodes.py, utils/layout.py, arch.py, pipeline.py, the provider):
digits to text, UPC-A and ITF-14, the `barcode` entries and the `:barcode:` line, the kind names and the provider's variable; the
defaults are what they were."""
import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.pipeline import OcrPipeline, PageDetections
from lumina_ocr.utils import barcodes as bc
from lumina_ocr.utils import layout

from test_barcode_layout import _line, _rows
from test_mark_layout import _service, q


def digits(s):
    return [int(c) for c in s]


def test_digits_to_text():
    assert bc.symbols_text(bc.KIND_EAN13, digits("4006381333931")) == "4006381333931"
    assert bc.symbols_text(bc.KIND_EAN13, digits("4006381333932")) is None and bc.symbols_text(bc.KIND_EAN13, digits("400638133393")) is None
    assert bc.symbols_text(bc.KIND_EAN8, digits("96385074")) == "96385074" and bc.symbols_text(bc.KIND_EAN8, digits("96385075")) is None
    assert bc.symbols_text(bc.KIND_UPCE, digits("01234565")) == "01234565" and bc.symbols_text(bc.KIND_UPCE, digits("01234566")) is None
    assert bc.symbols_text(bc.KIND_UPCE, digits("21234565")) is None                                 # number system 0 or 1
    assert bc.symbols_text(bc.KIND_ITF, digits("123456")) == "123456" and bc.symbols_text(bc.KIND_ITF, digits("1234")) is None
    assert bc.symbols_text(bc.KIND_ITF, digits("12345")) is None and bc.symbols_text(bc.KIND_ITF, [1, 2, 3, 4, 5, 10]) is None
    assert bc.symbols_text(6, [1]) is None
    assert bc.mod10_ok(digits("00012345678905")) and not bc.mod10_ok(digits("00012345678906")) and bc.mod10_ok(digits("036000291452"))


def test_upce_to_upca_every_branch():
    for upce, upca in (("01234565", "012345000065"), ("04252614", "042100005264"), ("01234531", "012300000451"), ("01234543", "012340000053"),
                       ("01200003", "012000000003"), ("11234511", "112100003451")):
        assert bc.upce_to_upca(digits(upce)) == digits(upca), upce
        assert bc.mod10_ok(digits(upca)) and bc.symbols_text(bc.KIND_UPCE, digits(upce)) == upce, upce
    assert bc.upce_to_upca(digits("0123456")) is None and bc.upce_to_upca(digits("31234565")) is None


def test_entries_upca_itf14_polygon_and_validator():
    rows, syms = _rows(((100, 200, 289, 249, 2, 13, 50, 0), digits("4006381333931")), ((100, 300, 289, 349, 2, 13, 25, 1), digits("0036000291452")),
                       ((400, 100, 429, 233, 3, 8, 30, 2), digits("96385074")), ((20, 400, 121, 439, 4, 8, 40, 0), digits("01234565")),
                       ((200, 400, 411, 439, 5, 14, 40, 4), digits("00012345678905")), ((200, 500, 411, 539, 5, 14, 40, 0), digits("00012345678906")),
                       ((20, 500, 119, 539, 5, 6, 40, 3), digits("123456")), ((20, 600, 119, 639, 2, 13, 40, 0), digits("4006381333932")))
    found = bc.read_barcodes(rows, syms)
    assert [(f["kind"], f["content"], f["reversed"], f["vertical"], f.get("itf14", False)) for f in found] == [
        ("EAN13", "4006381333931", False, False, False), ("UPCA", "036000291452", True, False, False), ("EAN8", "96385074", False, True, False),
        ("UPCE", "01234565", False, False, False), ("ITF", "00012345678905", False, False, True), ("ITF", "00012345678906", False, False, False),
        ("ITF", "123456", True, True, False)]                                                          # the failing EAN-13 is left out
    assert found[0]["polygon"] == [100.0, 200.0, 290.0, 200.0, 290.0, 250.0, 100.0, 250.0] and found[0]["confidence"] == 1.0
    assert found[1]["confidence"] == 0.5 and found[2]["confidence"] == 1.0
    boxes = layout.build_barcode_boxes(found, 3)
    assert boxes[0] == {"type": "barcode", "kind": "EAN13", "content": "4006381333931", "confidence": 1.0, "polygon": found[0]["polygon"], "page_number": 3}
    assert boxes[4]["itf14"] is True and "itf14" not in boxes[5] and "itf14" not in boxes[0]
    assert layout.validate_layout_boxes(boxes) == [] and {b["kind"] for b in boxes} == {"EAN13", "UPCA", "EAN8", "UPCE", "ITF"}
    assert layout.validate_layout_boxes([dict(boxes[0], kind="EAN")]) != []


def test_markdown_line_and_the_digits_below_a_strip_stay():
    lines = [_line(50, 20, 400, 50, "Invoice 17"), _line(100, 252, 290, 270, "4 006381 333931"), _line(50, 300, 400, 330, "Total 12.00")]
    merged, _ = layout.reading_order(lines)
    found = bc.read_barcodes(*_rows(((100, 200, 289, 249, 2, 13, 50, 0), digits("4006381333931"))))
    assert layout.page_markdown(merged, barcodes=found) == "Invoice 17\n:barcode: 4006381333931\n4 006381 333931\nTotal 12.00"
    on_it = _line(110, 205, 280, 245, "|||l1")
    assert [bc.inside_any(t[0], found) for t in (on_it, lines[1])] == [True, False]                  # the human-readable digits lie outside the hull


def test_kind_names():
    assert arch.BARCODE_KINDS == dict(code128=1, code39=2, ean13=4, ean8=8, upce=16, itf=32)
    assert [arch.BARCODE_KINDS[k.lower()] for k in bc.KINDS] == [1 << i for i in range(6)]           # name k is bit k is device kind k
    assert arch.barcode_kinds_mask(arch.BARCODE_KINDS_DEFAULT) == 3 and arch.barcode_kinds_mask("all") == 63
    assert arch.barcode_kinds_mask("ean13, ITF") == 36 and arch.barcode_kinds_mask(["upce"]) == 16 and arch.barcode_kinds_mask("code128,all") == 63
    for bad in ("", ",", "ean", "ean13,codabar", ["upca"]):
        with pytest.raises(ValueError):
            arch.barcode_kinds_mask(bad)
    assert arch.BARCODE_PARAMS == dict(threshold=arch.MARK_PARAMS["threshold"], quiet=5, max_dist=24, min_rows=8, row_gap=2, max_codes=64)


class NoEngine:
    num_classes, cls_loaded = 6625, False

    def __init__(self):
        self.calls = []

    def barcodes(self, *a, **kw):
        self.calls.append(kw)


def test_pipeline_option_and_its_default():
    e = NoEngine()
    assert OcrPipeline(e, barcodes=True).barcode_kinds == 3 and OcrPipeline(e).barcode_kinds == 3
    OcrPipeline(e, barcodes=True)._submit_barcodes(None)
    OcrPipeline(e, barcodes=True, barcode_kinds=("code39", "code128"))._submit_barcodes(None)
    OcrPipeline(e, barcodes=True, barcode_kinds="all")._submit_barcodes(None)
    OcrPipeline(e, barcodes=True, barcode_kinds=("ean13",))._submit_barcodes(None)
    assert [c["kinds"] for c in e.calls] == [None, None, 63, 4]                                      # the default kinds go through the old entry
    assert OcrPipeline(e, barcode_kinds="all")._submit_barcodes(None) is None                        # without barcodes the kinds do nothing
    with pytest.raises(ValueError, match="codabar"):
        OcrPipeline(e, barcodes=True, barcode_kinds=("codabar",))


def test_provider_variable(monkeypatch):
    from PIL import Image
    for var in ("LUMINA_OCR_BARCODES", "LUMINA_OCR_BARCODE_KINDS"):
        monkeypatch.delenv(var, raising=False)
    s = _service()
    assert s._use_barcodes is False and s._barcode_kinds == "code128,code39" and s.get_status()["barcode_kinds"] == []
    monkeypatch.setenv("LUMINA_OCR_BARCODES", "1")
    assert _service().get_status()["barcode_kinds"] == ["code128", "code39"]
    monkeypatch.setenv("LUMINA_OCR_BARCODE_KINDS", "all")
    assert _service().get_status()["barcode_kinds"] == ["code128", "code39", "ean13", "ean8", "upce", "itf"]
    monkeypatch.setenv("LUMINA_OCR_BARCODE_KINDS", "itf, EAN13")
    assert _service().get_status()["barcode_kinds"] == ["ean13", "itf"]
    monkeypatch.setenv("LUMINA_OCR_BARCODE_KINDS", "ean13,codabar")
    monkeypatch.setenv("LUMINA_OCR_ALLOW_SYNTHETIC", "1")
    r = _service().process_image_sync(Image.new("RGB", (64, 48), (255, 255, 255)))
    assert not r.success and "LUMINA_OCR_BARCODE_KINDS" in r.error and "codabar" in r.error           # errors are data; no engine was built for it
    monkeypatch.setenv("LUMINA_OCR_BARCODES", "0")                                                    # alone the variable has no effect
    assert _service().get_status()["barcode_kinds"] == [] and _service()._use_barcodes is False


def test_finish_page_with_the_new_kinds():
    s = _service()
    quads = np.array([q(150, 52), q(195, 225), q(150, 300)], np.int32)
    rows, syms = _rows(((100, 200, 289, 249, 2, 13, 50, 0), digits("0036000291452")), ((400, 200, 611, 249, 5, 14, 50, 4), digits("00012345678905")))
    d = PageDetections(quads, ["Invoice", "|||1l", "Total"], np.array([0.9, 0.8, 0.7], np.float32), np.ones(3, np.float32), 1000, 700,
                       barcodes=rows, barcode_syms=syms)
    out = s._finish_page(d, b"jpeg", (700, 1000), 1, (1000, 700), 0.0)
    codes = [b for b in out.layout_boxes if b["type"] == "barcode"]
    assert [(b["kind"], b["content"], b.get("itf14")) for b in codes] == [("UPCA", "036000291452", None), ("ITF", "00012345678905", True)]
    assert out.json_output["barcodes_count"] == 2 and layout.validate_layout_boxes(out.layout_boxes) == []
    assert out.markdown == "Invoice\n:barcode: 036000291452\n:barcode: 00012345678905\nTotal"       # the line on the strip is dropped
