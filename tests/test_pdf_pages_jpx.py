"""CPU: utils/pdf_pages.read_pages(..., jpx=True) finds the /JPXDecode page images of hand-assembled scanned PDFs (opt-in, like
strip_filters); with jpx=False they are refused as before; /SMaskInData, a colour space outside DeviceGray / DeviceRGB and a size that
disagrees with the codestream are refused."""
import pytest

import jp2_cases as jc
import pdf_cases as pc
from lumina_ocr.utils import pdf_pages

W, H = 130, 100


def jpx_obj(data, width=W, height=H, cs="/DeviceRGB", extra=""):
    e = "/Type /XObject /Subtype /Image /Width %d /Height %d %s /BitsPerComponent 8 /Filter /JPXDecode %s" % (
        width, height, ("/ColorSpace " + cs) if cs else "", extra)
    return pc.stream_obj(e, data)


@pytest.fixture(scope="module")
def files():
    return {
        "rgb": jc.write(jc.content("page", H, W, "RGB", 1), irreversible=False),
        "grey": jc.write(jc.content("page", H, W, "L", 2), irreversible=False),
        "raw": jc.write(jc.content("page", H, W, "RGB", 3), irreversible=False, no_jp2=True),
    }


def test_one_page(files):
    pdf = pc.document([{"image": jpx_obj(files["rgb"]), "box": (468, 360)}])
    (e,) = pdf_pages.read_pages(pdf, jpx=True)
    assert isinstance(e, pdf_pages.PageImage), e
    assert (e.filter, e.width, e.height, e.rotate, e.params) == ("JPXDecode", W, H, 0, {"components": 3})
    assert bytes(e.stream) == files["rgb"]


def test_three_pages_and_container_forms(files):
    pages = [{"image": jpx_obj(files["rgb"]), "box": (468, 360)},
             {"image": jpx_obj(files["grey"], cs="/DeviceGray"), "box": (468, 360), "attrs": "/Rotate 90"},
             {"image": jpx_obj(files["raw"], cs=""), "box": (468, 360)}]   # no /ColorSpace: the codestream's own
    for kw in ({}, {"xref": "stream", "objstm": True}):
        got = pdf_pages.read_pages(pc.document(pages, **kw), jpx=True)
        assert all(isinstance(e, pdf_pages.PageImage) for e in got), got
        assert [(e.filter, e.params["components"], e.rotate) for e in got] == [("JPXDecode", 3, 0), ("JPXDecode", 1, 90), ("JPXDecode", 3, 0)]
        assert [bytes(e.stream) for e in got] == [files["rgb"], files["grey"], files["raw"]]


def test_refused_without_the_option(files):
    pdf = pc.document([{"image": jpx_obj(files["rgb"]), "box": (468, 360)}])
    for got in (pdf_pages.read_pages(pdf), pdf_pages.read_pages(pdf, jpx=False), pdf_pages.read_pages(pdf, strip_filters=True)):
        assert isinstance(got[0], pdf_pages.PdfRefused) and got[0].reason == "image filter JPXDecode"


@pytest.mark.parametrize("what,word", [("smask_in_data", "SMaskInData"), ("width", "dictionary says"), ("height", "dictionary says"),
                                       ("cs_cmyk", "ColorSpace"), ("cs_mismatch", "components"), ("smask", "/SMask"), ("mask", "/Mask"),
                                       ("decode", "/Decode"), ("not_jp2", "SOC"), ("image_mask", "/ImageMask")])
def test_refusals(files, what, word):
    obj = {
        "smask_in_data": lambda: jpx_obj(files["rgb"], extra="/SMaskInData 1"),
        "width": lambda: jpx_obj(files["rgb"], width=W + 1),
        "height": lambda: jpx_obj(files["rgb"], height=H - 1),
        "cs_cmyk": lambda: jpx_obj(files["rgb"], cs="/DeviceCMYK"),
        "cs_mismatch": lambda: jpx_obj(files["grey"], cs="/DeviceRGB"),
        "smask": lambda: jpx_obj(files["rgb"], extra="/SMask 1 0 R"),
        "mask": lambda: jpx_obj(files["rgb"], extra="/Mask [0 0 0 0 0 0]"),
        "decode": lambda: jpx_obj(files["rgb"], extra="/Decode [1 0 1 0 1 0]"),
        "not_jp2": lambda: jpx_obj(b"\x00" * 64),
        "image_mask": lambda: jpx_obj(files["grey"], cs="", extra="/ImageMask true"),
    }[what]()
    (e,) = pdf_pages.read_pages(pc.document([{"image": obj, "box": (468, 360)}]), jpx=True)
    assert isinstance(e, pdf_pages.PdfRefused) and word in e.reason, e


def test_smask_in_data_zero_is_taken(files):
    (e,) = pdf_pages.read_pages(pc.document([{"image": jpx_obj(files["rgb"], extra="/SMaskInData 0"), "box": (468, 360)}]), jpx=True)
    assert isinstance(e, pdf_pages.PageImage)


def test_other_filters_unchanged_with_the_option(files):
    """jpx=True changes nothing for a page of another filter"""
    import zlib
    import numpy as np
    rows = np.zeros((4, 6), np.uint8)
    img = pc.image_obj(6, 4, "/FlateDecode", zlib.compress(rows.tobytes()))
    pdf = pc.document([{"image": img, "box": (60, 40)}])
    a, b = pdf_pages.read_pages(pdf)[0], pdf_pages.read_pages(pdf, jpx=True)[0]
    assert isinstance(a, pdf_pages.PageImage) and (a.filter, a.params, a.width, a.height) == (b.filter, b.params, b.width, b.height)
