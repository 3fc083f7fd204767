"""CPU: utils/pdf_pages.py, the host reader that finds the page images of scanned PDFs.  Pillow-written files, the test-side writer
(tests/pdf_cases.py) for what Pillow never writes, each refusal reason, and damaged files: the only acceptable outcomes are PdfRefused
or valid records, promptly."""
import io
import time
import zlib

import numpy as np
import pytest
from PIL import Image, features

import pdf_cases as pc
from lumina_ocr.utils import pdf_pages as pp


def _pil_pdf(images, **kw) -> bytes:
    op = io.BytesIO()
    images[0].save(op, "PDF", save_all=len(images) > 1, append_images=images[1:], **kw)
    return op.getvalue()


def _rgb(h=40, w=30, seed=0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _gray_flate_page(w=31, h=17, pred_parms="", data=None, **kw):
    g = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    data = zlib.compress(g.tobytes()) if data is None else data
    return g, {"image": pc.image_obj(w, h, "/FlateDecode", data, parms=pred_parms, **kw), "box": (w * 2, h * 2)}


def _ok(entry) -> pp.PageImage:
    assert isinstance(entry, pp.PageImage), getattr(entry, "reason", entry)
    return entry


# ---- Pillow-written files ----
def test_pillow_rgb_and_gray_pages_are_dct():
    for mode, comps in (("RGB", 3), ("L", 1)):
        im = Image.fromarray(_rgb()).convert(mode)
        data = _pil_pdf([im])
        (page,) = pp.read_pages(data)
        page = _ok(page)
        assert (page.filter, page.width, page.height, page.rotate, page.params["components"]) == ("DCTDecode", 30, 40, 0, comps)
        assert isinstance(page.stream, memoryview) and bytes(page.stream[:2]) == b"\xff\xd8"
        embedded = Image.open(io.BytesIO(page.stream))
        assert embedded.format == "JPEG" and embedded.size == (30, 40) and embedded.mode == mode


@pytest.mark.skipif(not features.check("libtiff"), reason="Pillow writes mode-1 pages as Group 4 through libtiff")
def test_pillow_bilevel_page_is_group4():
    import ccitt_reference as cr
    bm = np.random.default_rng(5).random((33, 70)) < 0.4
    im = Image.fromarray(np.where(bm, 0, 255).astype(np.uint8)).convert("1")
    (page,) = pp.read_pages(_pil_pdf([im]))
    page = _ok(page)
    assert (page.filter, page.width, page.height) == ("CCITTFaxDecode", 70, 33)
    assert page.params == {"K": -1, "EncodedByteAlign": False, "BlackIs1": True, "invert": False}
    status, bits = cr.decode(page.stream, 70, 33, black_is_1=True)   # (Pillow leaves the TIFF's directory after the data)
    assert status == 0 and np.array_equal(bits == 0, bm)


def test_pillow_multi_page_with_resolution():
    ims = [Image.fromarray(_rgb(50 + 10 * k, 40, k)) for k in range(3)]
    pages = pp.read_pages(_pil_pdf(ims, resolution=200.0))
    assert [(p.width, p.height) for p in map(_ok, pages)] == [(40, 50), (40, 60), (40, 70)]
    assert pages[0].media_box[2] == pytest.approx(40 * 72 / 200) and pages[2].media_box[3] == pytest.approx(70 * 72 / 200)


# ---- the test-side writer: what Pillow never writes ----
@pytest.mark.parametrize("xref,objstm", [("table", False), ("stream", False), ("stream", True)])
def test_flate_predictors_through_each_container(xref, objstm):
    w, h = 31, 17
    g = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    rgb = _rgb(h, w, 4)
    pages = [
        {"image": pc.image_obj(w, h, "/FlateDecode", zlib.compress(g.tobytes())), "box": (w, h)},
        {"image": pc.image_obj(w, h, "[/FlateDecode]", zlib.compress(pc.tiff_predict_rows(rgb.reshape(h, -1), 3)), cs="/DeviceRGB",
                               parms="[<< /Predictor 2 /Colors 3 /BitsPerComponent 8 /Columns %d >>]" % w), "box": (w, h), "deflate_content": True},
        {"image": pc.image_obj(w, h, "/FlateDecode", zlib.compress(pc.png_filter_rows(g, 1, [0, 1, 2, 3, 4])),
                               parms="<< /Predictor 15 /Columns %d >>" % w), "box": (w, h)},
    ]
    got = [_ok(p) for p in pp.read_pages(pc.document(pages, xref=xref, objstm=objstm))]
    assert [p.params["predictor"] for p in got] == [1, 2, 15]
    assert [(p.params["components"], p.params["bits"], p.params["indexed"], p.params["invert"]) for p in got] == [(1, 8, False, False), (3, 8, False, False), (1, 8, False, False)]
    assert zlib.decompress(got[0].stream) == g.tobytes()
    assert all(p.filter == "FlateDecode" and (p.width, p.height) == (w, h) for p in got)


def test_inherited_rotate_mediabox_and_resources():
    g, page = _gray_flate_page()
    page["media"] = False
    data = pc.document([page, dict(page, attrs="/Rotate 270")], tree_attrs="/Rotate 90 /MediaBox [0 0 62 34]")
    a, b = (_ok(p) for p in pp.read_pages(data))
    assert (a.rotate, b.rotate) == (90, 270) and a.media_box == (0.0, 0.0, 62.0, 34.0)


def test_indexed_colour_string_and_stream_lookup():
    w, h = 20, 9
    idx = np.random.default_rng(8).integers(0, 16, (h, w))
    lut = np.random.default_rng(9).integers(0, 256, (16, 3), dtype=np.uint8)
    packed = zlib.compress(pc.pack_bits(idx, 4).tobytes())
    hexlut = "<" + lut.tobytes().hex() + ">"
    p1 = _ok(pp.read_pages(pc.document([{"image": pc.image_obj(w, h, "/FlateDecode", packed, cs="[/Indexed /DeviceRGB 15 %s]" % hexlut, bits=4), "box": (w, h)}]))[0])
    assert (p1.params["components"], p1.params["bits"], p1.params["indexed"]) == (1, 4, True)
    pal = np.frombuffer(p1.params["palette"], np.uint8).reshape(256, 3)
    assert np.array_equal(pal[:16], lut) and np.array_equal(pal[16:], np.repeat(lut[15:16], 240, axis=0))
    # grey base, the lookup in a (deflated) stream: serialize() by hand to add the lookup object
    glut = np.arange(0, 256, 17, dtype=np.uint8)[::-1].copy()
    objs = {1: b"<< /Type /Catalog /Pages 2 0 R >>", 2: b"<< /Type /Pages /Count 1 /Kids [3 0 R] >>",
            3: b"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 20 9] /Resources << /XObject << /Im0 5 0 R >> >> /Contents 4 0 R >>",
            4: pc.stream_obj("", pc.page_content(w, h)),
            5: pc.image_obj(w, h, "/FlateDecode", packed, cs="[/Indexed /DeviceGray 15 6 0 R]", bits=4),
            6: pc.stream_obj("/Filter /FlateDecode", zlib.compress(glut.tobytes()))}
    p2 = _ok(pp.read_pages(pc.serialize(objs))[0])
    assert np.array_equal(np.frombuffer(p2.params["palette"], np.uint8).reshape(256, 3)[:16], np.repeat(glut[:, None], 3, axis=1))


def test_decode_inversion_and_icc_based():
    g, page = _gray_flate_page(extra="/Decode [1 0]")
    assert _ok(pp.read_pages(pc.document([page]))[0]).params["invert"] is True
    g, page = _gray_flate_page(extra="/Decode [0 1]")
    assert _ok(pp.read_pages(pc.document([page]))[0]).params["invert"] is False
    # ICCBased N = 3 is read as DeviceRGB
    rgb = _rgb(9, 20, 2)
    objs = {1: b"<< /Type /Catalog /Pages 2 0 R >>", 2: b"<< /Type /Pages /Count 1 /Kids [3 0 R] >>",
            3: b"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 20 9] /Resources << /XObject << /Im0 5 0 R >> >> /Contents 4 0 R >>",
            4: pc.stream_obj("", pc.page_content(20, 9)),
            5: pc.image_obj(20, 9, "/FlateDecode", zlib.compress(rgb.tobytes()), cs="[/ICCBased 6 0 R]"),
            6: pc.stream_obj("/N 3", b"not a real profile")}
    assert _ok(pp.read_pages(pc.serialize(objs))[0]).params["components"] == 3
    objs[6] = pc.stream_obj("/N 4", b"cmyk")
    assert "ICCBased" in pp.read_pages(pc.serialize(objs))[0].reason


def test_prev_chain_newest_definition_wins():
    g, page = _gray_flate_page()
    objs_doc = pc.document([page])
    assert _ok(pp.read_pages(objs_doc)[0]).rotate == 0
    # the same document, its page object replaced in an incremental update (object 3 is the first page)
    new_page = b"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 62 34] /Rotate 180 /Resources << /XObject << /Im0 5 0 R >> >> /Contents 4 0 R >>"
    base = {1: b"<< /Type /Catalog /Pages 2 0 R >>", 2: b"<< /Type /Pages /Count 1 /Kids [3 0 R] >>",
            3: new_page.replace(b"/Rotate 180", b"/Rotate 90"), 4: pc.stream_obj("", pc.page_content(62, 34)), 5: page["image"]}
    data = pc.serialize(base, updates={3: new_page})
    assert data.count(b"startxref") == 2 and b"/Prev" in data
    assert _ok(pp.read_pages(data)[0]).rotate == 180


def test_prev_loop_and_page_tree_cycle_end():
    g, page = _gray_flate_page()
    data = pc.document([page])
    at = int(data[data.rindex(b"startxref") + 9:].split()[0])
    looped = data.replace(b"/Root 1 0 R", b"/Root 1 0 R /Prev %d" % at)
    looped = looped[:looped.rindex(b"startxref")] + b"startxref\n%d\n%%%%EOF\n" % at
    assert isinstance(pp.read_pages(looped)[0], pp.PageImage)   # the section is read once
    cyc = {1: b"<< /Type /Catalog /Pages 2 0 R >>", 2: b"<< /Type /Pages /Count 1 /Kids [3 0 R] >>", 3: b"<< /Type /Pages /Count 1 /Kids [2 0 R] >>"}
    with pytest.raises(pp.PdfRefused, match="cycle"):
        pp.read_pages(pc.serialize(cyc))
    loop = {1: b"<< /Type /Catalog /Pages 2 0 R >>", 2: b"<< /Type /Pages /Count 1 /Kids 3 0 R >>", 3: b"4 0 R", 4: b"3 0 R"}
    with pytest.raises(pp.PdfRefused, match="loop"):
        pp.read_pages(pc.serialize(loop))


# ---- refusals ----
def _reason(pages_or_data) -> str:
    entry = pp.read_pages(pages_or_data if isinstance(pages_or_data, bytes) else pc.document(pages_or_data))[0]
    assert isinstance(entry, pp.PdfRefused)
    return entry.reason


def test_each_refusal_reason():
    g, page = _gray_flate_page()
    w, h = page["box"]
    assert "text" in _reason([dict(page, content=b"BT /F1 12 Tf 10 10 Td (hello) Tj ET")])
    assert "text" in _reason([dict(page, content=pc.page_content(w, h) + b"\nBT (x) Tj ET")])
    assert "several images" in _reason([dict(page, image=[page["image"], page["image"]])])
    assert "axis-aligned" in _reason([dict(page, cm="%g 3 -3 %g 0 0" % (w, h))])
    assert "axis-aligned" in _reason([dict(page, cm="%g 0 0 %g 0 %g" % (w, -h, h))])          # mirrored
    assert "cover" in _reason([dict(page, cm="%g 0 0 %g 0 0" % (w * 0.9, h))])
    assert "cover" in _reason([dict(page, cm="%g 0 0 %g 2 0" % (w, h))])                      # shifted by 3 % of the width
    assert isinstance(pp.read_pages(pc.document([dict(page, cm="%g 0 0 %g 0.3 0" % (w, h))]))[0], pp.PageImage)   # 0.5 %: within 1 %
    assert "inline" in _reason([dict(page, content=b"q 62 0 0 34 0 0 cm BI /W 1 /H 1 /BPC 8 /CS /G ID \x00 EI Q")])
    assert "clipping" in _reason([dict(page, content=b"W n\n" + pc.page_content(w, h))])
    assert "operator" in _reason([dict(page, content=b"0 0 10 10 re f\n" + pc.page_content(w, h))])
    assert "SMask" in _reason([_gray_flate_page(extra="/SMask 1 0 R")[1]])
    assert "ImageMask" in _reason([_gray_flate_page(extra="/ImageMask true")[1]])
    chain = pc.image_obj(31, 17, "[/ASCIIHexDecode /FlateDecode]", b"00>")
    assert "filter chain" in _reason([dict(page, image=chain)])
    assert "filter" in _reason([dict(page, image=pc.image_obj(31, 17, "/LZWDecode", b"\x80"))])
    assert "Decode" in _reason([_gray_flate_page(extra="/Decode [0.2 0.8]")[1]])
    assert "colour space" in _reason([_gray_flate_page(cs="/DeviceCMYK")[1]])
    assert "bits" in _reason([_gray_flate_page(bits=16)[1]])
    assert "predictor" in _reason([_gray_flate_page(pred_parms="<< /Predictor 12 /Columns 30 >>")[1]])
    with pytest.raises(pp.PdfRefused, match="Encrypt"):
        pp.read_pages(pc.document([page], trailer_extra="/Encrypt << /Filter /Standard >>"))
    for junk in (b"", b"hello", b"%PDF-1.4\n", b"%PDF-1.4\nstartxref\n999999\n%%EOF"):
        with pytest.raises(pp.PdfRefused):
            pp.read_pages(junk)


def test_a_refused_page_does_not_refuse_its_neighbours():
    g, page = _gray_flate_page()
    got = pp.read_pages(pc.document([page, dict(page, content=b"BT (x) Tj ET"), page]))
    assert [isinstance(p, pp.PageImage) for p in got] == [True, False, True]


def test_stream_length_is_checked_against_the_file():
    g, page = _gray_flate_page()
    k = page["image"].index(b"/Length")
    body = page["image"][:k] + b"/Length 99999999" + page["image"][page["image"].index(b" >>", k):]
    bad = pc.document([dict(page, image=body)])
    entry = pp.read_pages(bad)[0]
    assert isinstance(entry, pp.PdfRefused) and "Length" in entry.reason


# ---- damaged files ----
def _three_files():
    g, page = _gray_flate_page()
    files = [pc.document([page, page], xref="stream", objstm=True), pc.document([page], tree_attrs="/Rotate 90"),
             _pil_pdf([Image.fromarray(_rgb(20, 16, 1)), Image.fromarray(_rgb(20, 16, 2))])]
    return files


def _outcome_is_valid(data: bytes) -> float:
    t0 = time.perf_counter()
    try:
        for entry in pp.read_pages(data):
            if isinstance(entry, pp.PageImage):
                assert entry.filter in pp.FILTERS and 0 < entry.width <= 65535 and 0 < entry.height <= 65535
                assert entry.rotate in (0, 90, 180, 270) and len(entry.stream) <= len(data)
            else:
                assert isinstance(entry, pp.PdfRefused) and entry.reason
    except pp.PdfRefused as e:
        assert e.reason
    return time.perf_counter() - t0


def test_truncations_at_every_97th_byte():
    for data in _three_files():
        for cut in range(0, len(data), 97):
            assert _outcome_is_valid(data[:cut]) < 1.0


def test_seeded_byte_flips():
    rng = np.random.default_rng(2024)
    for data in _three_files():
        for _ in range(150):
            buf = bytearray(data)
            for at in rng.integers(0, len(buf), int(rng.integers(1, 6))):
                buf[at] = int(rng.integers(0, 256))
            assert _outcome_is_valid(bytes(buf)) < 1.0
