"""CPU: the layered-page reader (utils/pdf_pages.py read_pages(layers=True)) and the restatement of lumina_ocr_page_compose
(pdf_layers_reference.py): strips, a stencil over a background, /SMask, a /Mask stream, invisible text, the refusals, and damage."""
import functools

import numpy as np
import pytest

import pdf_cases as pc
import pdf_layer_cases as lc
import pdf_layers_reference as lr
from lumina_ocr.utils import pdf_pages as pp

BOX = lc.BOX


@functools.lru_cache(maxsize=None)
def _page():
    return lc.source_page()


def _read(page_dicts, **kw):
    return pp.read_pages(pc.document(page_dicts if isinstance(page_dicts, list) else [page_dicts]), layers=True, **kw)


def _one(page_dict, **kw):
    (e,) = _read(page_dict, **kw)
    assert not isinstance(e, pp.PdfRefused), e.reason
    return e


def _reason(page_dict, **kw) -> str:
    (e,) = _read(page_dict, **kw)
    assert isinstance(e, pp.PdfRefused), e
    return e.reason


# ---- strips ----
CUTS = {2: [413], 3: [1, 640], 7: [90, 91, 333, 500, 777, 998]}   # unequal bands, 1-row bands among them


@pytest.mark.parametrize("bands", [2, 3, 7])
def test_strips_give_the_source_bitmap_in_either_paint_order(bands):
    page = _page()
    bitmaps = []
    for reverse in (False, True):
        d, want = lc.strips_page(page, CUTS[bands], ["rgb", "gray", "g4"], reverse=reverse)
        e = _one(d)
        assert isinstance(e, pp.PageLayers) and (e.width, e.height) == (lc.W, lc.H) and len(e.layers) == bands
        assert all(l.kind == 0 and l.rect[0] == 0 and l.rect[2] == lc.W for l in e.layers)
        assert sorted((l.rect[1], l.rect[3]) for l in e.layers) == list(zip([0] + CUTS[bands], CUTS[bands] + [lc.H]))
        assert {l.image.filter for l in e.layers} == {"FlateDecode", "CCITTFaxDecode"} if bands > 2 else True
        assert lr.compose_params_ok(lc.layer_table(e, decode=lambda r: np.zeros((r.height, r.width, 3), np.uint8)), 1, e.height, e.width)
        got = lc.render(e)
        assert np.array_equal(got, want)
        bitmaps.append(got)
    assert np.array_equal(bitmaps[0], bitmaps[1])


# ---- mixed raster content ----
@pytest.mark.parametrize("decode, g4", [("", False), ("[0 1]", False), ("[1 0]", False), ("", True)])
def test_stencil_over_a_background(decode, g4):
    d, want = lc.mixed_raster_page(decode, g4)
    e = _one(d)
    assert isinstance(e, pp.PageLayers) and (e.width, e.height) == (699, 1002)
    bg, st = e.layers
    assert (bg.kind, bg.rect, st.kind, st.rect, st.fill, st.flip) == (0, (0, 0, 699, 1002), 1, (0, 0, 699, 1002), lc.FILL8, int(decode == "[1 0]"))
    assert (bg.image.width, bg.image.height, st.mask.width, st.mask.height) == (233, 334, 699, 1002) and st.image is None
    assert st.mask.params["invert"] is False
    assert np.array_equal(lc.render(e), want)


def _blend(src, a, dst):
    """round(src a / 255 + dst (255 - a) / 255) in Python integers: the nearest integer to t / 255 (t / 255 is never at a half)"""
    out = np.empty(src.shape, np.uint8)
    for idx in np.ndindex(*src.shape):
        t = int(src[idx]) * int(a[idx[:2]]) + int(dst[idx]) * (255 - int(a[idx[:2]]))
        out[idx] = (2 * t + 255) // 510
    return out


@pytest.mark.parametrize("one_bit, decode", [(False, ""), (False, "[1 0]"), (True, ""), (True, "[1 0]")])
def test_soft_mask(one_bit, decode):
    d, bg, fg, alpha = lc.smask_page(5, one_bit, decode)
    e = _one(d)
    assert isinstance(e, pp.PageLayers) and (e.width, e.height) == (699, 1002) and [l.kind for l in e.layers] == [0, 2]
    top = e.layers[1]
    assert (top.image.width, top.mask.width, top.flip, top.mask.params["invert"]) == (233, 699, int(decode == "[1 0]"), False)
    got = lc.render(e)
    a = (255 - alpha.astype(np.int64)) if decode == "[1 0]" else alpha.astype(np.int64)
    up = np.repeat(np.repeat(fg, 3, axis=0), 3, axis=1)
    if one_bit:
        want = np.where(a[:, :, None] == 255, up, bg)
    else:
        assert set(np.unique(a)) == set(lc.ALPHAS)
        t = up.astype(np.int64) * a[:, :, None] + bg.astype(np.int64) * (255 - a[:, :, None])
        want = ((2 * t + 255) // 510).astype(np.uint8)   # the nearest integer to t / 255, all of them
        rows = slice(0, 14)                               # ... and in Python integers, pixel by pixel, on rows that hold every alpha
        assert np.array_equal(_blend(up[rows, :60], a[rows, :60], bg[rows, :60]), want[rows, :60])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("decode", ["", "[1 0]"])
def test_explicit_mask(decode):
    d, want = lc.mask_page(5, decode)
    e = _one(d)
    assert [l.kind for l in e.layers] == [0, 3] and e.layers[1].flip == int(decode == "[1 0]")
    assert np.array_equal(lc.render(e), want)


def test_div255_is_rounding_for_every_product():
    t = np.arange(255 * 255 + 1, dtype=np.int64)
    assert np.array_equal(lr.div255(t), (2 * t + 255) // 510)


# ---- sampling ----
def test_non_integer_scale_equals_the_per_pixel_formula():
    rng = np.random.default_rng(5)
    src, mask, under = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((9, 23, 3), (31, 40, 3), (13, 67, 3)))
    layers = [(0, 0, (0, 0, 67, 13), 0, (0, 0, 0), under, None),
              (0, 0, (0, 2, 67, 31), 0, (0, 0, 0), src, None),            # 23 samples over 67 columns, 9 over 29 rows
              (0, 2, (-5, -3, 80, 20), 1, (0, 0, 0), src, mask),
              (0, 1, (3, 1, 50, 12), 0, (9, 8, 7), None, mask),
              (0, 3, (10, 5, 67, 40), 0, (0, 0, 0), src, mask)]
    got = lr.compose((37, 67), 1, layers)[0]
    for y in range(37):
        for x in range(67):
            c = (255, 255, 255)
            for l in layers:
                c = lr.compose_pixel(c, l, x, y)
            assert tuple(got[y, x]) == c, (x, y)
    assert [lr.sample_map(d, 67, 23) for d in (0, 1, 2, 3, 66)] == [0, 0, 0, 1, 22]


# ---- invisible text ----
def test_invisible_text_over_one_image_is_todays_record():
    page = _page()
    img = lc.rgb_obj(page)
    plain = pp.read_pages(pc.document([{"image": img, "box": BOX}]))[0]
    text = b"\nBT /F1 12 Tf 3 Tr 1 0 0 1 20 300 Tm (poor embedded text) Tj [(a) -20 (b)] TJ T* (c) ' ET"
    e = _one({"image": img, "box": BOX, "content": pc.page_content(*BOX) + text})
    assert isinstance(e, pp.PageImage)
    assert (e.filter, bytes(e.stream), e.params, e.width, e.height, e.rotate, e.media_box) == (
        plain.filter, bytes(plain.stream), plain.params, plain.width, plain.height, plain.rotate, plain.media_box)
    # marked content around it, and Tr set before BT
    e = _one({"image": img, "box": BOX, "content": b"/Artifact BMC 3 Tr " + pc.page_content(*BOX) + b" EMC /OC /MC0 BDC BT (x) Tj ET EMC"})
    assert isinstance(e, pp.PageImage)


@pytest.mark.parametrize("text", [b"BT 0 Tr (seen) Tj ET", b"q 3 Tr Q BT (seen) Tj ET", b"BT (seen) Tj 3 Tr ET", b"BT 3 Tr ET (outside) Tj"])
def test_visible_text_is_refused(text):
    img = lc.gray_obj(_page()[:40, :30, 0].copy())
    assert "text operators on the page (Tj)" == _reason({"image": img, "box": BOX, "content": pc.page_content(*BOX) + b"\n" + text})


# ---- refusals ----
def _strips(content=None, **kw):
    d, _ = lc.strips_page(_page()[:60, :50], [20], ["gray"])
    if content is not None:
        d["content"] = content(d["content"]) if callable(content) else content
    d.update(kw)
    return d


def test_each_refusal_reason():
    small = _page()[:60, :50]
    gray = lc.gray_obj(small[:, :, 0].copy())
    bits = (small[:, :, 0] >= 128).astype(np.uint8)
    assert "axis-aligned" in _reason(_strips(lambda c: c.replace(b"cm /Im1", b"cm 1 0 0 -1 0 1 cm /Im1")))                     # a flipped cm
    assert _reason(_strips(lambda c: b"/GS0 gs\n" + c)) == "ExtGState GS0 not found"
    assert "content operator 'k'" == _reason(_strips(lambda c: b"0 0 0 1 k\n" + c))
    assert "content operator 're'" == _reason(_strips(lambda c: b"0 0 10 10 re f\n" + c))
    assert "clipping" in _reason(_strips(lambda c: b"W n\n" + c))
    assert "fill colour space" in _reason(_strips(lambda c: b"/DeviceCMYK cs\n" + c))
    assert "malformed fill colour" == _reason(_strips(lambda c: b"1.5 g\n" + c))
    # 64 layers pass, 65 do not
    many = lambda n: {"image": [gray], "box": BOX, "content": b"\n".join(lc.place("Im0", BOX) for _ in range(n))}
    assert len(_one(many(64)).layers) == 64
    assert _reason(many(65)) == "more than 64 images on the page"
    # a hull that leaves a fifth of the box bare
    assert "do not cover the MediaBox" in _reason({"image": [gray, gray], "box": BOX, "content": lc.place("Im0", BOX, y0=216) + lc.place("Im1", BOX, y0=72, y1=216)})
    # a canvas over the cap: 65535 x 1100 samples; and a side above 65535
    wide = pc.image_obj(65535, 1100, "/FlateDecode", b"", extra="")
    assert "above the cap" in _reason({"image": [wide, gray], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX)})
    assert "canvas of" in _reason({"image": [gray, gray], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX, x1=0.1, y1=0.1)})
    # masks
    assert "stencil with 8 bits" in _reason({"image": [gray, lc.stencil_obj(bits, bpc=8)], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX)})
    d, *_ = lc.smask_page(5, False, mask_extra=" /Matte [1 1 1]")
    assert _reason(d) == "/Matte"
    d, _ = lc.mask_page(5, mask="[0 10 0 10 0 10]")
    assert _reason(d) == "colour-key /Mask"
    d, *_ = lc.smask_page(5, False, mask_extra=" /SMask 7 0 R")
    assert _reason(d) == "/SMask on a mask"
    two = {"image": [gray, lc.stencil_obj(bits, extra="/SMask 5 0 R")], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX)}
    assert _reason(two) == "/SMask on a stencil"
    sid = {"image": [gray, lc.gray_obj(small[:, :, 0].copy(), extra="/SMaskInData 1")], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX)}
    assert _reason(sid) == "/SMaskInData 1"
    assert "/Decode" in _reason({"image": [gray, lc.stencil_obj(bits, "[0 0.5]")], "box": BOX, "content": lc.place("Im0", BOX) + lc.place("Im1", BOX)})


@pytest.mark.parametrize("entries, reason", [
    ("/Type /ExtGState /SA true /OP false /op false /OPM 1 /CA 1 /ca 1.0 /BM /Normal /SMask /None /AIS false", None),
    ("/BM /Compatible", None),
    ("/ca 0.5", "ExtGState /ca 0.5 (constant alpha)"),
    ("/CA 0.5", "ExtGState /CA 0.5 (constant alpha)"),
    ("/BM /Multiply", "ExtGState /BM Multiply (blend mode)"),
    ("/SMask << /S /Alpha >>", "ExtGState /SMask"),
    ("/AIS true", "ExtGState /AIS true"),
    ("/LW 2", "ExtGState /LW"),
])
def test_extgstate(entries, reason):
    d = _strips(lambda c: b"/GS0 gs\n" + c)
    data = pc.document([d]).replace(b"/Resources << /XObject", b"/Resources << /ExtGState << /GS0 << %s >> >> /XObject" % entries.encode())
    data = _fix_xref(data)   # (the page object grew)
    (e,) = pp.read_pages(data, layers=True)
    if reason is None:
        assert isinstance(e, pp.PageLayers), getattr(e, "reason", e)
    else:
        assert isinstance(e, pp.PdfRefused) and e.reason == reason


def _fix_xref(data: bytes) -> bytes:
    """a classic cross-reference table written anew for a file whose objects moved"""
    import re
    body = data[:data.rindex(b"xref\n")]
    offs = {int(m.group(1)): m.start() for m in re.finditer(rb"(?m)^(\d+) 0 obj\n", body)}
    out = bytearray(body)
    at = len(out)
    out += pc._table(offs, max(offs) + 1) + b"trailer\n<< /Size %d /Root 1 0 R >>\nstartxref\n%d\n%%%%EOF\n" % (max(offs) + 1, at)
    return bytes(out)


def test_fill_colour_operators_and_the_state_stack():
    small = _page()[:60, :50]
    gray = lc.gray_obj(small[:, :, 0].copy())
    st = lc.stencil_obj((small[:, :, 0] >= 128).astype(np.uint8))
    c = (lc.place("Im0", BOX) + b"\n" + lc.place("Im1", BOX) + b"\nq 0.5 g " + lc.place("Im1", BOX) + b" Q " + lc.place("Im1", BOX)
         + b"\n/DeviceRGB cs " + lc.place("Im1", BOX) + b" 1 0.5 0 sc " + lc.place("Im1", BOX) + b"\n/DeviceGray cs 1 scn " + lc.place("Im1", BOX))
    e = _one({"image": [gray, st], "box": BOX, "content": c})
    assert [l.fill for l in e.layers[1:]] == [(0, 0, 0), (128, 128, 128), (0, 0, 0), (0, 0, 0), (255, 128, 0), (255, 255, 255)]
    assert "malformed fill colour" == _reason({"image": [gray, st], "box": BOX, "content": lc.place("Im0", BOX) + b" 1 0 0 sc " + lc.place("Im1", BOX)})


# ---- layers=False: today's answers ----
def _files():
    fi = lc.first_image_numbers([3, 2, 3, 3, 1])
    pages = [lc.strips_page(_page(), CUTS[3], ["rgb", "gray", "g4"])[0], lc.mixed_raster_page()[0], lc.smask_page(fi[2], False)[0],
             lc.mask_page(fi[3])[0], {"image": lc.gray_obj(_page()[:, :, 0].copy()), "box": BOX,
                                      "content": pc.page_content(*BOX) + b"\nBT 3 Tr (x) Tj ET"}]
    return pc.document(pages)


def test_layers_off_gives_todays_answers():
    got = pp.read_pages(_files())
    assert [e.reason for e in got] == ["several images on the page", "content operator 'rg'", "several images on the page",
                                       "several images on the page", "text operators on the page (BT)"]
    assert [e.reason for e in pp.read_pages(_files(), False, False)] == [e.reason for e in got]
    one = pc.document([{"image": lc.stencil_obj(np.zeros((4, 4), np.uint8)), "box": BOX}])
    assert pp.read_pages(one)[0].reason == "/ImageMask"
    on = pp.read_pages(_files(), layers=True)
    assert [type(e).__name__ for e in on] == ["PageLayers"] * 4 + ["PageImage"]


# ---- damage ----
def _damage_region(data: bytes):
    """the byte ranges of the content stream and the image dictionaries (from `<<` to `stream`) of a one-page file"""
    import re
    spans = []
    for m in re.finditer(rb"(?m)^(\d+) 0 obj\n", data):
        if int(m.group(1)) < 4:
            continue
        s = data.index(b"stream\n", m.end())
        if int(m.group(1)) == 4:
            spans.append((m.end(), data.index(b"endstream", s)))   # the content stream with its dictionary
        else:
            spans.append((m.end(), s))
    return spans


@pytest.mark.parametrize("which", ["strips", "mixed"])
def test_damage_is_refused_or_yields_safe_rectangles(which):
    small = _page()[:48, :40]
    d = lc.strips_page(small, [1, 30], ["rgb", "gray", "g4"])[0] if which == "strips" else _small_mixed()
    data = pc.document([d])
    variants = 0
    for s, e in _damage_region(data):
        for at in range(s, e):
            muts = [data[:at] + data[at + 1:]] + [data[:at] + bytes([data[at] ^ (1 << b)]) + data[at + 1:] for b in range(8)]
            for mut in muts:
                variants += 1
                try:
                    entries = pp.read_pages(mut, layers=True)
                except pp.PdfRefused:
                    continue
                for en in entries:
                    if isinstance(en, pp.PageLayers):
                        assert 0 < en.width <= 65535 and 0 < en.height <= 65535 and en.width * en.height <= pp.MAX_CANVAS_PIXELS
                        assert len(en.layers) <= pp.MAX_LAYERS
                        assert _rects_ok(en), (at, en)
                    else:
                        assert isinstance(en, (pp.PageImage, pp.PdfRefused))
    assert variants > 3000


def _rects_ok(en) -> bool:
    """compose_params_ok's twin over the record's rectangles and sizes (no pixel is decoded: shapes stand for the images)"""
    class Shape:
        ndim = 3
        def __init__(self, r):
            self.shape = (r.height, r.width, 3)
    table = [(0, l.kind, l.rect, l.flip, l.fill, None if l.image is None else Shape(l.image), None if l.mask is None else Shape(l.mask)) for l in en.layers]
    return lr.compose_params_ok(table, 1, en.height, en.width)


def _small_mixed():
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (14, 10, 3), dtype=np.uint8)
    bits = rng.integers(0, 2, (42, 30), dtype=np.uint8)
    content = lc.place("Im0", BOX) + b"\n" + lc.FILL.encode() + b"\n" + lc.place("Im1", BOX)
    return {"image": [lc.rgb_obj(bg), lc.stencil_obj(bits)], "box": BOX, "content": content}
