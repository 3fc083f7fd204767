"""Scanned PDFs with /JBIG2Decode images for the tests of the PDF reader and of the device path: made with the test-side JBIG2 encoder
(tests/jbig2_writer.py) and the helpers of tests/pdf_layer_cases.py.  Pages are small (231 x 330 samples) because the encoder and the
restatement are plain Python."""
import functools

import numpy as np

import jbig2_reference as jr
import jbig2_writer as jw
import pdf_cases as pc
import pdf_layer_cases as lc
import pdf_layers_reference as lr
from lumina_ocr.utils import pdf_pages as pp

BOX = (84, 120)          # points; the full-resolution images are 231 x 330, the low-resolution ones 77 x 110
FULL, LOW = (330, 231), (110, 77)


def jbig2_obj(black, globals_ref=None, decode="", mask=False, split=0, extra=""):
    """(image object body, globals stream body or None): a /JBIG2Decode image of the bitmap `black` (1 = black), a DeviceGray image or
    an /ImageMask; split: that many leading segments go to the globals stream referenced as `globals_ref`"""
    h, w = black.shape
    stream = jw.page(w, h, [dict(bitmap=black[:h // 2], tmpl=3, tpgd=True), dict(bitmap=black[h // 2:], y=h // 2, tmpl=2, tpgd=True)])
    g = None
    if split:
        g, stream = jw.split_globals(stream, split)
    parms = "/DecodeParms << /JBIG2Globals %s >>" % globals_ref if split else ""
    kind = "/ImageMask true" if mask else "/ColorSpace /DeviceGray"
    e = "/Type /XObject /Subtype /Image /Width %d /Height %d %s /BitsPerComponent 1 /Filter /JBIG2Decode %s %s %s" % (
        w, h, kind, parms, ("/Decode " + decode) if decode else "", extra)
    return pc.stream_obj(e, stream), (None if g is None else pc.stream_obj("", g))


def decode_record(rec):
    """pdf_layer_cases.decode_record, with the JBIG2 records decoded by the restatement"""
    if rec.filter != "JBIG2Decode":
        return lc.decode_record(rec)
    st, rgb = jr.decode(bytes(rec.stream), rec.params["globals"], rec.height, rec.width, rec.params["invert"])
    assert st == 0
    return rgb


def render(entry):
    if isinstance(entry, pp.PageImage):
        return decode_record(entry)
    assert isinstance(entry, pp.PageLayers), entry
    return lr.compose((entry.height, entry.width), 1, lc.layer_table(entry, decode=decode_record))[0]


@functools.lru_cache(maxsize=None)
def _ink():
    """the text of a page as a bitmap, 1 = ink"""
    return (lc.source_page(51, *FULL).mean(axis=2) < 128).astype(np.uint8)


def _grey(black):
    return np.repeat(np.where(black, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _upsampled(a):
    return np.repeat(np.repeat(a, 3, axis=0), 3, axis=1)


@functools.lru_cache(maxsize=None)
def files():
    """name -> (PDF bytes, expected bitmap of its one page, whether the page needs layers=True)"""
    ink = _ink()
    out = {}
    first = lc.first_image_numbers([2])[0]
    plain, _ = jbig2_obj(ink)
    out["one_image"] = (pc.document([{"image": plain, "box": BOX}]), _grey(ink), False)
    img, g = jbig2_obj(ink, globals_ref="%d 0 R" % (first + 1), split=2)
    out["one_image_globals"] = (pc.document([{"image": [img, g], "box": BOX, "content": lc.place("Im0", BOX)}]), _grey(ink), False)
    inv, _ = jbig2_obj(ink, decode="[1 0]")
    out["decode_1_0"] = (pc.document([{"image": inv, "box": BOX}]), 255 - _grey(ink), False)
    alone, _ = jbig2_obj(ink, mask=True)
    out["image_mask_alone"] = (pc.document([{"image": alone, "box": BOX}]), _grey(ink), False)
    # a JBIG2 stencil in FILL over a DCT background of a third of its resolution
    bg = lc.source_page(52, *LOW)
    jpeg = pc.jpeg_bytes(bg)
    shown = lc.decode_record(pp.PageImage("DCTDecode", memoryview(jpeg), {"components": 3}, LOW[1], LOW[0], 0))
    stencil, _ = jbig2_obj(ink, mask=True)
    content = lc.place("Im0", BOX) + b"\n" + lc.FILL.encode() + b"\n" + lc.place("Im1", BOX)
    page = {"image": [pc.image_obj(LOW[1], LOW[0], "/DCTDecode", jpeg, cs="/DeviceRGB"), stencil], "box": BOX, "content": content}
    out["stencil_over_dct"] = (pc.document([page]), np.where(ink[:, :, None] == 1, np.asarray(lc.FILL8, np.uint8), _upsampled(shown)).astype(np.uint8), True)
    # a foreground with a JBIG2 /Mask stream: a sample that reads 1 (a white JBIG2 pixel) is masked out
    first = lc.first_image_numbers([3])[0]
    back, fore = lc.source_page(53, *FULL), lc.source_page(54, *LOW)
    mask, _ = jbig2_obj(ink, mask=True)
    page = {"image": [lc.rgb_obj(back), lc.rgb_obj(fore, extra="/Mask %d 0 R" % (first + 2)), mask], "box": BOX,
            "content": lc.place("Im0", BOX) + b"\n" + lc.place("Im1", BOX)}
    out["mask_stream"] = (pc.document([page]), np.where(ink[:, :, None] == 1, _upsampled(fore), back).astype(np.uint8), True)
    # a 1-bit JBIG2 /SMask: alpha 0 at a black JBIG2 pixel (sample 0), 255 at a white one
    smask, _ = jbig2_obj(ink)
    page = {"image": [lc.rgb_obj(back), lc.rgb_obj(fore, extra="/SMask %d 0 R" % (first + 2)), smask], "box": BOX,
            "content": lc.place("Im0", BOX) + b"\n" + lc.place("Im1", BOX)}
    out["smask"] = (pc.document([page]), np.where(ink[:, :, None] == 1, back, _upsampled(fore)).astype(np.uint8), True)
    return out
