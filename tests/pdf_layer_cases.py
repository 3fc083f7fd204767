"""Writers for the layered scanned pages utils/pdf_pages.py reads with layers=True (strips, a stencil over a background, /SMask, a /Mask
stream, invisible text) and for the pages it refuses, on top of pdf_cases.document / image_obj; a host decoder for the records the
reader returns, so that reader + restatement (pdf_layers_reference.compose) can be held against the source bitmap without a GPU."""
import io
import zlib

import numpy as np
from PIL import Image

import ccitt_cases as cc
import pdf_cases as pc
import pdf_layers_reference as lr
from lumina_ocr import synth
from lumina_ocr.utils import pdf_pages as pp

W, H = 700, 1000
BOX = (252, 360)
FILL = "0.1 0.2 0.6 rg"
FILL8 = (26, 51, 153)   # floor(v * 255 + 0.5)
ALPHAS = (0, 1, 127, 128, 254, 255)


def source_page(seed: int = 31, h: int = H, w: int = W) -> np.ndarray:
    return synth.synth_page(h, w, seed, n_lines=12)[0]


# ---- image XObjects ----
def rgb_obj(a: np.ndarray, extra: str = "") -> bytes:
    h, w = a.shape[:2]
    return pc.image_obj(w, h, "/FlateDecode", zlib.compress(pc.png_filter_rows(a.reshape(h, -1), 3, [1, 2, 4]), 6), cs="/DeviceRGB",
                        parms="<< /Predictor 15 /Colors 3 /BitsPerComponent 8 /Columns %d >>" % w, extra=extra)


def gray_obj(g: np.ndarray, extra: str = "") -> bytes:
    h, w = g.shape
    return pc.image_obj(w, h, "/FlateDecode", zlib.compress(g.tobytes(), 6), extra=extra)


def g4_obj(black: np.ndarray, extra: str = "") -> bytes:
    h, w = black.shape
    return pc.image_obj(w, h, "/CCITTFaxDecode", cc.g4_encode(black), bits=1, parms="<< /K -1 /Columns %d /Rows %d >>" % (w, h), extra=extra)


def bits_obj(bits: np.ndarray, extra: str = "", cs: str = "/DeviceGray") -> bytes:
    """a 1-bit Flate image of the samples `bits` (0 | 1)"""
    h, w = bits.shape
    return pc.image_obj(w, h, "/FlateDecode", zlib.compress(pc.pack_bits(bits, 1).tobytes(), 6), cs=cs, bits=1, extra=extra)


def stencil_obj(bits: np.ndarray, decode: str = "", g4: bool = False, bpc: int = 1, extra: str = "") -> bytes:
    """an /ImageMask image of the samples `bits` (0 | 1; with the default /Decode a 0 is painted), Flate or Group 4 (coded black = sample 0)"""
    h, w = bits.shape
    if g4:
        filt, parms, data = "/CCITTFaxDecode", "/DecodeParms << /K -1 /Columns %d /Rows %d >>" % (w, h), cc.g4_encode(bits == 0)
    else:
        filt, parms = "/FlateDecode", ""
        data = zlib.compress((pc.pack_bits(bits, 1) if bpc == 1 else (bits * 255).astype(np.uint8)).tobytes(), 6)
    e = "/Type /XObject /Subtype /Image /Width %d /Height %d /ImageMask true /BitsPerComponent %d /Filter %s %s %s %s" % (
        w, h, bpc, filt, parms, ("/Decode " + decode) if decode else "", extra)
    return pc.stream_obj(e, data)


def place(name: str, box, x0=0.0, y0=0.0, x1=None, y1=None) -> bytes:
    """q cm Do Q of an image over [x0, x1] x [y0, y1] of the box, in user space (y upwards)"""
    x1, y1 = box[0] if x1 is None else x1, box[1] if y1 is None else y1
    return b"q %.8f 0 0 %.8f %.8f %.8f cm /%s Do Q\n" % (x1 - x0, y1 - y0, x0, y0, name.encode())


# ---- pages: (page dict for pc.document, expected bitmap or None) ----
def strips_page(page: np.ndarray, cuts, codings, box=BOX, reverse: bool = False, attrs: str = ""):
    """the page cut into bands at rows `cuts`, band k coded as codings[k % len]: "rgb" (Flate, predictor 15), "gray" (8-bit Flate),
    "g4" (Group 4).  A grey or bilevel band shows the page's luma / its ink, so the expected bitmap is returned with the page."""
    h, w = page.shape[:2]
    edges = [0] + list(cuts) + [h]
    want = page.copy()
    images, content = [], []
    for k, (r0, r1) in enumerate(zip(edges[:-1], edges[1:])):
        band, coding = page[r0:r1], codings[k % len(codings)]
        if coding == "rgb":
            images.append(rgb_obj(band))
        elif coding == "gray":
            g = band[:, :, 1].copy()
            images.append(gray_obj(g))
            want[r0:r1] = g[:, :, None]
        else:
            black = band.mean(axis=2) < 128
            images.append(g4_obj(black))
            want[r0:r1] = np.where(black, 0, 255).astype(np.uint8)[:, :, None]
        content.append(place("Im%d" % k, box, y0=box[1] * (h - r1) / h, y1=box[1] * (h - r0) / h))
    if reverse:
        content.reverse()
    return {"image": images, "box": box, "content": b"\n".join(content), "attrs": attrs}, want


def background_and_bits(seed: int = 32):
    """(background 334 x 233 RGB, text samples 1002 x 699: 0 where the full-resolution page has ink)"""
    bg = source_page(seed, 334, 233)
    bits = (source_page(seed + 1, 1002, 699).mean(axis=2) >= 128).astype(np.uint8)
    return bg, bits


def mixed_raster_page(decode: str = "", g4: bool = False, box=BOX, seed: int = 32, attrs: str = ""):
    """a low-resolution colour background under a full-resolution stencil painted in FILL"""
    bg, bits = background_and_bits(seed)
    paint = (bits == 0) if decode in ("", "[0 1]") else (bits == 1)
    want = np.where(paint[:, :, None], np.asarray(FILL8, np.uint8), np.repeat(np.repeat(bg, 3, axis=0), 3, axis=1))
    content = place("Im0", box) + b"\n" + FILL.encode() + b"\n" + place("Im1", box)
    return {"image": [rgb_obj(bg), stencil_obj(bits, decode, g4)], "box": box, "content": content, "attrs": attrs}, want.astype(np.uint8)


def alpha_plane(h: int, w: int) -> np.ndarray:
    """8-bit alpha that holds every value of ALPHAS in every 6 columns, and whole rows of each"""
    a = np.asarray(ALPHAS, np.uint8)[(np.arange(w)[None, :] + np.arange(h)[:, None] // 7) % len(ALPHAS)]
    return np.ascontiguousarray(a)


def smask_page(first_img: int, one_bit: bool, decode: str = "", box=BOX, seed: int = 34, mask_extra: str = ""):
    """a full-resolution background, then a foreground of a third of its resolution with an /SMask of the full resolution.
    first_img: the object number pc.document gives the page's first image (the /SMask is referenced by number).
    -> (page dict, background, foreground, alpha 0..255 as the mask's samples read before /Decode)"""
    bg, fg = source_page(seed, 1002, 699), source_page(seed + 1, 334, 233)
    if one_bit:
        bits = (source_page(seed + 2, 1002, 699).mean(axis=2) >= 128).astype(np.uint8)
        alpha, mask = bits * 255, bits_obj(bits, extra=("/Decode " + decode if decode else "") + mask_extra)
    else:
        alpha = alpha_plane(1002, 699)
        mask = gray_obj(alpha, extra=("/Decode " + decode if decode else "") + mask_extra)
    images = [rgb_obj(bg), rgb_obj(fg, extra="/SMask %d 0 R" % (first_img + 2)), mask]
    content = place("Im0", box) + b"\n" + place("Im1", box)
    return {"image": images, "box": box, "content": content}, bg, fg, alpha


def mask_page(first_img: int, decode: str = "", box=BOX, seed: int = 37, mask=None):
    """a background, then a foreground with an explicit /Mask stream (a sample that reads 1 after /Decode is masked out)
    -> (page dict, expected bitmap)"""
    bg, fg = source_page(seed, 1002, 699), source_page(seed + 1, 334, 233)
    bits = (source_page(seed + 2, 1002, 699).mean(axis=2) >= 128).astype(np.uint8)
    out = (bits == 1) if decode in ("", "[0 1]") else (bits == 0)
    want = np.where(out[:, :, None], bg, np.repeat(np.repeat(fg, 3, axis=0), 3, axis=1))
    images = [rgb_obj(bg), rgb_obj(fg, extra="/Mask %s" % (mask or "%d 0 R" % (first_img + 2))), stencil_obj(bits, decode)]
    content = place("Im0", box) + b"\n" + place("Im1", box)
    return {"image": images, "box": box, "content": content}, want.astype(np.uint8)


def first_image_numbers(counts):
    """the object number of each page's first image in pc.document, from the pages' image counts"""
    out, num = [], 3
    for c in counts:
        out.append(num + 2)
        num += 2 + c
    return out


# ---- the records on the host ----
def decode_record(rec: pp.PageImage) -> np.ndarray:
    """what the device decoders write for the record: uint8 [h][w][3]"""
    w, h, q = rec.width, rec.height, rec.params
    if rec.filter == "DCTDecode":
        return np.asarray(Image.open(io.BytesIO(bytes(rec.stream))).convert("RGB"))
    if rec.filter == "CCITTFaxDecode":
        assert q["K"] < 0 and not q["EncodedByteAlign"]
        bits = cc.libtiff_bits(bytes(rec.stream), w, h) ^ int(q["BlackIs1"]) ^ int(q["invert"])
        return np.repeat((bits * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    assert rec.filter == "FlateDecode" and not q["indexed"] and q["bits"] in (1, 8) and q["predictor"] in (1, 15)
    data = zlib.decompress(bytes(rec.stream))
    if q["predictor"] >= 10:
        data = pp._png_unpredict(data, w, q["components"], q["bits"])
    rb = (w * q["components"] * q["bits"] + 7) // 8
    rows = np.frombuffer(data, np.uint8)[:rb * h].reshape(h, rb)
    if q["bits"] == 1:
        rows = np.unpackbits(rows, axis=1)[:, :w] * 255
    a = rows.reshape(h, w, q["components"])
    if q["invert"]:
        a = 255 - a
    return np.ascontiguousarray(np.broadcast_to(a, (h, w, 3)) if q["components"] == 1 else a).astype(np.uint8)


def layer_table(entry: pp.PageLayers, page: int = 0, decode=decode_record):
    """the page's layers as the tuples pdf_layers_reference.compose and Engine.page_compose take"""
    return [(page, l.kind, l.rect, l.flip, l.fill, None if l.image is None else decode(l.image), None if l.mask is None else decode(l.mask))
            for l in entry.layers]


def render(entry) -> np.ndarray:
    """the bitmap of one accepted page: its image, or its layers through the restatement"""
    if isinstance(entry, pp.PageImage):
        return decode_record(entry)
    assert isinstance(entry, pp.PageLayers), entry
    return lr.compose((entry.height, entry.width), 1, layer_table(entry))[0]
