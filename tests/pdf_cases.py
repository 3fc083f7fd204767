"""A small PDF writer for the tests of utils/pdf_pages.py and the provider's scanned-PDF path: what Pillow's writer never emits (Flate
images with predictors, xref streams, object streams, inherited attributes, Indexed colour, /Decode, incremental updates, refusals)."""
import io
import struct
import zlib

import numpy as np
from PIL import Image


def stream_obj(entries: str, data: bytes) -> bytes:
    return b"<< %s /Length %d >>\nstream\n" % (entries.encode("latin-1"), len(data)) + data + b"\nendstream"


def image_obj(width, height, filt, data, cs="/DeviceGray", bits=8, parms="", extra="") -> bytes:
    e = "/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace %s /BitsPerComponent %d /Filter %s %s %s" % (
        width, height, cs, bits, filt, ("/DecodeParms " + parms) if parms else "", extra)
    return stream_obj(e, data)


def page_content(w, h, names=("Im0",), cm=None) -> bytes:
    return b"\n".join(b"q %s cm /%s Do Q" % ((cm or "%g 0 0 %g 0 0" % (w, h)).encode(), n.encode()) for n in names)


def document(pages, tree_attrs="", trailer_extra="", **kw) -> bytes:
    """pages: dicts with image (an image_obj body, or a list of them), box=(w, h) in points, and optionally content (bytes), attrs (str
    added to the page dictionary), media (False: no /MediaBox on the page, it is inherited from tree_attrs).  Objects: 1 catalog,
    2 page tree, then per page: page, content, image(s)."""
    objs = {1: b"<< /Type /Catalog /Pages 2 0 R >>"}
    kids, num = [], 3
    for pg in pages:
        images = pg["image"] if isinstance(pg["image"], list) else [pg["image"]]
        w, h = pg["box"]
        page_num, content_num, first_img = num, num + 1, num + 2
        names = ["Im%d" % k for k in range(len(images))]
        xo = " ".join("/%s %d 0 R" % (n, first_img + k) for k, n in enumerate(names))
        media = "/MediaBox [0 0 %g %g]" % (w, h) if pg.get("media", True) else ""
        objs[page_num] = ("<< /Type /Page /Parent 2 0 R %s /Resources << /XObject << %s >> >> /Contents %d 0 R %s >>"
                          % (media, xo, content_num, pg.get("attrs", ""))).encode()
        content = pg.get("content", page_content(w, h, names, pg.get("cm")))
        objs[content_num] = stream_obj("/Filter /FlateDecode", zlib.compress(content)) if pg.get("deflate_content") else stream_obj("", content)
        for k, body in enumerate(images):
            objs[first_img + k] = body
        kids.append(page_num)
        num = first_img + len(images)
    objs[2] = ("<< /Type /Pages /Count %d /Kids [%s] %s >>" % (len(kids), " ".join("%d 0 R" % k for k in kids), tree_attrs)).encode()
    return serialize(objs, trailer_extra=trailer_extra, **kw)


def _table(offsets, size) -> bytes:
    out = b"xref\n"
    for n in sorted(offsets):
        out += b"%d 1\n%010d 00000 n \n" % (n, offsets[n])
    return out


def serialize(objs, xref="table", objstm=False, trailer_extra="", updates=None) -> bytes:
    """xref: "table" | "stream"; objstm: every non-stream object but the catalog goes into one object stream (needs xref="stream");
    updates: {object number: new body} appended as an incremental update with /Prev (classic tables)."""
    out = bytearray(b"%PDF-1.5\n%\xe2\xe3\xcf\xd3\n")
    offsets, packed = {}, {}
    size = max(objs) + 1
    if objstm:
        assert xref == "stream"
        inside = [n for n in sorted(objs) if b"stream\n" not in objs[n] and n != 1]
        body, head = b"", b""
        for n in inside:
            head += b"%d %d " % (n, len(body))
            body += objs[n] + b"\n"
        stm_num = size
        size += 1
        packed = {n: (stm_num, k) for k, n in enumerate(inside)}
        objs = {n: b for n, b in objs.items() if n not in packed}
        objs[stm_num] = stream_obj("/Type /ObjStm /N %d /First %d /Filter /FlateDecode" % (len(inside), len(head)), zlib.compress(head + body))
    for n in sorted(objs):
        offsets[n] = len(out)
        out += b"%d 0 obj\n" % n + objs[n] + b"\nendobj\n"
    if xref == "table":
        at = len(out)
        out += _table(offsets, size) + ("trailer\n<< /Size %d /Root 1 0 R %s >>\nstartxref\n%d\n%%%%EOF\n" % (size, trailer_extra, at)).encode()
        if updates:
            new = {}
            for n in sorted(updates):
                new[n] = len(out)
                out += b"%d 0 obj\n" % n + updates[n] + b"\nendobj\n"
            at2 = len(out)
            out += _table(new, size) + ("trailer\n<< /Size %d /Root 1 0 R /Prev %d >>\nstartxref\n%d\n%%%%EOF\n" % (size, at, at2)).encode()
        return bytes(out)
    # an xref stream: W [1 4 2], PNG predictor 12 (Up) over 7-byte rows
    xnum = size
    size += 1
    offsets[xnum] = len(out)
    rows = []
    for n in range(size):
        if n in offsets:
            rows.append(struct.pack(">BIH", 1, offsets[n], 0))
        elif n in packed:
            rows.append(struct.pack(">BIH", 2, packed[n][0], packed[n][1]))
        else:
            rows.append(struct.pack(">BIH", 0, 0, 65535 if n == 0 else 0))
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(size, 7).astype(np.int16)
    filtered = np.concatenate([np.full((size, 1), 2, np.int16), (a - np.vstack([np.zeros((1, 7), np.int16), a[:-1]])) & 255], axis=1)
    data = zlib.compress(filtered.astype(np.uint8).tobytes())
    e = "/Type /XRef /Size %d /W [1 4 2] /Root 1 0 R /Filter /FlateDecode /DecodeParms << /Predictor 12 /Columns 7 >> %s" % (size, trailer_extra)
    out += b"%d 0 obj\n" % xnum + stream_obj(e, data) + b"\nendobj\nstartxref\n%d\n%%%%EOF\n" % offsets[xnum]
    return bytes(out)


# ---- image streams ----
def png_filter_rows(rows: np.ndarray, bpp: int, types) -> bytes:
    """uint8 [H][row bytes] -> PNG-filtered rows (filter byte + data), row r with filter types[r % len(types)]"""
    h, rb = rows.shape
    a = rows.astype(np.int32)
    out = bytearray()
    for r in range(h):
        ft = types[r % len(types)]
        cur = a[r]
        up = a[r - 1] if r else np.zeros(rb, np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - up
        elif ft == 3:
            f = cur - ((left + up) >> 1)
        else:
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            f = cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out += bytes([ft]) + (f & 255).astype(np.uint8).tobytes()
    return bytes(out)


def tiff_predict_rows(rows: np.ndarray, comps: int) -> bytes:
    """uint8 [H][W * comps] -> /Predictor 2 rows (each sample minus the same component of the pixel on its left)"""
    a = rows.astype(np.int32).reshape(rows.shape[0], -1, comps)
    d = a.copy()
    d[:, 1:] -= a[:, :-1]
    return (d & 255).astype(np.uint8).tobytes()


def pack_bits(samples: np.ndarray, bits: int) -> np.ndarray:
    """[H][W] samples of `bits` bits -> uint8 [H][ceil(W * bits / 8)], the first sample in the high bits, rows padded with zeros"""
    h, w = samples.shape
    per = 8 // bits
    pad = (-w) % per
    s = np.concatenate([samples.astype(np.uint8), np.zeros((h, pad), np.uint8)], axis=1).reshape(h, -1, per)
    out = np.zeros(s.shape[:2], np.uint8)
    for k in range(per):
        out |= s[:, :, k] << (8 - bits * (k + 1))
    return out


def deflate(data: bytes, kind: str = "dynamic") -> bytes:
    """a zlib stream of stored, fixed-Huffman or dynamic-Huffman blocks"""
    if kind == "stored":
        return zlib.compress(data, 0)
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED if kind == "fixed" else zlib.Z_DEFAULT_STRATEGY)
    return c.compress(data) + c.flush()


def jpeg_bytes(rgb: np.ndarray, quality: int = 90) -> bytes:
    op = io.BytesIO()
    Image.fromarray(rgb).save(op, "JPEG", quality=quality)
    return op.getvalue()
